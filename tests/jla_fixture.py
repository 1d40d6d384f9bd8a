"""Shared by the JLA tests: the goldens of the compiled reference
(tests/golden/jla/*.tar.xz: inputs from tools/jla_make_fixture.py, outputs
from tools/jla_ref_harness.f90), in-test synthetic datasets, a long-double
restatement of JLA_alpha_beta_like as their high-precision reference, and the
edge datasets of test_gpu_jla_edges.py with the input conditions that
test_supernovae.py checks without a GPU."""
import atexit
import io
import lzma
import os
import shutil
import tarfile
import tempfile

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "jla_loglike_longdouble needs x87 extended precision"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jla", "jla_fixture.tar.xz")
GOLDEN_UPPER = os.path.join(os.path.dirname(GOLDEN), "jla_upper.tar.xz")
NAMES = ["syn37", "syn70", "syn131", "syn37_diag", "syn5_indef"]
NAMES_UPPER = ["syn21_upper"]
COMPONENTS = ("mag", "stretch", "colour", "mag_stretch", "mag_colour", "stretch_colour")
BLOCK = dict(mag=(0, 0), stretch=(1, 1), colour=(2, 2), mag_stretch=(0, 1), mag_colour=(0, 2), stretch_colour=(1, 2))
LOGZERO = 1e30


class Golden:
    """One golden dataset: its path, the (alpha, beta) and mu of its cases and the reference's -lnL."""

    def __init__(self, d):
        self.dataset = os.path.join(d, "jla.dataset")
        lines = open(os.path.join(d, "cases.txt")).read().split("\n")
        nc = int(lines[0])
        self.ab = np.array([[float(x) for x in lines[1 + 2 * i].split()] for i in range(nc)])
        self.mu = np.array([[float(x) for x in lines[2 + 2 * i].split()] for i in range(nc)])
        self.ref = np.array([float(x) for x in open(os.path.join(d, "ref.txt")).read().split()])
        assert len(self.ref) == nc


def extract(tmpdir, archive=GOLDEN, names=NAMES):
    """{name: Golden} with the archive extracted under tmpdir."""
    with open(archive, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    return {n: Golden(os.path.join(str(tmpdir), "jla", n)) for n in names}


def make_synthetic(d, n, comps, two, seed, fmt="%.17g"):
    """A seeded dataset of n supernovae under directory d, its component
    matrices cut from one jointly positive-semidefinite matrix (so V(alpha,
    beta) is positive definite); returns (dataset path, mu [3][n], ab [3][2])."""
    rng = np.random.RandomState(seed)
    os.makedirs(d, exist_ok=True)
    z = np.sort(rng.uniform(0.01, 1.2, n))
    third = rng.uniform(8.0, 12.0, n)
    if n > 1:
        third[0], third[-1] = 9.0, 11.0      # both scriptm sets populated
    with open(os.path.join(d, "lc.txt"), "w") as f:
        f.write("#name zcmb zhel dz mb dmb x1 dx1 color dcolor 3rdvar d3rdvar cov_m_s cov_m_c cov_s_c set\n")
        for i in range(n):
            mb = 5 * np.log10((1 + z[i]) * z[i] * (1 + 0.5 * z[i]) * 299792.458 / 70) + 25 - 19.05 \
                + 0.1 * rng.standard_normal()
            row = [z[i], z[i] * (1 + 1e-3 * rng.standard_normal()), 0.0, mb, rng.uniform(0.08, 0.2),
                   rng.standard_normal(), rng.uniform(0.1, 0.5), 0.1 * rng.standard_normal(), rng.uniform(0.02, 0.06),
                   third[i], 0.1, 1e-3 * rng.standard_normal(), 1e-4 * rng.standard_normal(),
                   1e-4 * rng.standard_normal()]
            f.write("sn%04d " % i + " ".join(fmt % x for x in row) + " %d\n" % rng.randint(0, 4))
    A = rng.standard_normal((3 * n, 3 * n + 7))
    Jm = A @ A.T / (3 * n + 7)
    sc = np.repeat(np.array([0.02, 0.1, 0.01]), n)
    Jm = Jm * sc[:, None] * sc[None, :]
    with open(os.path.join(d, "jla.dataset"), "w") as f:
        f.write("name = JLAtest\ndata_file = lc.txt\npecz = 0.0005\nintrinsicdisp = 0.1\nintrinsicdisp1 = 0.08\n")
        f.write("twoscriptmfit = %s\nscriptmcut = 10.0\n" % ("T" if two else "F"))
        for k in comps:
            a, b = BLOCK[k]
            M = Jm[a * n:(a + 1) * n, b * n:(b + 1) * n]
            M = (M + M.T) / 2
            with open(os.path.join(d, k + ".dat"), "w") as g:
                g.write("%d\n" % n)
                g.write("\n".join(" ".join(fmt % x for x in r) for r in M) + "\n")
            f.write("has_%s_covmat = T\n%s_covmat_file = %s.dat\n" % (k, k, k))
    mu0 = 5 * np.log10((1 + z) * z * (1 + 0.5 * z) * 299792.458 / 70) + 25
    mu = mu0[None, :] + 0.05 * rng.standard_normal((3, n))
    ab = np.array([[0.141, 3.101], [0.0, 0.0], [-0.05, 3.6]])
    return os.path.join(d, "jla.dataset"), mu, ab


# ------------------------------------------------------------ long-double reference

def jla_loglike_longdouble(D, alpha, beta, mu):
    """JLA_alpha_beta_like (supernovae_JLA.f90:1028-1168) restated in
    np.longdouble on a JLADataset: V(alpha, beta) factored by an unblocked column
    Cholesky with the right-hand sides [diffmag, A1, A2] carried along as three
    extra rows.  Returns (-lnL, index of the first non-positive or NaN pivot, else
    -1); -lnL is LOGZERO where the reference returns it."""
    ld = np.longdouble

    def f(x):
        return np.asarray(x, dtype=np.float64).astype(ld)
    a, b = ld(alpha), ld(beta)
    dv = f(D.pre_vars) + a * a * f(D.stretch_var) + b * b * f(D.colour_var) + 2 * a * f(D.cov_ms) \
        - 2 * b * f(D.cov_mc) - 2 * a * b * f(D.cov_sc)
    iv = 1 / dv
    mag, mu = f(D.mag), f(mu)
    scriptm = np.sum((mag - mu) * iv) / np.sum(iv)
    dm = mag - mu + a * f(D.stretch) - b * f(D.colour) - scriptm
    R = np.stack([dm, f(D.one), f(D.A2)])
    if D.diag_errors:
        G = (R * iv) @ R.T
    else:
        n = D.nsn
        coef = {"mag": ld(1), "stretch": a * a, "colour": b * b, "mag_stretch": 2 * a, "mag_colour": -2 * b,
                "stretch_colour": -2 * a * b}
        M = np.zeros((n + 3, n), dtype=ld)
        M[:n] = np.diag(dv)
        for k in COMPONENTS:
            if k in D.comp:
                M[:n] += coef[k] * f(D.comp[k])
        M[n:] = R
        for j in range(n):
            col = M[j:, j] - M[j:, :j] @ M[j, :j]
            if not col[0] > 0:
                return ld(LOGZERO), j                    # DPOTRF status /= 0 (:1085-1092)
            M[j:, j] = col / np.sqrt(col[0])
        G = M[n:] @ M[n:].T
    A, B, C, E, Dd, F = G[0, 0], G[0, 1], G[0, 2], G[1, 1], G[1, 2], G[2, 2]
    tp = 1 / (2 * ld(np.pi))                             # the reference's twopi is a double constant
    if D.twoscriptmfit:
        g = F - Dd * Dd / E
        if not g > 0:
            return ld(LOGZERO), -1
        chisq = A + np.log(E * tp) + np.log(g * tp) - C * C / g - B * B * F / (E * g) + 2 * B * C * Dd / (E * g)
    else:
        chisq = A + np.log(E * tp) - B * B / E
    return chisq / 2, -1


def rel_distance(x, ref):
    """max |x / ref - 1| against long-double values, formed in long double."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(x, dtype=np.float64).astype(np.longdouble) / ref - 1).max())


def jla_V(D, alpha, beta):
    """V(alpha, beta) of a JLADataset with component matrices, in float64 (for its condition number)."""
    a, b = float(alpha), float(beta)
    V = np.diag(D.pre_vars + a * a * D.stretch_var + b * b * D.colour_var + 2 * a * D.cov_ms - 2 * b * D.cov_mc
                - 2 * a * b * D.cov_sc)
    coef = {"mag": 1.0, "stretch": a * a, "colour": b * b, "mag_stretch": 2 * a, "mag_colour": -2 * b,
            "stretch_colour": -2 * a * b}
    for k, m in D.comp.items():
        V = V + coef[k] * m
    return V


# ------------------------------------------------------------ datasets from explicit arrays

def read_lc(d):
    """(names, rows [n][15]) of the light-curve file make_synthetic wrote under d: the 14 numbers and the set."""
    t = [l.split() for l in open(os.path.join(d, "lc.txt")) if not l.startswith("#")]
    return [r[0] for r in t], np.array([[float(x) for x in r[1:]] for r in t])


def write_dataset(d, names, rows, mats, two, fmt="%.17g", pecz=0.0005, idisp=(0.1, 0.08)):
    """A dataset under d from explicit arrays: light-curve rows as read_lc gives
    them and the component matrices {name: [n][n]} written as they are (no
    symmetrisation), so a test can place single entries.  Returns its path."""
    os.makedirs(d, exist_ok=True)
    n = len(rows)
    with open(os.path.join(d, "lc.txt"), "w") as f:
        f.write("#name zcmb zhel dz mb dmb x1 dx1 color dcolor 3rdvar d3rdvar cov_m_s cov_m_c cov_s_c set\n")
        for nm, r in zip(names, rows):
            f.write(nm + " " + " ".join(fmt % x for x in r[:14]) + " %d\n" % r[14])
    with open(os.path.join(d, "jla.dataset"), "w") as f:
        f.write("name = JLAtest\ndata_file = lc.txt\npecz = %r\nintrinsicdisp = %r\nintrinsicdisp1 = %r\n"
                % (float(pecz), float(idisp[0]), float(idisp[1])))
        f.write("twoscriptmfit = %s\nscriptmcut = 10.0\n" % ("T" if two else "F"))
        for k in COMPONENTS:
            if k not in mats:
                continue
            M = np.asarray(mats[k], dtype=np.float64)
            assert M.shape == (n, n)
            with open(os.path.join(d, k + ".dat"), "w") as g:
                g.write("%d\n" % n)
                g.write("\n".join(" ".join(fmt % x for x in r) for r in M) + "\n")
            f.write("has_%s_covmat = T\n%s_covmat_file = %s.dat\n" % (k, k, k))
    return os.path.join(d, "jla.dataset")


def read_matrix(path):
    """A component matrix file as written, both triangles."""
    with open(path) as f:
        n = int(f.readline())
        return np.array(f.read().split(), dtype=np.float64).reshape(n, n)


# ------------------------------------------------------------ the edge datasets

# (nsn, p).  nsn = 230: Np = 240, T = 15, ten padded rows; p in the first tile, its last row, the next tile's first
# row, mid, a late tile, the last real row of the padded tile.  A block column J has (T - J + 3) / 4 slabs, so four
# at most there; nsn = 257 (T = 17, five slabs while J < 2, one real row in the last tile) adds the waves' second lap.
PIVOT = [(230, p) for p in (0, 15, 16, 100, 223, 229)] + [(257, p) for p in (0, 20, 100, 256)]
PIVOT_S = 3.0                            # V[p, p] drops by alpha^2 PIVOT_S
PIVOT_AB = np.array([[0.2, 1.0], [0.0, 0.0], [0.05, 1.0]])      # not positive definite, and two that are
SLAB_NSN = (230, 257)                    # 5 slabs at J = 0; Np = 272 with one real row in the last tile
SUBSETS = {k: (k,) for k in COMPONENTS}
SUBSETS["nomag"] = ("stretch", "colour", "stretch_colour")
ILL_S, ILL_RHO, ILL_SCALE = 0.15, 1.0 - 1e-6, 1e-2   # mag = s^2 (rho 1 1^T + (1 - rho) I); every error times 1e-2

EDGE_NAMES = ["pivot_%d_%d" % np_ for np_ in PIVOT] + ["slabs_%d_%d" % (n, t) for n in SLAB_NSN for t in (0, 1)] \
    + ["subset_" + k for k in SUBSETS] + ["diag300_0", "diag300_1", "illcond"]


class Edge:
    """One edge dataset: its path, the (alpha, beta) and mu of its cases, and on
    first use its JLADataset and the long-double reference of every case."""

    def __init__(self, dataset, mu, ab):
        self.dataset, self.mu, self.ab = dataset, mu, np.array(ab)
        self._D = self._ref = None

    @property
    def D(self):
        if self._D is None:
            from cosmomc_amd.supernovae import JLADataset
            self._D = JLADataset(self.dataset)
        return self._D

    def _reference(self):
        if self._ref is None:
            r = [jla_loglike_longdouble(self.D, a, b, m) for (a, b), m in zip(self.ab, self.mu)]
            self._ref = (np.array([v for v, _ in r], dtype=np.longdouble), np.array([p for _, p in r]))
        return self._ref

    @property
    def ref(self):
        """-lnL [cases] in long double"""
        return self._reference()[0]

    @property
    def bad(self):
        """first non-positive pivot [cases], -1 where there is none"""
        return self._reference()[1]


_edges = {}
_edge_root = None


def _make_edge(name, d):
    kind, _, arg = name.partition("_")
    if kind == "pivot":
        nsn, p = (int(x) for x in arg.split("_"))
        ds, mu, _ = make_synthetic(d, nsn, ("mag",), True, 10 * nsn)
        names, rows = read_lc(d)
        S = np.zeros((nsn, nsn))
        S[p, p] = -PIVOT_S
        return Edge(write_dataset(d, names, rows, {"mag": read_matrix(os.path.join(d, "mag.dat")), "stretch": S}, True),
                    mu, PIVOT_AB)
    if kind == "slabs":
        nsn, two = (int(x) for x in arg.split("_"))
        return Edge(*make_synthetic(d, nsn, COMPONENTS, bool(two), 10 * nsn + two, fmt="%.9g"))
    if kind == "subset":
        return Edge(*make_synthetic(d, 33, SUBSETS[arg], True, 3300))
    if kind == "diag300":
        return Edge(*make_synthetic(d, 300, (), bool(int(arg)), 3000 + int(arg)))
    if name == "illcond":
        ds, mu, ab = make_synthetic(d, 230, (), True, 2300)
        names, rows = read_lc(d)
        rows[:, [4, 6, 8]] *= ILL_SCALE           # dmb, dx1, dcolor
        rows[:, 11:14] = 0.0                      # cov_m_s, cov_m_c, cov_s_c
        mag = ILL_S ** 2 * (ILL_RHO * np.ones((230, 230)) + (1 - ILL_RHO) * np.eye(230))
        return Edge(write_dataset(d, names, rows, {"mag": mag}, True, pecz=0.0005 * ILL_SCALE,
                                  idisp=(0.1 * ILL_SCALE, 0.08 * ILL_SCALE)), mu, ab)
    raise KeyError(name)


def edge(name):
    """The edge dataset of that name, written once per process under a temporary directory."""
    global _edge_root
    if name not in _edges:
        if _edge_root is None:
            _edge_root = tempfile.mkdtemp(prefix="jla_edges_")
            atexit.register(shutil.rmtree, _edge_root, True)
        _edges[name] = _make_edge(name, os.path.join(_edge_root, name))
    return _edges[name]
