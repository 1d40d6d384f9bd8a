"""Shared by the JLA tests: the goldens of the compiled reference
(tests/golden/jla/jla_fixture.tar.xz: inputs from tools/jla_make_fixture.py,
outputs from tools/jla_ref_harness.f90) and in-test synthetic datasets."""
import io
import lzma
import os
import tarfile

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jla", "jla_fixture.tar.xz")
NAMES = ["syn37", "syn70", "syn131", "syn37_diag", "syn5_indef"]
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


def extract(tmpdir):
    """{name: Golden} with the archive extracted under tmpdir."""
    with open(GOLDEN, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    return {n: Golden(os.path.join(str(tmpdir), "jla", n)) for n in NAMES}


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
