"""Shared by the tests of the alpha, beta-marginalised JLA likelihood: the
goldens of the compiled reference's jla_LnLike with JLA_marginalize = T
(tests/golden/jla/jla_marge.tar.xz: options from tools/jla_make_fixture.py
--archive marge, outputs from tools/jla_marge_ref_harness.f90; the datasets
and mu rows are those of jla_fixture.tar.xz, by name), and a long-double
restatement of the integral on jla_fixture.jla_loglike_longdouble."""
import io
import lzma
import os
import tarfile

import numpy as np

import jla_fixture as jf

GOLDEN = os.path.join(os.path.dirname(jf.GOLDEN), "jla_marge.tar.xz")
CASES = ["syn37_s7", "syn37_s0", "syn70_s2", "syn131_s1", "syn37_diag_s7", "syn5_indef_s2"]
RTOL = 1e-10      # the project's golden tolerance (RTOL of test_gpu_jla.py)


class MargeCase:
    """One golden case: its dataset (a jla_fixture.Golden, for the path and the
    mu rows), the options, and per mu row the reference's -lnL, the grid's
    points and how many of them the reference kept."""

    def __init__(self, d, datasets):
        opt = dict(l.split("=") for l in open(os.path.join(d, "options.txt")).read().split("\n") if l.strip())
        opt = {k.strip(): v.strip() for k, v in opt.items()}
        self.g = datasets[opt["dataset"]]
        self.dataset, self.mu = self.g.dataset, self.g.mu
        self.steps = int(opt["JLA_marge_steps"])
        self.width_alpha, self.width_beta = float(opt["JLA_step_width_alpha"]), float(opt["JLA_step_width_beta"])
        t = np.array([[float(x) for x in l.split()] for l in open(os.path.join(d, "ref.txt")) if l.strip()])
        assert len(t) == len(self.mu)
        self.ref = t[:, 0]
        assert len(set(t[:, 1])) == 1 and len(set(t[:, 2])) == 1
        self.n_points, self.n_kept = int(t[0, 1]), int(t[0, 2])

    @property
    def options(self):
        return dict(steps=self.steps, width_alpha=self.width_alpha, width_beta=self.width_beta)


def extract(tmpdir):
    """{case: MargeCase} with both archives extracted under tmpdir."""
    datasets = jf.extract(tmpdir)
    with open(GOLDEN, "rb") as f:
        tar = tarfile.open(fileobj=io.BytesIO(lzma.decompress(f.read())))
        try:
            tar.extractall(str(tmpdir), filter="data")
        except TypeError:
            tar.extractall(str(tmpdir))
    return {c: MargeCase(os.path.join(str(tmpdir), "jla_marge", c), datasets) for c in CASES}


def marge_longdouble(D, mu, steps, width_alpha, width_beta, center=None):
    """jla_LnLike with JLA_marginalize = T (supernovae_JLA.f90:1207-1217) for one
    mu row in np.longdouble: jla_loglike_longdouble at every grid point, those
    whose V has a non-positive pivot dropped, and a long-double log-sum.
    Returns (-lnL, kept points)."""
    from cosmomc_amd.supernovae import jla_marge_grid
    ld = np.longdouble
    al, be = jla_marge_grid(steps, width_alpha, width_beta, center)
    L = []
    for a, b in zip(al, be):
        v, piv = jf.jla_loglike_longdouble(D, a, b, mu)
        if piv >= 0:
            continue
        assert v != jf.LOGZERO, "the reference stops here (tempG <= 0)"
        L.append(v)
    L = np.array(L, dtype=ld)
    best = L.min()
    return best - np.log(np.sum(np.exp(-L + best)) * ld(width_alpha) * ld(width_beta)), len(L)


def marge_longdouble_rows(D, mu, steps, width_alpha, width_beta):
    """marge_longdouble of every row of mu: ([rows] long double, kept points)."""
    r = [marge_longdouble(D, m, steps, width_alpha, width_beta) for m in mu]
    assert len({k for _, k in r}) == 1
    return np.array([v for v, _ in r], dtype=np.longdouble), r[0][1]
