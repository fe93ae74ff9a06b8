"""The fluctuation methods of the device generator without a GPU: the numpy restatement (tests/fluctuate_method_cases.py)
of the normal deviate against Python's own AS 241 and against scipy's `ndtri`; the distributions of gauss, gauss+poisson
and scaled_poisson; the independence of the Gaussian block from the Poisson blocks; placement; the identities with the
Poisson generator; the generator's own source (csrc/fluctuate_device.hpp) compiled for the host against the
restatement; and `method=` of pisa_amd/analysis/ensemble.py with a solver that draws through the restatement.
tests/test_gpu_fluctuate_methods.py holds the kernel to the restatement, so what is shown here of the restatement's
distribution is shown of the kernel's.

The gates are those of a correct sampler, as in tests/test_host_fluctuate.py: p >= 1e-4, moments within 5 standard
errors, correlations below 5 / sqrt(N), tail counts within 5 binomial standard errors; the seeds are fixed.

The quantile function against `scipy.special.ndtri`: on the sample of `_quantile_sample` (the lattice's ends, both sides
of every branch edge, 10^4 random lattice points of which a quarter in the far tails) the restatement's worst relative
distance from `ndtri` was measured on the CPU as 3.73 eps, so the gate is NDTRI_EPS = 15 eps (4 times that, 14.9);
Python's own AS 241 shows the same distance.
"""
import math
import os
import statistics
import subprocess

import numpy as np
import pytest
from scipy import integrate, special, stats

from tests import ensemble_cases as ec
from tests import ensemble_mc_cases as emc
from tests import fluctuate_cases as fc
from tests import fluctuate_method_cases as fm
from tests.test_host_fluctuate import _chi2_p

N_TRIALS, N_BINS = 2000, 100
N = N_TRIALS * N_BINS
EPS = fc.EPS
NDTRI_EPS = 15.0
PAIRS = ((0.5, 0.4), (3.0, 1.0), (9.5, 2.0), (37.5, 5.0), (1000.0, 40.0), (2.0, 3.0))      # (mu, sigma)
SHAPES_SEED, SHAPES_STREAM = 1, 3           # the seed of the GPU test's shapes: proved free of marginal entries here


# ------------------------------------------------------------------------------------ the quantile function
def _lattice(k):
    return (np.asarray(k, dtype=np.float64) + 0.5) * 2.0 ** -52


def _quantile_sample():
    rs = np.random.RandomState(7)
    edges = []
    for x in (0.075, 0.925, math.exp(-25.0), 1.0 - math.exp(-25.0)):       # |q| = 0.425 and r = 5, both sides
        k = int(math.floor(x * 2.0 ** 52))
        edges += [k - 2, k - 1, k, k + 1, k + 2]
    k = np.concatenate([[0, 2 ** 52 - 1, 2 ** 51 - 1, 2 ** 51], edges, rs.randint(0, 2 ** 52, 7500, dtype=np.int64),
                        rs.randint(0, 2 ** 20, 1250, dtype=np.int64), 2 ** 52 - 1 - rs.randint(0, 2 ** 20, 1250, dtype=np.int64)])
    return _lattice(k)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_the_open_uniform_and_the_lattice_ends():
    F = np.uint64(0xFFFFFFFF)
    assert fm.unit_open(np.uint64(0), np.uint64(0)) == 2.0 ** -53
    assert fm.unit_open(F, F) == 1.0 - 2.0 ** -53
    assert fm.unit_open(np.uint64(1 << 6), np.uint64(0)) == 2.0 ** -26 + 2.0 ** -53
    z, lo, hi = fm.normal(np.array([2.0 ** -53, 1.0 - 2.0 ** -53, 0.5]))
    assert z[2] == 0.0 and lo[2] == 0.0 and hi[2] == 0.0
    assert z[0] == -z[1] and 8.2095 < z[1] < 8.2096 and lo[1] <= z[1] <= hi[1]
    # the lattice is symmetric about 1/2: u and 1 - u give -z and z, bit for bit
    u = _quantile_sample()
    assert np.array_equal(fm.normal(1.0 - u)[0], -fm.normal(u)[0])


def test_quantile_against_python_and_ndtri():
    u = _quantile_sample()
    z, lo, hi = fm.normal(u)
    central = np.abs(u - 0.5) <= 0.425
    assert np.all(lo <= z) and np.all(z <= hi) and np.array_equal(lo[central], hi[central])
    assert np.all(lo[~central] < hi[~central])
    own = np.array([statistics.NormalDist().inv_cdf(float(x)) for x in u])
    worst_own = float(_ulps(z, own).max())
    ref = special.ndtri(u)
    rel = np.abs(z - ref) / np.abs(ref)
    rel_own = np.abs(own - ref) / np.abs(ref)
    print("against Python's AS 241: %.1f ulps; against ndtri: %.2f eps (Python's own: %.2f eps); window %.1f ulps"
          % (worst_own, rel.max() / EPS, rel_own.max() / EPS, float(_ulps(lo, hi).max())))
    assert worst_own <= 4.0
    assert rel.max() <= NDTRI_EPS * EPS


# ------------------------------------------------------------------------------------------- distributions
def _sample(mu, sigma, method, seed, stream=0):
    """N entries of one (mean, sigma), addressed as a 2000 x 100 launch addresses them"""
    return fm.block(np.full(N_BINS, mu), np.full(N_BINS, sigma), method, N_TRIALS, seed, stream)[0]


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_gauss_distribution(seed):
    for mu, sigma in PAIRS + ((0.0, 1.0),):
        x = _sample(mu, sigma, "gauss", seed)
        z = (x - mu) / sigma
        p = float(stats.kstest(z.ravel(), "norm").pvalue)
        z_mean = (x.mean() - mu) / (sigma / math.sqrt(N))
        z_var = (x.var(ddof=1) - sigma ** 2) / (sigma ** 2 * math.sqrt(2.0 / N))
        print("seed %d mu %g sigma %g: KS p %.4f z(mean) %+.2f z(var) %+.2f" % (seed, mu, sigma, p, z_mean, z_var))
        assert p >= 1e-4 and abs(z_mean) <= 5.0 and abs(z_var) <= 5.0, (seed, mu, sigma, p, z_mean, z_var)
        for cut in (3.0, 4.0):
            q = float(stats.norm.sf(cut))
            for side, n in (("below", int(np.sum(z < -cut))), ("above", int(np.sum(z > cut)))):
                dev = (n - N * q) / math.sqrt(N * q * (1.0 - q))
                print("    %s %g sigma: %d (expected %.1f, %+.2f)" % (side, cut, n, N * q, dev))
                assert abs(dev) <= 5.0, (seed, mu, sigma, cut, side, n)


_PMF = {}


def _gauss_poisson_pmf(mu, sigma):
    """P(k) = integral N(g; mu, sigma) Poisson(k; max(g, 0)) dg, k = lo ... hi -> (lo, pmf)"""
    if (mu, sigma) not in _PMF:
        spread = math.sqrt(max(mu, 0.0) + sigma * sigma)
        lo = max(0, int(math.floor(mu - 12.0 * spread - 12.0)))
        hi = int(math.ceil(max(mu, 0.0) + 12.0 * spread + 30.0))
        a, b = max(mu - 12.0 * sigma, 0.0), mu + 12.0 * sigma
        pts = [mu] if a < mu < b else None
        pmf = np.array([integrate.quad(lambda g, k=k: stats.norm.pdf(g, mu, sigma) * stats.poisson.pmf(k, g), a, b,
                                       points=pts, epsabs=1e-15, epsrel=1e-12, limit=200)[0] for k in range(lo, hi + 1)])
        if lo == 0:
            pmf[0] += stats.norm.cdf(0.0, mu, sigma)
        assert abs(pmf.sum() - 1.0) < 1e-12, (mu, sigma, pmf.sum())
        _PMF[(mu, sigma)] = (lo, pmf)
    return _PMF[(mu, sigma)]


def _chi2_cells(x, lo, pmf):
    """goodness of fit against a pmf on lo ... lo + len - 1: cells merged from the left until each expects >= 5"""
    expect = N * pmf
    seen = np.bincount(np.clip(x, lo, lo + pmf.size - 1).astype(np.int64).ravel() - lo, minlength=pmf.size).astype(np.float64)
    cells_e, cells_o, e, o = [], [], 0.0, 0.0
    for ei, oi in zip(expect, seen):
        e, o = e + ei, o + oi
        if e >= 5.0:
            cells_e.append(e), cells_o.append(o)
            e = o = 0.0
    cells_e[-1] += e
    cells_o[-1] += o
    E, O = np.array(cells_e), np.array(cells_o)
    assert abs(E.sum() - N) < 1e-6 * N and O.sum() == N
    return float(stats.chi2.sf(np.sum((O - E) ** 2 / E), E.size - 1)), E.size


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_gauss_poisson_distribution(seed):
    for mu, sigma in PAIRS:
        lo, pmf = _gauss_poisson_pmf(mu, sigma)
        ks = np.arange(lo, lo + pmf.size, dtype=np.float64)
        m1 = float(np.sum(ks * pmf))
        m2 = float(np.sum((ks - m1) ** 2 * pmf))
        m4 = float(np.sum((ks - m1) ** 4 * pmf))
        x = _sample(mu, sigma, "gauss+poisson", seed)
        assert np.all(x == np.rint(x)) and x.min() >= 0
        p, cells = _chi2_cells(x, lo, pmf)
        z_mean = (x.mean() - m1) / math.sqrt(m2 / N)
        z_var = (x.var(ddof=1) - m2) / math.sqrt((m4 - m2 * m2) / N)
        print("seed %d mu %g sigma %g: cells %d p %.4f z(mean) %+.2f z(var) %+.2f" % (seed, mu, sigma, cells, p, z_mean, z_var))
        assert p >= 1e-4 and abs(z_mean) <= 5.0 and abs(z_var) <= 5.0, (seed, mu, sigma, p, z_mean, z_var)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_scaled_poisson_distribution(seed):
    for mu, sigma in PAIRS:
        s = (sigma * sigma) / mu
        lam = mu / s
        x = _sample(mu, sigma, "scaled_poisson", seed)
        k = np.rint(x / s)                               # value / s is an integer: the value is that integer times s
        assert k.min() >= 0 and np.array_equal(k * s, x)
        p, cells = _chi2_p(k, lam)
        z_mean = (x.mean() - mu) / math.sqrt(sigma ** 2 / N)
        z_var = (k.var(ddof=1) - lam) / math.sqrt((lam + 2.0 * lam * lam) / N)
        print("seed %d mu %g sigma %g (lam %g): cells %d p %.4f z(mean) %+.2f z(var) %+.2f"
              % (seed, mu, sigma, lam, cells, p, z_mean, z_var))
        assert p >= 1e-4 and abs(z_mean) <= 5.0 and abs(z_var) <= 5.0, (seed, mu, sigma, p, z_mean, z_var)
        # mean mu and variance sigma^2, in the map's own units
        assert abs(x.var(ddof=1) - sigma ** 2) <= 5.0 * s * s * math.sqrt((lam + 2.0 * lam * lam) / N)


def _corr(a, b):
    return float(np.corrcoef(np.ravel(a), np.ravel(b))[0, 1])


@pytest.mark.parametrize("mu", (3.0, 50.0))
def test_the_gaussian_block_is_independent_of_the_poisson_blocks(mu):
    sigma = 0.5 * math.sqrt(mu)
    z = _sample(0.0, 1.0, "gauss", 1)                    # mu = 0, sigma = 1: the deviate itself
    assert np.array_equal(z, fm.normal(fm.deviates(*np.meshgrid(np.arange(N_TRIALS), np.arange(N_BINS), indexing="ij"), 0, 1))[0])
    k = _sample(mu, sigma, "gauss+poisson", 1)
    g = np.maximum(mu + sigma * z, 0.0)
    live = g > 0.0
    r = _corr(z[live], ((k - g) / np.sqrt(np.where(live, g, 1.0)))[live])
    print("mu %g: correlation of z with the Poisson residual %+.2f / sqrt(N)" % (mu, r * math.sqrt(live.sum())))
    assert abs(r) < 5.0 / math.sqrt(live.sum())
    # and the Poisson draws of the plain method (the same blocks j = 0, 1, ...) do not know z either
    r = _corr(z, fc.block(np.full(N_BINS, mu), N_TRIALS, 1)[0])
    assert abs(r) < 5.0 / math.sqrt(N)


# ---------------------------------------------------------------------------- placement, identities, edges
@pytest.mark.parametrize("method", fm.METHODS)
def test_placement_one_block_or_several(method):
    mu, sigma = fm.palette_rows(70)
    for T, first in ((23, 0), (23, 2 ** 32 - 23)):
        full = fm.block(mu, sigma, method, T, 9, stream=2, first_trial=first)[0]
        assert np.isnan(full[:, np.isnan(mu)]).all()
        for n in (2, 3):
            parts = np.array_split(np.arange(T), n)
            got = np.concatenate([fm.block(mu, sigma, method, len(p), 9, stream=2, first_trial=first + int(p[0]))[0]
                                  for p in parts])
            assert np.array_equal(got, full, equal_nan=True), (method, T, first, n)
    # the number of bins is not part of an entry either
    assert np.array_equal(fm.block(mu[:17], sigma[:17], method, 5, 9)[0], fm.block(mu, sigma, method, 5, 9)[0][:, :17],
                          equal_nan=True)


def _toy(metric="llh", sumw2=True):
    from pisa_amd.analysis import ensemble as en

    hist, var, points, penalty = ec.toy_grid(metric)
    return en, en.TemplateGrid(hist, var if sumw2 else None, points, None, penalty, metric), hist, var


def test_identities_with_the_poisson_generator():
    mu, sigma = fm.palette_rows(70)
    want, marginal = fc.block(mu, 30, 5, stream=2, first_trial=4)
    got = fm.block(mu, None, "poisson", 30, 5, stream=2, first_trial=4)
    assert np.array_equal(got[0], want, equal_nan=True) and np.array_equal(got[3], marginal)
    zero = fm.block(mu, np.zeros_like(mu), "gauss+poisson", 30, 5, stream=2, first_trial=4)
    assert np.array_equal(zero[0], want, equal_nan=True) and np.array_equal(zero[3], marginal)
    assert np.array_equal(fm.block(mu, np.zeros_like(mu), "gauss", 3, 5)[0], np.tile(mu, (3, 1)), equal_nan=True)
    # scaled_poisson with sigma = sqrt(mu) through the ensemble: the scale is exactly 1 and the call is the poisson call
    en, _, hist, _ = _toy()
    grid = en.TemplateGrid(hist, np.sqrt(hist) ** 2, np.zeros((9, 2)))
    solver = fm.NumpyMethodSolver()
    got = en.pseudo_data(grid, 3, 20, 8, generator="device", solver=solver, method="scaled_poisson")
    assert np.array_equal(got, fc.block(hist[3], 20, 8, stream=3)[0])
    assert np.array_equal(got, en.pseudo_data(grid, 3, 20, 8, generator="device", solver=solver))
    assert solver.calls == [("draw", 20, 3, 0)] * 2


def test_means_and_sigmas_without_a_draw():
    nan, inf = float("nan"), float("inf")
    mu = np.array([nan, 5.0, 5.0, 5.0, 5.0, 2.0 ** 52, 0.0, -1.0, 5.0, 0.0, inf])
    sg = np.array([1.0, -1.0, nan, inf, 1.0, 2.0 ** 50, 1.0, 1.0, 0.0, nan, 1.0])
    g = fm.block(mu, sg, "gauss", 40, 4)[0]
    assert np.isnan(g[:, :4]).all() and np.isfinite(g[:, 4:10]).sum() == 40 * 5 and np.isnan(g[:, 9]).all()
    assert np.all(g[:, 8] == 5.0) and np.any(g[:, 6] < 0.0) and np.all(g[:, 10] == inf)
    gp, _, _, marginal = fm.block(mu, sg, "gauss+poisson", 40, 4)
    assert np.isnan(gp[:, :4]).all() and np.isfinite(gp[:, 4]).all() and np.isnan(gp[:, 9:]).all()
    z5, z7 = (fm.normal(fm.deviates(np.arange(40), np.full(40, b), 0, 4))[0] for b in (5, 7))
    over = 2.0 ** 52 + 2.0 ** 50 * z5 > 2.0 ** 52                                 # g > 2^52 -> NaN
    assert over.any() and not over.all() and np.array_equal(np.isnan(gp[:, 5]), over)
    assert np.all(gp[:, 7][-1.0 + z7 < 0.0] == 0.0)                               # a negative g is clipped, not refused
    assert not marginal[np.isnan(gp)].any()
    sp = fm.block(mu, sg, "scaled_poisson", 40, 4)[0]
    assert np.isnan(sp[:, :4]).all() and np.isfinite(sp[:, 4]).all() and np.all(sp[:, [6, 9]] == 0.0)
    assert np.isnan(sp[:, [7, 8, 10]]).all()                    # mu < 0; sigma == 0 with mu != 0; mu = inf
    assert np.isnan(fm.block([5.0], [1e200], "scaled_poisson", 3, 4)[0]).all()            # sigma sigma overflows


# ------------------------------------------------------------- the generator's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through pisa::fl_fluctuate: (n_bins, n_trials, seed, stream, first_trial, method) as six
// uint64, then the row of means and the row of sigmas; the entries of all cases, one after the other, go to the output
// file; the number of cases that set the status goes to stdout
#include "fluctuate_device.hpp"
#include <stdio.h>
#include <vector>
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t head[6];
    int bad_cases = 0;
    while (fread(head, 8, 6, in) == 6) {
        std::vector<double> mu(head[0]), sigma(head[0]), row(head[0]);
        if (fread(mu.data(), 8, mu.size(), in) != mu.size()) return 3;
        if (fread(sigma.data(), 8, sigma.size(), in) != sigma.size()) return 3;
        bool bad = false;
        for (uint64_t t = 0; t < head[1]; t++) {
            for (uint64_t b = 0; b < head[0]; b++)
                row[b] = pisa::fl_fluctuate((int)head[5], mu[b], sigma[b], (uint32_t)b, (uint32_t)(head[4] + t),
                                            (uint32_t)head[3], (uint32_t)head[2], (uint32_t)(head[2] >> 32), bad);
            fwrite(row.data(), 8, row.size(), out);
        }
        bad_cases += bad;
    }
    fclose(out);
    printf("%d\n", bad_cases);
    return 0;
}
"""


def shape_cases():
    """the shapes of the GPU test: (mu, sigma, T, first_trial) for (T, B) in {1, 2, 65, 257} x {1, 63, 64, 65, 257}"""
    return [fm.palette_rows(B) + (T, 2 ** 32 - T if (T, B) == (65, 65) else 0)
            for T in (1, 2, 65, 257) for B in (1, 63, 64, 65, 257)]


def test_the_generator_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/fluctuate_device.hpp compiled with g++ under ASan + UBSan, without contraction, and run as a program of its
    own on the shapes and the seed of the GPU test for all four methods, and on means and sigmas without a draw: gauss
    inside [lo, hi] (`==` in the central branch), counts `==` on every entry that is not marginal, and none marginal on
    the shapes at this seed"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "fluct_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = [(mu, sg, T, SHAPES_SEED, SHAPES_STREAM, first, method) for method in fm.METHODS
             for mu, sg, T, first in shape_cases()]
    n_shapes = len(cases)
    nan, inf = float("nan"), float("inf")
    mu = np.array([nan, 5.0, 5.0, 5.0, 5.0, 2.0 ** 52, 0.0, -1.0, 5.0, 0.0, inf, 5.0])
    sg = np.array([1.0, -1.0, nan, inf, 1.0, 2.0 ** 50, 1.0, 1.0, 0.0, nan, 1.0, 1e200])
    cases += [(mu, sg, 40, 2 ** 64 - 3, 2 ** 32 - 1, 7, method) for method in fm.METHODS]
    with open(tmp_path / "cases.bin", "wb") as fh:
        for mu, sg, T, seed, stream, first, method in cases:
            fh.write(np.array([mu.size, T, seed, stream, first, fm.METHODS.index(method)], dtype=np.uint64).tobytes())
            fh.write(np.ascontiguousarray(mu, dtype=np.float64).tobytes())
            fh.write(np.ascontiguousarray(sg, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    exact = tails = 0
    for i, (mu, sg, T, seed, stream, first, method) in enumerate(cases):
        want, lo, hi, marginal = fm.block(mu, sg, method, T, seed, stream, first)
        got = got_all[at:at + want.size].reshape(want.shape)
        at += want.size
        both_nan = np.isnan(got) & np.isnan(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (i, method)
        if method == "gauss":
            assert np.all(both_nan | ((lo <= got) & (got <= hi))), (i, T, mu.size)
            exact += int(np.sum(~both_nan & (lo == hi)))
            tails += int(np.sum(~both_nan & (lo != hi)))
        else:
            assert np.all(marginal | (got == want) | both_nan), (i, method, T, mu.size)
        if i < n_shapes:
            assert not (marginal & ~fm.wide_window(mu, sg, method)[None, :]).any(), (method, T, mu.size)
    assert at == got_all.size
    assert exact >= 0.8 * (exact + tails)
    # the palette's scaled_poisson rows hold sigma == 0 with mu != 0 from 6 bins on; the edge rows set it for every
    # method (a negative and an infinite mean for poisson)
    want_bad = sum(1 for mu, sg, T, seed, stream, first, method in cases[:n_shapes]
                   if method == "scaled_poisson" and mu.size > 1) + 4
    assert int(res.stdout) == want_bad


# ------------------------------------------------------------------------------------- the ensemble's plumbing
class _Solver(fm.NumpyMethodSolver):
    """the MC-uncertainty metrics from the restatement of tests/ensemble_mc_cases.py"""

    def best(self, kind, data, expected, sigma2=None, offset=None, k0=0):
        if kind not in ("correct_chi2", "mcllh_mean", "mcllh_eff", "conv_llh"):
            return super().best(kind, data, expected, sigma2, offset, k0)
        self.calls.append(("best", kind, np.shape(data), np.shape(expected)))
        return emc.reduce_matrix(kind, emc.direct_form_mc(kind, data, expected, sigma2), offset, k0)


def test_feldman_cousins_with_a_method_and_the_device_generator():
    metric, method = "mcllh_eff", "gauss+poisson"
    en, grid, hist, var = _toy(metric)
    T, cl, seed = 64, (0.6827, 0.90), 1
    solver = _Solver()
    crit = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device", method=method)
    assert crit.shape == (9, 2) and np.all(crit >= 0) and np.all(crit[:, 1] >= crit[:, 0])
    assert solver.calls[:2] == [("fluctuate", method, T, 0, 0), ("best", metric, (T, hist.shape[1]), hist.shape)]
    assert [c[3] for c in solver.calls if c[0] == "fluctuate"] == list(range(9))
    assert not any(c[0] == "draw" for c in solver.calls)
    for k0 in (0, 5):
        data = en.pseudo_data(grid, k0, T, seed, generator="device", solver=solver, method=" Gauss + Poisson ")
        assert np.array_equal(data, fm.block(hist[k0], np.sqrt(var[k0]), method, T, seed, stream=k0)[0])
        assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver), cl), crit[k0])
    chunked = _Solver()
    got = en.feldman_cousins(grid, metric, T, cl, seed, solver=chunked, generator="device", method=method,
                             chunk_bytes=7 * 8 * hist.shape[1])
    assert np.array_equal(got, crit)
    assert [c[2:] for c in chunked.calls if c[0] == "fluctuate"][:10] == [(min(7, T - f), 0, f) for f in range(0, T, 7)]
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, solver=chunked, generator="device", method=method,
                                             chunk_bytes=1), crit)
    sub = en.feldman_cousins(grid, metric, T, cl, seed, true_points=[7, 2], solver=solver, generator="device", method=method)
    assert np.array_equal(sub, crit[[7, 2]])
    # other pseudo-data than the Poisson method's, which still draws through `draw` alone
    plain = _Solver()
    assert not np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, solver=plain, generator="device"), crit)
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, solver=plain, generator="device", method="poisson"),
                          en.feldman_cousins(grid, metric, T, cl, seed, solver=plain, generator="device"))
    assert not any(c[0] == "fluctuate" for c in plain.calls)


def test_scaled_poisson_row_rules_on_the_device_generator():
    en, grid, hist, var = _toy()
    solver = fm.NumpyMethodSolver()
    got = en.pseudo_data(grid, 2, 10, 6, generator="device", solver=solver, method="scaled_poisson")
    assert solver.calls == [("fluctuate", "scaled_poisson", 10, 2, 0)]
    assert np.array_equal(got, fm.block(hist[2], np.sqrt(var[2]), "scaled_poisson", 10, 6, stream=2)[0])
    k = got / (var[2] / hist[2])
    assert np.all(np.abs(k - np.rint(k)) < 1e-9)
    # a non-zero bin without an error: the whole row takes its Poisson expectation, and that is the poisson call; zero
    # and NaN bins stay 0 and NaN; a grid without sumw2 is a grid of such rows
    h, v = hist.copy(), var.copy()
    h[2, 0], h[2, 1], v[2, 5] = 0.0, np.nan, 0.0
    for g in (en.TemplateGrid(h, v, np.zeros((9, 2))), en.TemplateGrid(h, None, np.zeros((9, 2)))):
        solver = fm.NumpyMethodSolver()
        got = en.pseudo_data(g, 2, 10, 6, generator="device", solver=solver, method="scaled_poisson")
        assert solver.calls == [("draw", 10, 2, 0)]
        assert np.array_equal(got, fc.block(h[2], 10, 6, stream=2)[0], equal_nan=True)
        assert np.all(got[:, 0] == 0.0) and np.isnan(got[:, 1]).all()


def _template_maps(hist, sumw2):
    from pisa_amd.core.map import Map

    binning = [dict(name="x", bin_edges=np.linspace(0.0, 1.0, hist.shape[1] // 4 + 1)),
               dict(name="y", bin_edges=np.linspace(0.0, 1.0, 5))]
    shape = (hist.shape[1] // 4, 4)
    return [Map(name="total", hist=h.reshape(shape), binning=binning, error_hist=np.sqrt(v).reshape(shape))
            for h, v in zip(hist, sumw2)]


@pytest.mark.parametrize("method", fm.METHODS)
def test_host_generator_is_the_loop_over_map_fluctuate(method):
    en, grid, hist, var = _toy()
    rows = [(hist, var, grid)]
    h, v = hist.copy(), var.copy()
    h[4, 1], v[4, 5] = np.nan, 0.0               # a NaN bin; for scaled_poisson the row rule (-> the scale 1)
    rows.append((h, v, en.TemplateGrid(h, v, np.zeros((9, 2)))))
    for h, v, g in rows:
        maps = _template_maps(h, v)
        rs = np.random.RandomState(3)
        want = np.stack([maps[4].fluctuate(method, random_state=rs).nominal_values.ravel() for _ in range(5)])
        assert np.array_equal(en.pseudo_data(g, 4, 5, 3, method=method), want, equal_nan=True)
        assert np.array_equal(en.pseudo_data(g, 4, 5, np.random.RandomState(3), generator="host", method=method), want,
                              equal_nan=True)
    # feldman_cousins: every true point from its own RandomState([seed, k0])
    solver = fm.NumpyMethodSolver()
    crit = en.feldman_cousins(grid, "llh", 12, (0.9,), 1, true_points=[4, 7], solver=solver, method=method)
    for i, k0 in enumerate((4, 7)):
        data = en.pseudo_data(grid, k0, 12, np.random.RandomState([1, k0]), method=method)
        assert np.array_equal(en.critical_values(en.delta_metric(data, grid, "llh", k0, solver), (0.9,)), crit[i])
    assert not any(c[0] in ("draw", "fluctuate") for c in solver.calls)


def test_what_is_refused():
    en, grid, hist, var = _toy()
    assert tuple(en.FLUCTUATE_METHODS) == ("poisson", "scaled_poisson", "gauss", "gauss+poisson")
    plain = fc.NumpyDrawSolver()
    for method in fm.METHODS[1:]:
        with pytest.raises(ValueError, match="fluctuate"):
            en.feldman_cousins(grid, "llh", 8, random_state=1, solver=plain, generator="device", method=method)
        with pytest.raises(ValueError, match="fluctuate"):
            en.pseudo_data(grid, 0, 8, 1, generator="device", solver=plain, method=method)
    assert plain.calls == []
    bare = en.TemplateGrid(hist, None, np.zeros((9, 2)))
    for method in ("gauss", "gauss+poisson"):
        for generator in en.GENERATORS:
            with pytest.raises(ValueError, match="sumw2"):
                en.pseudo_data(bare, 0, 8, 1, generator=generator, solver=fm.NumpyMethodSolver(), method=method)
            with pytest.raises(ValueError, match="sumw2"):
                en.feldman_cousins(bare, "llh", 8, random_state=1, solver=fm.NumpyMethodSolver(), generator=generator,
                                   method=method)
    for generator in en.GENERATORS:
        with pytest.raises(ValueError, match='Map fluctuation method "binomial" not recognized'):
            en.pseudo_data(grid, 0, 8, 1, generator=generator, solver=fm.NumpyMethodSolver(), method="binomial")
        with pytest.raises(ValueError, match="not recognized"):
            en.feldman_cousins(grid, "llh", 8, random_state=1, solver=fm.NumpyMethodSolver(), generator=generator,
                               method="none")
