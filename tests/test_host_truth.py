"""Pseudo-data with drawn nuisance truths without a GPU: the truth draw and the mean of csrc/fluctuate_device.hpp
(`fl_truth`, `fl_linear_mean`) compiled for the host against the numpy restatement (tests/truth_cases.py); the
distribution of the restatement's truths (normal, truncated normal); the mean against the profiled fit's own
expression; and `nuisance="prior"` of pisa_amd/analysis/ensemble.py on both generators with solvers that run the
restatements.  tests/test_gpu_truth.py holds the kernels to the restatement, so what is shown here of the
restatement's distribution is shown of the kernels'.

The statistical gates are those of a correct sampler at T = 65 536 truths: mean and variance within 5 standard errors
of the distribution's own (the normal's 1 / sqrt(T) and sqrt(2 / T) in units of the scale; the truncated normal's from
`scipy.stats.truncnorm`'s moments); the seeds are fixed.
"""
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

from tests import ensemble_cases as ec
from tests import fluctuate_cases as fc
from tests import fluctuate_method_cases as fm
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc
from tests import truth_cases as tc

N_STAT = 65536


# ------------------------------------------------------------- the generator's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through pisa::fl_truth, pisa::fl_linear_mean and pisa::fl_fluctuate, the loops of the two
// kernels of fluctuate_linear.hip: (J, T, B, seed, stream, first_trial, method) as seven uint64, then scale, shift,
// lower, upper [J], mu0, sigma [B] and R [J][B]; per case eta [T][J], data [T][B] and (exhausted, clipped, bad) as
// doubles go to the output file
#include "fluctuate_device.hpp"
#include <stdio.h>
#include <vector>
static bool get(FILE *in, std::vector<double> &v) { return fread(v.data(), 8, v.size(), in) == v.size(); }
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t h[7];
    while (fread(h, 8, 7, in) == 7) {
        const uint64_t J = h[0], T = h[1], B = h[2];
        const uint32_t k0 = (uint32_t)h[3], k1 = (uint32_t)(h[3] >> 32), stream = (uint32_t)h[4];
        std::vector<double> scale(J), shift(J), lower(J), upper(J), mu0(B), sigma(B), R(J * B), eta(T * J), row(B);
        if (!get(in, scale) || !get(in, shift) || !get(in, lower) || !get(in, upper) || !get(in, mu0) ||
            !get(in, sigma) || !get(in, R))
            return 3;
        bool exhausted = false, bad = false;
        double n_clipped = 0.0;
        for (uint64_t t = 0; t < T; t++)
            for (uint64_t j = 0; j < J; j++)
                eta[t * J + j] = pisa::fl_truth((uint32_t)j, (uint32_t)(h[5] + t), stream, k0, k1, scale[j], shift[j],
                                                lower[j], upper[j], exhausted);
        fwrite(eta.data(), 8, eta.size(), out);
        for (uint64_t t = 0; t < T; t++) {
            for (uint64_t b = 0; b < B; b++) {
                bool clipped;
                const double mu = pisa::fl_linear_mean(mu0[b], R.data() + b, (int64_t)B, eta.data() + t * J, (int)J,
                                                       clipped);
                n_clipped += clipped;
                row[b] = pisa::fl_fluctuate((int)h[6], mu, sigma[b], (uint32_t)b, (uint32_t)(h[5] + t), stream, k0, k1,
                                            bad);
            }
            fwrite(row.data(), 8, row.size(), out);
        }
        const double tail[3] = {(double)exhausted, n_clipped, (double)bad};
        fwrite(tail, 8, 3, out);
    }
    fclose(out);
    return 0;
}
"""

_METHOD_CODE = {"poisson": 0, "gauss": 2, "gauss+poisson": 3}


def _cases():
    """(J, T, B, seed, stream, first, method, (scale, shift, lower, upper), mu0, sigma, R): the truth shapes of the
    GPU test with every kind of box (one bin of data each), its data shapes with every method, and a box that no
    candidate enters"""
    out = []
    for T, J in tc.TRUTH_SHAPES:
        for kind in tc.KINDS:
            out.append((J, T, 1, tc.SEED, tc.STREAM, tc.first_trial_of(T), "poisson", tc.priors(J, kind),
                        np.array([5.0]), np.array([1.0]), np.zeros((J, 1))))
    for i, (T, B) in enumerate(tc.DATA_SHAPES):
        mu0, sigma, R, pri = tc.data_case(T, B, i)
        for method in tc.METHODS:
            out.append((R.shape[0], T, B, tc.SEED, tc.STREAM, tc.first_trial_of(T), method, pri, mu0, sigma, R))
    far = (np.array([1.0, 1.0]), np.zeros(2), np.array([40.0, -np.inf]), np.array([np.inf, -40.0]))
    out.append((2, 3, 2, 2 ** 64 - 3, 2 ** 32 - 1, 7, "gauss", far, np.array([5.0, 5.0]), np.ones(2),
                np.full((2, 2), 0.1)))
    return out


def test_the_truth_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/fluctuate_device.hpp compiled with g++ under ASan + UBSan, without contraction, and run as a program of its
    own: truths inside the restatement's window (`==` where the accepted candidate is from the central branch of AS 241,
    at least 0.8 of those drawn), none marginal at the seed of the GPU test's shapes; on the program's own truths the
    data `==` wherever not marginal, none marginal either, and the clipped counts equal"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "truth_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = _cases()
    with open(tmp_path / "cases.bin", "wb") as fh:
        for J, T, B, seed, stream, first, method, pri, mu0, sigma, R in cases:
            fh.write(np.array([J, T, B, seed, stream, first, _METHOD_CODE[method]], dtype=np.uint64).tobytes())
            for a in pri + (mu0, sigma, R):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    exact = drawn = clipped_total = 0
    kinds_seen = set()
    for i, (J, T, B, seed, stream, first, method, pri, mu0, sigma, R) in enumerate(cases):
        eta = got_all[at:at + T * J].reshape(T, J)
        data = got_all[at + T * J:at + T * J + T * B].reshape(T, B)
        exhausted, n_clipped, bad = got_all[at + T * J + T * B:at + T * J + T * B + 3]
        at += T * J + T * B + 3
        tr = tc.truths(*pri, T, seed, stream, first)
        last = i == len(cases) - 1
        assert bool(exhausted) == tr["exhausted"] == last and not bad, i
        assert not tr["marginal"].any(), (i, T, J)
        assert np.all((tr["lo"] <= eta) & (eta <= tr["hi"])), (i, T, J)
        assert np.all((pri[2][None, :] <= eta) & (eta <= pri[3][None, :]) | (pri[0] == 0.0)[None, :])
        assert np.array_equal(eta[:, pri[0] == 0.0], np.broadcast_to(pri[1][pri[0] == 0.0], (T, int((pri[0] == 0.0).sum()))))
        if last:
            assert np.array_equal(eta, np.tile([40.0, -40.0], (T, 1))) and np.all(tr["tries"] == tc.ATTEMPTS)
            continue
        exact += int(np.sum((tr["lo"] == tr["hi"]) & (tr["tries"] > 0)))
        drawn += int(np.sum(tr["tries"] > 0))
        kinds_seen.add((int(tr["tries"].max()) > 1, bool((pri[0] == 0.0).any())))
        want, lo, hi, marginal, want_clipped = tc.block(mu0, sigma, R, eta, method, seed, stream, first)
        both_nan = np.isnan(data) & np.isnan(want)
        assert np.array_equal(np.isnan(data), np.isnan(want)), (i, method)
        assert not marginal.any(), (i, method, T, B)
        assert np.all(both_nan | ((lo <= data) & (data <= hi))), (i, method, T, B)
        if method != "gauss":
            assert np.all(both_nan | (data == want)), (i, method, T, B)
        assert int(n_clipped) == want_clipped
        clipped_total += want_clipped
    assert at == got_all.size
    print("%d truths drawn, %d compared with ==; %d means clipped" % (drawn, exact, clipped_total))
    assert exact >= 0.8 * drawn and clipped_total > 0
    assert kinds_seen >= {(False, False), (True, False), (True, True)}     # rejections happened; scale == 0 was there


# ------------------------------------------------------------------------------------------- distributions
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_truth_distributions(seed):
    """an unbounded truth is normal; a box of +-1 sigma and a box (0, +inf) give the truncated normal's moments"""
    scale, shift = 0.7, 0.3
    for a, b in ((-np.inf, np.inf), (-1.0, 1.0), (-shift / scale, np.inf)):          # the box in units of the scale
        lower, upper = shift + scale * a, shift + scale * b
        tr = tc.truths([scale], [shift], [lower], [upper], N_STAT, seed, stream=seed + 4)
        x = tr["eta"][:, 0]
        assert not tr["exhausted"] and np.all((lower <= x) & (x <= upper))
        z = (x - shift) / scale
        dist = stats.truncnorm(a, b) if np.isfinite(a) or np.isfinite(b) else stats.norm()
        m1, m2 = float(dist.mean()), float(dist.var())
        m4 = float(dist.expect(lambda v: (v - m1) ** 4)) if dist.dist.name == "truncnorm" else 3.0
        z_mean = (z.mean() - m1) / math.sqrt(m2 / N_STAT)
        z_var = (z.var(ddof=1) - m2) / math.sqrt((m4 - m2 * m2) / N_STAT)
        p = float(stats.kstest(z, dist.cdf).pvalue)
        print("seed %d box (%g, %g): z(mean) %+.2f z(var) %+.2f KS p %.4f, at most %d candidates"
              % (seed, a, b, z_mean, z_var, p, int(tr["tries"].max())))
        assert abs(z_mean) <= 5.0 and abs(z_var) <= 5.0 and p >= 1e-4, (seed, a, b, z_mean, z_var, p)
        if not np.isfinite(a):                  # the normal's own gates as the definition states them
            assert abs(z.mean()) <= 5.0 / math.sqrt(N_STAT) and abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / N_STAT)
            assert np.all(tr["tries"] == 1)


def test_truths_are_independent_of_the_data_draws_and_of_each_other():
    T = 20000
    tr = tc.truths(np.ones(3), np.zeros(3), None, None, T, 5, stream=2)["eta"]
    zd = fm.normal(fm.deviates(*np.meshgrid(np.arange(T), np.arange(3), indexing="ij"), 2, 5))[0]     # the bins' deviates
    for a, b in ((tr[:, 0], tr[:, 1]), (tr[:, 1], tr[:, 2]), (tr[:, 0], zd[:, 0]), (tr[:, 1], zd[:, 1]),
                 (tr[:-1, 0], tr[1:, 0])):
        assert abs(float(np.corrcoef(a, b)[0, 1])) < 5.0 / math.sqrt(T)


def test_placement_and_the_identity_with_fluctuate():
    mu0, sigma = fm.palette_rows(70)
    R = tc.responses(3, 70, mu0)
    pri = tc.priors(3, "mixed")
    for method in tc.METHODS:
        for T, first in ((23, 0), (23, 2 ** 32 - 23)):
            full = tc.linear(mu0, sigma, R, *pri, method, T, 9, stream=2, first_trial=first)
            for n in (2, 3):
                parts = [tc.linear(mu0, sigma, R, *pri, method, len(p), 9, stream=2, first_trial=first + int(p[0]))
                         for p in np.array_split(np.arange(T), n)]
                assert np.array_equal(np.concatenate([p["data"] for p in parts]), full["data"], equal_nan=True)
                assert np.array_equal(np.concatenate([p["eta"] for p in parts]), full["eta"])
                assert sum(p["clipped"] for p in parts) == full["clipped"]
            for other in (tc.linear(mu0, sigma, R, *pri, method, T, 10, stream=2, first_trial=first),
                          tc.linear(mu0, sigma, R, *pri, method, T, 9, stream=3, first_trial=first)):
                assert not np.array_equal(other["eta"], full["eta"])
                assert not np.array_equal(other["data"], full["data"], equal_nan=True)
        # every scale and shift 0: the entries of `fluctuate`
        zero = np.zeros(3)
        flat = tc.linear(mu0, sigma, R, zero, zero, None, None, method, 30, 5, stream=2, first_trial=4)
        want = fm.block(mu0, sigma, method, 30, 5, stream=2, first_trial=4)
        assert np.array_equal(flat["data"], want[0], equal_nan=True) and np.array_equal(flat["block"][3], want[3])
        assert flat["clipped"] == 0 and not flat["eta"].any()


def test_the_mean_is_the_expression_of_the_fit():
    """mu_t of the restatement, and of the host generator of ensemble.py, == `profile_cases._mu` bit for bit"""
    from pisa_amd.analysis import ensemble as en

    for J in (1, 3, 8):
        f = pc.family("poisson", 65, 1, 33, J)
        eta = f["eta0"]
        want = pc._mu(f["E"], f["R"], eta[:, None, :])[:, 0, :]
        got, clipped = tc.means(f["E"][0], f["R"][0], eta)
        assert not clipped.any() and np.array_equal(got, want)
        assert np.array_equal(np.stack([en._linear_mean(f["E"][0], f["R"][0], e) for e in eta]), want)
    mu, clipped = tc.means([1.0, np.nan, 1.0, 0.0], np.array([[1.0, 1.0, -1.0, 0.0]]), np.array([[-2.0], [0.5]]))
    assert np.array_equal(mu, [[0.0, np.nan, 3.0, 0.0], [1.5, np.nan, 0.5, 0.0]], equal_nan=True)
    assert np.array_equal(clipped, [[True, False, False, False], [False] * 4])
    assert np.array_equal(en._linear_mean(np.array([1.0, np.nan, 1.0, 0.0]), np.array([[1.0, 1.0, -1.0, 0.0]]), [-2.0]),
                          mu[0], equal_nan=True)


# ------------------------------------------------------------------------------------- the ensemble's plumbing
class _Solver(tc.NumpyTruthSolver, bc.NumpyBoundedProfileSolver):
    """draws through tests/truth_cases.py, fits through tests/profile_bounded_cases.py"""


def _toy(metric="llh", lower=None, upper=None, ips=(10.0, 0.0)):
    """the toy grid of tests/test_host_profiled.py: a normalisation with a 10 % Gaussian prior 0.05 above its mean and a
    free tilt"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    K, B = hist.shape
    x = np.linspace(-1.0, 1.0, B)
    R = np.stack([hist, hist * x[None, :]], axis=1)
    ips = np.array(ips)
    center = np.tile(np.array([[0.05, 0.0]]), (K, 1)) * (ips > 0)
    share = float(np.sum((ips * center[0]) ** 2)) * (1.0 if metric in ("chi2", "mod_chi2") else -0.5)
    prior_at_point = np.full(K, share)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty + prior_at_point, metric)
    resp = en.NuisanceResponse(("norm", "tilt"), R, ips, center, prior_at_point, np.full((K, 2), [1.0, 0.0]),
                               lower=lower, upper=upper)
    return en, grid, resp, hist, sumw2, R


@pytest.mark.parametrize("method", tc.METHODS)
def test_host_generator_is_the_described_loop(method):
    from scipy.stats import norm, poisson

    lower = np.tile(np.array([[-0.15, -np.inf]]), (9, 1))
    upper = np.array([0.1, np.inf])
    en, grid, resp, hist, sumw2, R = _toy(lower=lower, upper=upper, ips=(10.0, 4.0))
    k, T = 4, 6
    rs = np.random.RandomState(3)
    scale, shift = np.array([0.1, 0.25]), np.array([-0.05, 0.0])
    want, truth, refused = np.empty((T, hist.shape[1])), np.empty((T, 2)), 0
    for t in range(T):
        for j in range(2):
            while True:
                x = shift[j] + scale[j] * rs.standard_normal()
                if resp.lower[k, j] <= x <= resp.upper[k, j]:
                    break
                refused += 1
            truth[t, j] = x
        mu = np.maximum(hist[k] + R[k, 0] * truth[t, 0] + R[k, 1] * truth[t, 1], 0.0)
        if method == "poisson":
            want[t] = poisson.rvs(mu, random_state=rs)
        elif method == "gauss":
            want[t] = norm.rvs(loc=mu, scale=np.sqrt(sumw2[k]), random_state=rs)
        else:
            want[t] = poisson.rvs(np.clip(norm.rvs(loc=mu, scale=np.sqrt(sumw2[k]), random_state=rs), 0, None),
                                  random_state=rs)
    assert refused > 0
    got, eta = en.pseudo_data(grid, k, T, 3, method=method, response=resp, nuisance="prior", return_truth=True)
    assert np.array_equal(got, want) and np.array_equal(eta, truth)
    assert np.array_equal(en.pseudo_data(grid, k, T, np.random.RandomState(3), generator="host", method=method,
                                         response=resp, nuisance="prior"), want)
    # "fixed" is the call without the keyword, with or without a response, on both generators
    plain = en.pseudo_data(grid, k, T, 3, method=method)
    assert np.array_equal(en.pseudo_data(grid, k, T, 3, method=method, nuisance="fixed"), plain)
    assert np.array_equal(en.pseudo_data(grid, k, T, 3, method=method, response=resp, nuisance="fixed"), plain)
    data, none = en.pseudo_data(grid, k, T, 3, method=method, response=resp, return_truth=True)
    assert none is None and np.array_equal(data, plain) and not np.array_equal(plain, want)
    dev = en.pseudo_data(grid, k, T, 3, generator="device", solver=_Solver(), method=method)
    assert np.array_equal(en.pseudo_data(grid, k, T, 3, generator="device", solver=_Solver(), method=method,
                                         response=resp, nuisance="fixed"), dev)


def test_device_generator_draws_through_draw_linear():
    en, grid, resp, hist, sumw2, R = _toy(lower=np.array([-0.15, -np.inf]), upper=None)
    solver = _Solver()
    got, eta = en.pseudo_data(grid, 5, 20, 8, generator="device", solver=solver, method="gauss+poisson", response=resp,
                              nuisance="prior", return_truth=True)
    assert solver.calls == [("draw_linear", "gauss+poisson", 20, 5, 0)]
    # the normalisation: N(prior mean, 0.1) about a value 0.05 above the mean, inside its box; the tilt has no prior
    want = tc.linear(hist[5], np.sqrt(sumw2[5]), R[5], [0.1, 0.0], [-0.05, 0.0], [-0.15, -np.inf], None,
                     "gauss+poisson", 20, 8, stream=5)
    assert np.array_equal(got, want["data"]) and np.array_equal(eta, want["eta"])
    assert np.all(eta[:, 1] == 0.0) and np.all(eta[:, 0] >= -0.15) and np.unique(eta[:, 0]).size == 20
    # a shared response [J, B] and a response without a box
    shared = en.NuisanceResponse(("norm",), hist[4:5] * 1.0, [10.0], np.full((9, 1), 0.05))
    got = en.pseudo_data(grid, 2, 7, 8, generator="device", solver=solver, response=shared, nuisance="prior")
    assert np.array_equal(got, tc.linear(hist[2], None, hist[4:5], [0.1], [-0.05], None, None, "poisson", 7, 8,
                                         stream=2)["data"])


def test_feldman_cousins_with_drawn_truths():
    metric, T, cl, seed = "llh", 24, (0.6827, 0.90), 1
    en, grid, resp, hist, sumw2, R = _toy(metric, lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    points = [0, 5]
    for generator in en.GENERATORS:
        solver = _Solver()
        crit, info = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points, solver=solver,
                                        generator=generator, response=resp, nuisance="prior")
        assert crit.shape == (2, 2) and np.all(crit >= 0) and info["flagged"].shape == (2,)
        assert ("draw_linear" in [c[0] for c in solver.calls]) == (generator == "device")
        assert not any(c[0] in ("draw", "fluctuate") for c in solver.calls)
        for i, k0 in enumerate(points):
            rs = np.random.RandomState([seed, k0]) if generator == "host" else seed
            data = en.pseudo_data(grid, k0, T, rs, generator=generator, solver=solver, response=resp, nuisance="prior")
            assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver, resp), cl), crit[i])
        fixed, _ = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points, solver=solver,
                                      generator=generator, response=resp)
        assert not np.array_equal(fixed, crit)
        again, _ = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points, solver=solver,
                                      generator=generator, response=resp, nuisance="fixed")
        assert np.array_equal(again, fixed)
        if generator == "device":
            chunked = _Solver()
            got, _ = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points, solver=chunked,
                                        generator=generator, response=resp, nuisance="prior",
                                        chunk_bytes=7 * 8 * hist.shape[1])
            assert np.array_equal(got, crit)
            assert [c[2:] for c in chunked.calls if c[0] == "draw_linear"][:4] == [(7, 0, 0), (7, 0, 7), (7, 0, 14),
                                                                                   (3, 0, 21)]


def test_what_is_refused():
    en, grid, resp, hist, sumw2, R = _toy()
    solver = _Solver()
    for generator in en.GENERATORS:
        kw = dict(generator=generator, solver=solver)
        with pytest.raises(ValueError, match="needs response"):
            en.pseudo_data(grid, 0, 4, 1, nuisance="prior", **kw)
        with pytest.raises(ValueError, match="needs response"):
            en.feldman_cousins(grid, "llh", 4, random_state=1, nuisance="prior", **kw)
        with pytest.raises(ValueError, match="scaled_poisson"):
            en.pseudo_data(grid, 0, 4, 1, method="scaled_poisson", response=resp, nuisance="prior", **kw)
        with pytest.raises(ValueError, match="scaled_poisson"):
            en.feldman_cousins(grid, "llh", 4, random_state=1, method="scaled_poisson", response=resp, nuisance="prior",
                               **kw)
        with pytest.raises(ValueError, match="not among"):
            en.pseudo_data(grid, 0, 4, 1, response=resp, nuisance="posterior", **kw)
        with pytest.raises(ValueError, match="not among"):
            en.feldman_cousins(grid, "llh", 4, random_state=1, response=resp, nuisance="posterior", **kw)
        for metric in en.METRICS[4:]:
            mc_grid = en.TemplateGrid(hist, sumw2, np.zeros((9, 2)), None, None, metric)
            with pytest.raises(ValueError, match="not available for '%s'" % metric):
                en.pseudo_data(mc_grid, 0, 4, 1, response=resp, nuisance="prior", **kw)
            with pytest.raises(ValueError, match="not available for '%s'" % metric):
                en.feldman_cousins(grid, metric, 4, random_state=1, response=resp, nuisance="prior", **kw)
        other = en.NuisanceResponse(("a",), np.zeros((4, 1, 24)), [1.0])
        with pytest.raises(ValueError, match="does not belong"):
            en.pseudo_data(grid, 0, 4, 1, response=other, nuisance="prior", **kw)
        with pytest.raises(ValueError, match="outside the grid"):
            en.pseudo_data(grid, 9, 4, 1, response=resp, nuisance="prior", **kw)
    # a solver that cannot draw such data: the method is named
    plain = fm.NumpyMethodSolver()
    with pytest.raises(ValueError, match="draw_linear"):
        en.pseudo_data(grid, 0, 4, 1, generator="device", solver=plain, response=resp, nuisance="prior")
    with pytest.raises(ValueError, match="draw_linear"):
        en.feldman_cousins(grid, "llh", 4, random_state=1, generator="device", solver=plain, response=resp,
                           nuisance="prior")
    assert plain.calls == [] and solver.calls == []
    # a box with less than a quarter of the prior's mass: the normalisation's prior is N(-0.05, 0.1) in eta
    far = _toy(lower=np.array([0.05, -np.inf]), upper=None)[2]
    assert stats.norm.sf(1.0) < 0.25
    with pytest.raises(ValueError, match="mass"):
        en.pseudo_data(grid, 0, 4, 1, response=far, nuisance="prior")
    near = _toy(lower=np.array([0.0, -np.inf]), upper=None)[2]            # sf(0.5) = 0.31: drawn
    assert en.pseudo_data(grid, 0, 4, 1, response=near, nuisance="prior").shape == (4, 24)
