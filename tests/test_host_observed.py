"""Pseudo-data at nuisances fitted to the observed data without a GPU: the factor and the truth draw of
csrc/fluctuate_device.hpp (`fl_truth_factor`, `fl_truth_mvn`) compiled for the host against the numpy restatement
(tests/observed_cases.py); the factor against np.longdouble, which measures `observed_cases.G_FACTOR`; the identity with
the per-parameter truths of tests/truth_cases.py; the closure of the restatement's truths on their mean and covariance;
and `fit_observed`, `nuisance="profiled"` and `nuisance="fitted"` of pisa_amd/analysis/ensemble.py on both generators
with a solver that runs the restatements.  tests/test_gpu_observed.py holds the kernel to the restatement, so what is
shown here of the restatement's truths is shown of the kernel's.

G_FACTOR, measured here over every covariance kind x every box kind at J = 1 ... 8 (numpy 2.2): 0.224, at J = 4 with the
correlation 0.5 and coordinate 0 dead; `observed_cases.G_FACTOR` holds it rounded up (0.23), in units of eps kappa
max|cov|.  The closure gates are five standard errors of the sample mean and the sample covariance of T = 4096 normal
vectors, sqrt(cov_jj / T) and sqrt((cov_ii cov_jj + cov_ij^2) / T): derived, not tuned; the seed is fixed.
"""
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

from tests import ensemble_cases as ec
from tests import fluctuate_method_cases as fm
from tests import hesse_cases as hc
from tests import observed_cases as oc
from tests import profile_bounded_cases as bc
from tests import truth_cases as tc


# ------------------------------------------------------------------------------------------------- the factor
def _refused_covariances():
    nan, inf = float("nan"), float("inf")
    base = oc.covariance(3, "dense")

    def with_at(i, j, v):
        c = base.copy()
        c[i, j] = c[j, i] = v
        return c

    dead_row = oc.covariance(3, "one-dead")
    dead_row[1, 0] = dead_row[0, 1] = 0.1                       # a dead coordinate with an entry in its row
    return (with_at(0, 1, nan), with_at(2, 2, inf), with_at(1, 1, -1.0), dead_row,
            with_at(0, 1, 1.01 * np.sqrt(base[0, 0] * base[1, 1])),                 # correlation above 1
            np.array([[1.0, 1.0], [1.0, 1.0]]))                                     # singular: the second pivot is 0


def test_the_factor_against_longdouble_and_what_it_refuses():
    from pisa_amd.analysis import ensemble as en

    worst, where = 0.0, None
    for J in range(1, 9):
        for kinds, (mean, cov, lower, upper) in oc.cases(J):
            L = oc.truth_factor(cov)
            dead = np.diagonal(cov) == 0.0
            assert L is not None and np.array_equal(L, np.tril(L)), (J, kinds)
            assert not L[dead, :].any() and not L[:, dead].any() and np.all(np.diagonal(L)[~dead] > 0.0)
            assert np.array_equal(en._truth_factor(cov), L), (J, kinds)            # the host generator's own copy
            exact = oc.truth_factor(cov, np.longdouble)
            assert np.allclose(L, exact.astype(np.float64), rtol=1e-12, atol=0.0)
            r = oc.factor_ratio(cov)
            assert r <= oc.G_FACTOR, (J, kinds, r)
            if r > worst:
                worst, where = r, (J, kinds)
    print("G_FACTOR %.3f at %s" % (worst, where))
    assert worst <= oc.G_FACTOR
    assert worst >= 0.5 * oc.G_FACTOR                # (the figure is this measurement's, not a loose bound)
    for cov in _refused_covariances():
        assert oc.truth_factor(cov) is None and en._truth_factor(cov) is None
    assert oc.truth_factor(np.eye(9)) is None


# ------------------------------------------------------------- the generator's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through pisa::fl_truth_factor, pisa::fl_truth_mvn, pisa::fl_linear_mean and
// pisa::fl_fluctuate, the loops of truth_mvn_kernel and linear_kernel of fluctuate_linear.hip: (J, T, B, seed, stream,
// first_trial, method) as seven uint64, then mean [J], cov [J][J], lower, upper [J], mu0, sigma [B] and R [J][B]; per
// case (factored: 1 or 0) and L [J][J], and where factored eta [T][J], data [T][B] and (exhausted, clipped, bad), all
// as doubles, go to the output file
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
        std::vector<double> mean(J), cov(J * J), lower(J), upper(J), mu0(B), sigma(B), R(J * B), eta(T * J), row(B);
        if (!get(in, mean) || !get(in, cov) || !get(in, lower) || !get(in, upper) || !get(in, mu0) || !get(in, sigma) ||
            !get(in, R))
            return 3;
        double L[pisa::FL_MVN_MAX * pisa::FL_MVN_MAX];
        const double factored = pisa::fl_truth_factor(cov.data(), (int)J, L) ? 1.0 : 0.0;
        fwrite(&factored, 8, 1, out);
        for (uint64_t i = 0; i < J; i++) fwrite(L + i * pisa::FL_MVN_MAX, 8, J, out);
        if (factored == 0.0) continue;
        bool exhausted = false, bad = false;
        double n_clipped = 0.0;
        for (uint64_t t = 0; t < T; t++)
            pisa::fl_truth_mvn((uint32_t)(h[5] + t), stream, k0, k1, mean.data(), L, (int)J, lower.data(), upper.data(),
                               eta.data() + t * J, exhausted);
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


@functools.lru_cache(maxsize=None)
def _cases():
    """(what, J, T, B, seed, stream, first, method, (mean, cov, lower, upper), mu0, sigma, R): the truth shapes of the GPU
    test with every covariance kind x every box kind (one bin of data each), its data shapes with every method, the
    family that exhausts its candidates, and covariances without a factor"""
    out = []
    for T, J in oc.TRUTH_SHAPES:
        for kinds, fit in oc.cases(J):
            out.append(("truth", J, T, 1, oc.SEED, oc.STREAM, oc.first_trial_of(T), "poisson", fit, np.array([5.0]),
                        np.array([1.0]), np.zeros((J, 1))))
    for i, (T, B) in enumerate(oc.DATA_SHAPES):
        mu0, sigma, R, fit = oc.data_case(T, B, i)
        for method in oc.METHODS:
            out.append(("data", R.shape[0], T, B, oc.SEED, oc.STREAM, oc.first_trial_of(T), method, fit, mu0, sigma, R))
    out.append(("exhausted", 3, 5, 2, 2 ** 64 - 3, 2 ** 32 - 1, 7, "gauss", oc.exhausting_case(3), np.array([5.0, 5.0]),
                np.ones(2), np.full((3, 2), 0.1)))
    for cov in _refused_covariances():
        J = cov.shape[0]
        out.append(("refused", J, 2, 1, 1, 0, 0, "poisson", (np.zeros(J), cov, np.full(J, -np.inf), np.full(J, np.inf)),
                    np.array([5.0]), np.array([1.0]), np.zeros((J, 1))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _restated(i):
    """the restatement's truths of case i (computed once, shared by the tests below)"""
    what, J, T, B, seed, stream, first, method, fit, mu0, sigma, R = _cases()[i]
    return oc.truths_mvn(fit[0], oc.truth_factor(fit[1]), fit[2], fit[3], T, seed, stream, first)


def test_the_restatement_meets_the_conditions_of_the_gpu_test():
    """counted by the restatement alone, per shape (T, J) over every covariance kind x every box kind: no trial marginal
    at this seed, none exhausted, and at least 0.8^J of the drawn truths have every live deviate from the central
    branch of AS 241 (0.85 per deviate is the branch's mass), so they are compared with `==`"""
    share = {}
    for i, (what, J, T, B, seed, stream, first, method, fit, mu0, sigma, R) in enumerate(_cases()):
        if what not in ("truth", "data"):
            continue
        tr = _restated(i)
        assert not tr["marginal"].any() and not tr["exhausted"], (what, T, J, B)
        if what == "truth":
            drawn = tr["tries"] > 0
            exact = drawn & (tr["lo"] == tr["hi"]).all(axis=1)
            e, d = share.get((T, J), (0, 0))
            share[T, J] = (e + int(exact.sum()), d + int(drawn.sum()))
    assert set(share) == set(oc.TRUTH_SHAPES)
    for (T, J), (e, d) in share.items():
        assert d > 0 and e >= 0.8 ** J * d, (T, J, e, d)
    assert max(int(_restated(i)["tries"].max()) for i, c in enumerate(_cases()) if c[0] == "truth") > 1   # rejections


def test_the_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/fluctuate_device.hpp compiled with g++ under ASan + UBSan, without contraction, and run as a program of its
    own on the GPU test's shapes: the factor `==` the restatement's, refused where it refuses; every truth inside the
    restatement's window, which is `==` where every live deviate is from the central branch; on the program's own
    truths the data `==` wherever not marginal, none marginal, and the clipped counts equal; the exhausting family
    ends inside its box with the mark"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "observed_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = _cases()
    with open(tmp_path / "cases.bin", "wb") as fh:
        for what, J, T, B, seed, stream, first, method, fit, mu0, sigma, R in cases:
            fh.write(np.array([J, T, B, seed, stream, first, _METHOD_CODE[method]], dtype=np.uint64).tobytes())
            for a in fit + (mu0, sigma, R):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    exact = drawn = clipped_total = 0
    for i, (what, J, T, B, seed, stream, first, method, fit, mu0, sigma, R) in enumerate(cases):
        mean, cov, lower, upper = fit
        factored, L = got_all[at], got_all[at + 1:at + 1 + J * J].reshape(J, J)
        at += 1 + J * J
        want_L = oc.truth_factor(cov)
        assert bool(factored) == (want_L is not None) == (what != "refused"), (i, what)
        if what == "refused":
            continue
        assert np.array_equal(L, want_L), (i, what)
        eta = got_all[at:at + T * J].reshape(T, J)
        data = got_all[at + T * J:at + T * J + T * B].reshape(T, B)
        exhausted, n_clipped, bad = got_all[at + T * J + T * B:at + T * J + T * B + 3]
        at += T * J + T * B + 3
        tr = _restated(i)
        assert bool(exhausted) == tr["exhausted"] == (what == "exhausted") and not bad, (i, what)
        assert np.all((lower[None, :] <= eta) & (eta <= upper[None, :])), (i, what)
        dead = np.diagonal(cov) == 0.0
        assert np.array_equal(eta[:, dead], np.broadcast_to(mean[dead], (T, int(dead.sum()))))
        if what == "exhausted":
            assert np.all(tr["tries"] == oc.ATTEMPTS) and np.all((tr["lo"] <= eta) & (eta <= tr["hi"]))
            continue
        assert not tr["marginal"].any(), (i, T, J)
        assert np.all((tr["lo"] <= eta) & (eta <= tr["hi"])), (i, T, J)
        live = tr["tries"] > 0
        exact += int(np.sum(live & (tr["lo"] == tr["hi"]).all(axis=1)))
        drawn += int(live.sum())
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
    assert exact >= 0.8 ** 8 * drawn and clipped_total > 0


# ----------------------------------------------------------------------------------- identities and the closure
def test_a_diagonal_covariance_without_a_box_gives_the_truths_of_truth_cases():
    for T, J in oc.TRUTH_SHAPES:
        mean, cov, _, _ = oc.case(J, "diagonal", "none")
        first = oc.first_trial_of(T)
        got = oc.truths_mvn(mean, oc.truth_factor(cov), None, None, T, oc.SEED, oc.STREAM, first)
        want = tc.truths(np.sqrt(np.diagonal(cov)), mean, None, None, T, oc.SEED, oc.STREAM, first)
        for key in ("eta", "lo", "hi"):
            assert np.array_equal(got[key], want[key]), (T, J, key)
        assert np.all(got["tries"] == 1) and not got["marginal"].any()
    # and a dead coordinate is the scale 0 of `truths`
    mean, cov, _, _ = oc.case(3, "diagonal", "held")
    got = oc.truths_mvn(mean, oc.truth_factor(cov), None, None, 40, 5, 1)
    want = tc.truths(np.sqrt(np.diagonal(cov)), mean, None, None, 40, 5, 1)
    assert np.array_equal(got["eta"], want["eta"]) and np.all(got["eta"][:, 0] == mean[0])
    # the whole vector is rejected: the accepted candidate of a trial is one attempt's, in every coordinate
    mean, cov, lower, upper = oc.case(3, "diagonal", "one-sided")
    L = oc.truth_factor(cov)
    got = oc.truths_mvn(mean, L, lower, upper, 200, 5, 1)
    assert got["tries"].max() > 1
    for t in np.nonzero(got["tries"] > 1)[0][:5]:
        r = int(got["tries"][t]) - 1
        z = [fm.normal(tc.truth_deviates(np.array([t], dtype=np.uint64), np.array([k]), 1, 5, r))[0][0] for k in range(3)]
        assert np.array_equal(got["eta"][t], mean + np.diagonal(L) * np.array(z))


def test_placement():
    mean, cov, lower, upper = oc.case(3, "dense", "two-sided")
    mu0, sigma = fm.palette_rows(70)
    R = tc.responses(3, 70, mu0)
    for T, first in ((23, 0), (23, 2 ** 32 - 23)):
        full = oc.linear_mvn(mu0, sigma, R, mean, cov, lower, upper, "gauss+poisson", T, 9, 2, first)
        parts = [oc.linear_mvn(mu0, sigma, R, mean, cov, lower, upper, "gauss+poisson", len(p), 9, 2, first + int(p[0]))
                 for p in np.array_split(np.arange(T), 3)]
        assert np.array_equal(np.concatenate([p["data"] for p in parts]), full["data"], equal_nan=True)
        assert np.array_equal(np.concatenate([p["eta"] for p in parts]), full["eta"])
        for other in (oc.linear_mvn(mu0, sigma, R, mean, cov, lower, upper, "gauss+poisson", T, 10, 2, first),
                      oc.linear_mvn(mu0, sigma, R, mean, cov, lower, upper, "gauss+poisson", T, 9, 3, first)):
            assert not np.array_equal(other["eta"], full["eta"])


def test_closure_of_the_restatement():
    mean, cov, T, seed, stream = oc.closure_case()
    tr = oc.truths_mvn(mean, oc.truth_factor(cov), None, None, T, seed, stream)
    assert np.all(tr["tries"] == 1)
    oc.check_closure(tr["eta"], mean, cov)
    assert abs(np.corrcoef(tr["eta"][:, 0], tr["eta"][:, 2])[0, 1] - 0.5) < 0.1


# ------------------------------------------------------------------------------------- the ensemble's plumbing
def _toy(metric="llh", lower=None, upper=None, ips=(10.0, 4.0)):
    """the toy grid of tests/test_host_truth.py (a normalisation with a 10 % Gaussian prior 0.05 above its mean, a tilt
    with a prior of 0.25) and an observed map: one Poisson draw of point 4 at displaced truths"""
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
    observed = np.random.RandomState(5).poisson(hist[4] + 0.04 * R[4, 0] + 0.1 * R[4, 1]).astype(np.float64)
    return en, grid, resp, hist, sumw2, R, observed


def test_fit_observed_is_the_conditional_fit_at_every_point():
    en, grid, resp, hist, sumw2, R, observed = _toy(lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    solver = oc.NumpySolver()
    fit = en.fit_observed(observed, grid, "llh", resp, solver, covariance=True)
    K, J = 9, 2
    assert fit["eta"].shape == (K, J) and fit["status"].shape == (K,) and fit["cov"].shape == (K, J, J)
    assert fit["sigma"].shape == (K, J) and fit["hesse_status"].shape == (K,)
    assert [c[0] for c in solver.calls] == ["profiled_matrix", "hesse"]
    want = solver.profiled_matrix("llh", observed[None, :], hist, R, None, resp.inv_prior_sigma, resp.center, 32,
                                  lower=resp.lower, upper=resp.upper)
    assert np.array_equal(fit["eta"], want["eta"][0]) and np.array_equal(fit["status"], want["status"][0])
    _, info = en.delta_metric(observed, grid, "llh", 3, solver, resp, return_info=True, covariance=True)
    assert np.array_equal(fit["eta"][3], info["eta_at"][0]) and np.array_equal(fit["cov"][3], info["cov_at"][0])
    plain = en.fit_observed(observed[None, :], grid, "llh", resp, solver)
    assert set(plain) == {"eta", "status", "value"} and np.array_equal(plain["eta"], fit["eta"])
    # the data pull the parameters away from nominal
    assert np.all(np.abs(fit["eta"][4] - [0.04, 0.1]) < 4 * fit["sigma"][4]) and np.all(np.abs(fit["eta"][4]) > 0.01)


@pytest.mark.parametrize("method", oc.METHODS)
def test_profiled_is_the_generator_of_prior_with_scale_0(method):
    en, grid, resp, hist, sumw2, R, observed = _toy(lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    solver = oc.NumpySolver()
    eta_obs = en.fit_observed(observed, grid, "llh", resp, solver)["eta"]
    k, T = 5, 12
    sigma = None if method == "poisson" else np.sqrt(sumw2[k])
    kw = dict(method=method, response=resp, nuisance="profiled", observed=observed, return_truth=True)
    solver.calls.clear()
    got, truth = en.pseudo_data(grid, k, T, 8, generator="device", solver=solver, **kw)
    assert [c[0] for c in solver.calls] == ["profiled_matrix", "draw_linear"]
    want = solver.draw_linear(hist[k], R[k], sigma, method, T, 8, k, np.zeros(2), eta_obs[k], resp.lower, resp.upper)
    assert np.array_equal(got, want["data"]) and np.array_equal(truth, np.tile(eta_obs[k], (T, 1)))
    assert np.array_equal(truth, want["eta"])
    # the host generator: the generator of "prior" with scale 0 on the one RandomState -- nothing is drawn for the truths
    got, truth = en.pseudo_data(grid, k, T, 8, solver=solver, **kw)
    rs = np.random.RandomState(8)
    want = np.empty((T, hist.shape[1]))
    for t in range(T):
        eta = en._host_truths(np.zeros(2), eta_obs[k], resp.lower, resp.upper, rs)
        want[t] = en._host_row(en._linear_mean(hist[k], R[k], eta), sigma, method, rs)
    assert np.array_equal(got, want) and np.array_equal(truth, np.tile(eta_obs[k], (T, 1)))
    assert not np.array_equal(got, en.pseudo_data(grid, k, T, 8, method=method))


@pytest.mark.parametrize("method", oc.METHODS)
def test_host_generator_of_fitted_is_the_described_loop(method):
    from scipy.stats import norm, poisson

    lower, upper = np.array([-0.01, -0.5]), np.array([0.1, 0.5])
    en, grid, resp, hist, sumw2, R, observed = _toy(lower=lower, upper=upper)
    solver = oc.NumpySolver()
    k, T = 4, 8
    fit = en.fit_observed(observed, grid, "llh", resp, solver, covariance=True)
    mean, L = fit["eta"][k], oc.truth_factor(fit["cov"][k])
    assert L[1, 0] != 0.0                                            # the fit's covariance is not diagonal
    rs = np.random.RandomState(3)
    want, truth, refused = np.empty((T, hist.shape[1])), np.empty((T, 2)), 0
    for t in range(T):
        while True:
            z0 = rs.standard_normal()
            z1 = rs.standard_normal()
            x = np.array([mean[0] + L[0, 0] * z0, mean[1] + L[1, 0] * z0 + L[1, 1] * z1])
            if np.all((lower <= x) & (x <= upper)):
                break
            refused += 1
        truth[t] = x
        mu = np.maximum(hist[k] + R[k, 0] * x[0] + R[k, 1] * x[1], 0.0)
        if method == "poisson":
            want[t] = poisson.rvs(mu, random_state=rs)
        elif method == "gauss":
            want[t] = norm.rvs(loc=mu, scale=np.sqrt(sumw2[k]), random_state=rs)
        else:
            want[t] = poisson.rvs(np.clip(norm.rvs(loc=mu, scale=np.sqrt(sumw2[k]), random_state=rs), 0, None),
                                  random_state=rs)
    assert refused > 0
    got, eta = en.pseudo_data(grid, k, T, 3, solver=solver, method=method, response=resp, nuisance="fitted",
                              observed=observed, return_truth=True)
    assert np.array_equal(got, want) and np.array_equal(eta, truth)
    assert not any(c[0].startswith("draw") for c in solver.calls)


def test_device_generator_of_fitted_draws_through_draw_linear_mvn():
    en, grid, resp, hist, sumw2, R, observed = _toy(lower=np.array([-0.15, -np.inf]), upper=None)
    solver = oc.NumpySolver()
    got, eta = en.pseudo_data(grid, 5, 20, 8, generator="device", solver=solver, method="gauss+poisson", response=resp,
                              nuisance="fitted", observed=observed, return_truth=True)
    assert [c[0] for c in solver.calls] == ["profiled_matrix", "hesse", "draw_linear_mvn"]
    assert solver.calls[-1] == ("draw_linear_mvn", "gauss+poisson", 20, 5, 0)
    fit = en.fit_observed(observed, grid, "llh", resp, solver, covariance=True)
    want = oc.linear_mvn(hist[5], np.sqrt(sumw2[5]), R[5], fit["eta"][5], fit["cov"][5], [-0.15, -np.inf], None,
                         "gauss+poisson", 20, 8, stream=5)
    assert np.array_equal(got, want["data"]) and np.array_equal(eta, want["eta"])
    assert np.unique(eta[:, 0]).size == 20 and np.unique(eta[:, 1]).size == 20


def test_feldman_cousins_at_the_observed_fit():
    metric, T, cl, seed = "llh", 24, (0.6827, 0.90), 1
    en, grid, resp, hist, sumw2, R, observed = _toy(metric, lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    points = [0, 5]
    fit = en.fit_observed(observed, grid, metric, resp, oc.NumpySolver(), covariance=True)
    results = {}
    for nuisance in ("profiled", "fitted"):
        draw = "draw_linear" if nuisance == "profiled" else "draw_linear_mvn"
        for generator in en.GENERATORS:
            solver = oc.NumpySolver()
            kw = dict(true_points=points, solver=solver, generator=generator, response=resp, nuisance=nuisance,
                      observed=observed)
            crit, info = en.feldman_cousins(grid, metric, T, cl, seed, **kw)
            results[nuisance, generator] = crit
            assert crit.shape == (2, 2) and np.all(crit >= 0) and info["flagged"].shape == (2,)
            assert np.array_equal(info["eta_observed"], fit["eta"][points])
            assert ("cov_observed" in info) == (nuisance == "fitted")
            if nuisance == "fitted":
                assert np.array_equal(info["cov_observed"], fit["cov"][points])
            assert [c[0] for c in solver.calls].count("profiled_matrix") == 1          # fitted once for all points
            assert (draw in [c[0] for c in solver.calls]) == (generator == "device")
            assert not any(c[0] in ("draw", "fluctuate") for c in solver.calls)
            for i, k0 in enumerate(points):
                rs = np.random.RandomState([seed, k0]) if generator == "host" else seed
                data = en.pseudo_data(grid, k0, T, rs, generator=generator, solver=solver, response=resp,
                                      nuisance=nuisance, observed=observed)
                assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver, resp), cl),
                                      crit[i])
            # a subset of true points reproduces the full run's rows
            one, _ = en.feldman_cousins(grid, metric, T, cl, seed, **dict(kw, true_points=[5]))
            assert np.array_equal(one[0], crit[1])
            if generator == "device":
                chunked = oc.NumpySolver()
                got, _ = en.feldman_cousins(grid, metric, T, cl, seed, **dict(kw, solver=chunked),
                                            chunk_bytes=7 * 8 * hist.shape[1])
                assert np.array_equal(got, crit)
                assert [c[2:] for c in chunked.calls if c[0] == draw][:4] == [(7, 0, 0), (7, 0, 7), (7, 0, 14), (3, 0, 21)]
    solver = oc.NumpySolver()
    for generator in en.GENERATORS:
        kw = dict(true_points=points, solver=solver, generator=generator, response=resp)
        fixed, info = en.feldman_cousins(grid, metric, T, cl, seed, **kw)
        prior, _ = en.feldman_cousins(grid, metric, T, cl, seed, nuisance="prior", **kw)
        assert set(info) == {"flagged"}                                  # the keys of the existing modes are unchanged
        for nuisance in ("profiled", "fitted"):
            assert not np.array_equal(results[nuisance, generator], fixed)
            assert not np.array_equal(results[nuisance, generator], prior)
    assert not np.array_equal(results["profiled", "device"], results["fitted", "device"])


class _Tampered(oc.NumpySolver):
    """a solver whose fit of the observed map goes wrong at chosen points"""

    def __init__(self, flag_at=None, nan_at=None, indefinite_at=None, inflate=None):
        super().__init__()
        self.flag_at, self.nan_at, self.indefinite_at, self.inflate = flag_at, nan_at, indefinite_at, inflate

    def profiled_matrix(self, *args, **kw):
        out = super().profiled_matrix(*args, **kw)
        if self.flag_at is not None:
            out["status"] = np.array(out["status"])
            out["status"][0, self.flag_at] |= 1                          # PISA_HIP_PROFILE_NOT_CONVERGED
        return out

    def hesse(self, *args, **kw):
        out = {k: np.array(v) for k, v in super().hesse(*args, **kw).items()}
        if self.nan_at is not None:
            out["cov"][self.nan_at] = np.nan
            out["status"][self.nan_at] |= 4
        if self.indefinite_at is not None:
            out["cov"][self.indefinite_at, 0, 1] = out["cov"][self.indefinite_at, 1, 0] = 1.0
        if self.inflate is not None:
            out["cov"] *= self.inflate
        return out


def test_what_is_refused():
    en, grid, resp, hist, sumw2, R, observed = _toy(lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    solver = oc.NumpySolver()
    for generator in en.GENERATORS:
        kw = dict(generator=generator, solver=solver)
        for nuisance in ("profiled", "fitted"):
            on = dict(kw, nuisance=nuisance, response=resp, observed=observed)
            with pytest.raises(ValueError, match="needs observed"):
                en.pseudo_data(grid, 0, 4, 1, **dict(on, observed=None))
            with pytest.raises(ValueError, match="needs observed"):
                en.feldman_cousins(grid, "llh", 4, random_state=1, **dict(on, observed=None))
            with pytest.raises(ValueError, match="needs response"):
                en.pseudo_data(grid, 0, 4, 1, **dict(on, response=None))
            with pytest.raises(ValueError, match="needs response"):
                en.feldman_cousins(grid, "llh", 4, random_state=1, **dict(on, response=None))
            with pytest.raises(ValueError, match="scaled_poisson"):
                en.pseudo_data(grid, 0, 4, 1, method="scaled_poisson", **on)
            with pytest.raises(ValueError, match="scaled_poisson"):
                en.feldman_cousins(grid, "llh", 4, random_state=1, method="scaled_poisson", **on)
            for bad in (np.stack([observed, observed]), observed[:-1]):
                with pytest.raises(ValueError, match="one observed map"):
                    en.pseudo_data(grid, 0, 4, 1, **dict(on, observed=bad))
                with pytest.raises(ValueError, match="one observed map"):
                    en.feldman_cousins(grid, "llh", 4, random_state=1, **dict(on, observed=bad))
            for metric in en.METRICS[4:]:
                mc_grid = en.TemplateGrid(hist, sumw2, np.zeros((9, 2)), None, None, metric)
                with pytest.raises(ValueError, match="not available for '%s'" % metric):
                    en.pseudo_data(mc_grid, 0, 4, 1, **on)
                with pytest.raises(ValueError, match="not available for '%s'" % metric):
                    en.feldman_cousins(grid, metric, 4, random_state=1, **on)
            other = en.NuisanceResponse(("a",), np.zeros((4, 1, 24)), [1.0])
            with pytest.raises(ValueError, match="does not belong"):
                en.pseudo_data(grid, 0, 4, 1, **dict(on, response=other))
            with pytest.raises(ValueError, match="outside the grid"):
                en.pseudo_data(grid, 9, 4, 1, **on)
        for nuisance in ("fixed", "prior"):
            with pytest.raises(ValueError, match="observed= belongs"):
                en.pseudo_data(grid, 0, 4, 1, response=resp, nuisance=nuisance, observed=observed, **kw)
            with pytest.raises(ValueError, match="observed= belongs"):
                en.feldman_cousins(grid, "llh", 4, random_state=1, response=resp, nuisance=nuisance, observed=observed,
                                   **kw)
        with pytest.raises(ValueError, match="not among"):
            en.pseudo_data(grid, 0, 4, 1, response=resp, nuisance="posterior", observed=observed, **kw)
        with pytest.raises(ValueError, match="not among"):
            en.feldman_cousins(grid, "llh", 4, random_state=1, response=resp, nuisance="posterior", observed=observed,
                               **kw)
    assert solver.calls == []
    assert en.NUISANCE == ("fixed", "prior", "profiled", "fitted")
    # `fit_observed` itself
    for metric in en.METRICS[4:]:
        with pytest.raises(ValueError, match="not available for '%s'" % metric):
            en.fit_observed(observed, grid, metric, resp, solver)
    with pytest.raises(ValueError, match="does not belong"):
        en.fit_observed(observed, grid, "llh", en.NuisanceResponse(("a",), np.zeros((4, 1, 24)), [1.0]), solver)
    with pytest.raises(ValueError, match="profiled_matrix"):
        en.fit_observed(observed, grid, "llh", resp, fm.NumpyMethodSolver())
    with pytest.raises(ValueError, match="hesse"):
        en.fit_observed(observed, grid, "llh", resp, _NoHesse(), covariance=True)
    assert solver.calls == []
    # a solver that cannot draw such data: the method is named
    for nuisance, name, lacking in (("profiled", "draw_linear", _NoDraws()), ("fitted", "draw_linear_mvn", _NoMvn())):
        with pytest.raises(ValueError, match=name + r"\("):
            en.pseudo_data(grid, 0, 4, 1, generator="device", solver=lacking, response=resp, nuisance=nuisance,
                           observed=observed)
        with pytest.raises(ValueError, match=name + r"\("):
            en.feldman_cousins(grid, "llh", 4, random_state=1, generator="device", solver=lacking, response=resp,
                               nuisance=nuisance, observed=observed)
        assert lacking.calls == []
    # a fit that went wrong at a REQUESTED point: the points are named, before any draw
    for generator in en.GENERATORS:
        for nuisance, bad, pattern in (("profiled", _Tampered(flag_at=3), r"status flag at the points \[3\]"),
                                       ("fitted", _Tampered(flag_at=3), r"status flag at the points \[3\]"),
                                       ("fitted", _Tampered(nan_at=3), r"no covariance at the points \[3\]"),
                                       ("fitted", _Tampered(indefinite_at=3), r"no Cholesky factor at the points \[3\]"),
                                       ("fitted", _Tampered(inflate=1e4), "mass")):
            kw = dict(generator=generator, solver=bad, response=resp, nuisance=nuisance, observed=observed)
            with pytest.raises(ValueError, match=pattern):
                en.feldman_cousins(grid, "llh", 4, random_state=1, true_points=[2, 3], **kw)
            with pytest.raises(ValueError, match=pattern):
                en.pseudo_data(grid, 3, 4, 1, **kw)
            assert not any(c[0].startswith("draw") for c in bad.calls)
            if pattern != "mass":
                crit, _ = en.feldman_cousins(grid, "llh", 4, random_state=1, true_points=[2, 4], **kw)
                assert crit.shape == (2, 2)
    with pytest.raises(ValueError, match="'norm'"):
        en.pseudo_data(grid, 3, 4, 1, solver=_Tampered(inflate=1e4), response=resp, nuisance="fitted", observed=observed)
    assert stats.norm.cdf(0.25) - stats.norm.cdf(-0.25) < 0.25


class _NoHesse(tc.NumpyTruthSolver, bc.NumpyBoundedProfileSolver):
    """fits, but has no `hesse`"""


class _NoDraws(hc.NumpyHesseSolver, fm.NumpyMethodSolver):
    """fits and draws plain data, but has neither `draw_linear` nor `draw_linear_mvn`"""


class _NoMvn(tc.NumpyTruthSolver, hc.NumpyHesseSolver):
    """everything but `draw_linear_mvn`"""
