"""`pisa_hip_hypersurface_fit` on the device against the numpy restatement's two measures (tests/hsfit_cases.py):
  stationarity  |H^-1 (-g)|_i <= 1e-6 sqrt(cov_ii) for every free coefficient of every fitted problem
  covariance    |cov - cov_ref|_ij / sqrt(cov_ii cov_jj) <= 1e-10, cov_ref the inverse of the longdouble
                half-Hessian at the returned coefficients
plus: results do not depend on where a problem sits in the batch (bit for bit), the compile-time limits, bounds
and priors, the data rules (NaN, sigma = 0, too few sets), and `fit_hypersurfaces` end to end on planted events.

The seeded families of tests/hsfit_cases.py carry the same gates, and a third (the loss is at most 1e-9 relative above
the restatement's), to every form in both links, the set counts at the wavefront width, more problems than
workgroups, every bound shape, an exact anchor (a linear problem against the 40-digit solution of its normal
equations, tests/golden/hsfit_exact_ref.npz) and every status bit.  tests/test_host_hsfit.py holds the restatement
to a tenth of the gates on each of them first.  Worst figures on an MI355X (gates 1e-6, 1e-10, 1e-9):

  family (tests/hsfit_cases.py)              stationarity  covariance  loss excess  trial points
  forms: 5 forms x 2 links, 64 problems each   5.5e-14       6.6e-14     3.4e-14      <= 21
  sets: 63 / 64 / 65 / 127 / 128, log65,
        unused sets on lanes 63, 64 and last   3.4e-14       1.7e-14     5.3e-15      <= 6
  many: 4096 + 70 (64 distinct problems)       2.6e-14       1.1e-15     2.7e-14      <= 8
  box: six bound shapes, 32 problems each      3.5e-14       1.9e-13     1.8e-14      <= 35
       (loss above scipy's bounded fit: 1.3e-14)
  lin: linear problem, 4 variants              1.2e-12       2.4e-14     1.5e-13      <= 6
       against the 40-digit solution:          9.9e-13       1.9e-14     1.5e-13
  log-edge: min(1 + m x) in [0.03, 0.1]        1.5e-13       9.9e-16     1.4e-14      <= 7
  ill-twin_prior                               3.0e-14       4.2e-13     6.8e-15      <= 7
       against the 40-digit solution:          5.9e-14       8.9e-13     6.8e-15
  scan: exponential_scaled + linear, 2 x 256   status 0: 4.6e-13 (log), 1.9e-13 (identity);
        flagged 12.1 % (log) and 13.3 % (identity), the restatement's shares exactly
"""
import functools
import os
from collections import OrderedDict

import numpy as np
import pytest

from tests import hsfit_cases as H

pytestmark = pytest.mark.gpu

STATIONARITY, COVARIANCE, LOSS = 1e-6, 1e-10, 1e-9


def _fit(x, forms, y, sigma, p0, lo=None, hi=None, ips=None, log_mode=True, fix_intercept=False, max_iter=200):
    from pisa_amd import kernels as K

    n = len(p0)
    box = H.free_box(n)
    res = K.hypersurface_fit(x, forms, K.to_device(y), K.to_device(sigma), p0, box[0] if lo is None else lo,
                             box[1] if hi is None else hi, np.zeros(n) if ips is None else ips, log_mode,
                             fix_intercept, max_iter)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def _measures(forms, x, y, sigma, out, log_mode, ips=None, free=None, which=None):
    """the worst stationarity and covariance figures over the problems `which` (default: all)"""
    worst_s = worst_c = 0.0
    for k in (range(y.shape[1]) if which is None else which):
        fr = None if free is None else free[k]
        args = (forms, x, y[:, k], sigma[:, k], out["coef"][k])
        worst_s = max(worst_s, H.stationarity(*args, out["cov"][k], log_mode, ips, fr))
        worst_c = max(worst_c, H.cov_error(out["cov"][k], H.cov_reference(*args, log_mode, ips, fr), fr))
    return worst_s, worst_c


@pytest.fixture(scope="module")
def case_a():
    x, y, sigma, truth = H.case_a()
    out = _fit(x, H.FORMS_A, y, sigma, np.zeros(6))
    return x, y, sigma, truth, out


def test_seeded_inputs_meet_both_measures(case_a):
    x, y, sigma, _, out = case_a
    assert np.all(out["status"] == 0), np.bincount(out["status"])
    worst_s, worst_c = _measures(H.FORMS_A, x, y, sigma, out, True)
    lo, hi = H.free_box(6)
    ref = H.batch_solver(x, H.FORMS_A, y, sigma, np.zeros(6), lo, hi, np.zeros(6), True, False)
    excess = np.max((out["loss"] - ref["loss"]) / ref["loss"])
    print("stationarity %.3g, covariance %.3g, loss above the restatement's %.3g, trial points <= %d"
          % (worst_s, worst_c, excess, out["n_iter"].max()))
    assert worst_s <= STATIONARITY
    assert worst_c <= COVARIANCE
    assert excess <= LOSS
    np.testing.assert_allclose(out["chi2"], np.stack([H.chi2_all(H.FORMS_A, x, y[:, k], sigma[:, k], out["coef"][k], True)
                                                      for k in range(y.shape[1])], axis=1), rtol=1e-9, atol=1e-12)
    for k in range(y.shape[1]):
        assert np.array_equal(out["cov"][k], out["cov"][k].T)
    again = _fit(x, H.FORMS_A, y, sigma, np.zeros(6))
    for key in ("coef", "cov", "chi2", "loss"):
        assert _same_bits(out[key], again[key]), key
    assert np.array_equal(out["n_iter"], again["n_iter"]) and np.array_equal(out["status"], again["status"])


def test_results_do_not_depend_on_the_place_in_the_batch(case_a):
    x, y, sigma, _, out = case_a
    n = y.shape[1]
    rev = _fit(x, H.FORMS_A, y[:, ::-1].copy(), sigma[:, ::-1].copy(), np.zeros(6))
    # a batch of 150: the 128 problems at scattered places, the rest filled with repeats
    rs = np.random.RandomState(2)
    place = np.sort(rs.choice(150, n, replace=False))
    src = rs.randint(0, n, 150)
    src[place] = np.arange(n)
    big = _fit(x, H.FORMS_A, y[:, src].copy(), sigma[:, src].copy(), np.zeros(6))
    parts = [_fit(x, H.FORMS_A, y[:, a:b].copy(), sigma[:, a:b].copy(), np.zeros(6))
             for a, b in ((0, 50), (50, 100), (100, 128))]
    for key in ("coef", "cov", "loss"):
        assert _same_bits(rev[key][::-1], out[key]), key
        assert _same_bits(big[key][place], out[key]), key
        assert _same_bits(np.concatenate([p[key] for p in parts]), out[key]), key
    assert _same_bits(rev["chi2"][:, ::-1], out["chi2"])
    assert _same_bits(big["chi2"][:, place], out["chi2"])
    assert _same_bits(np.concatenate([p["chi2"] for p in parts], axis=1), out["chi2"])
    assert np.array_equal(big["n_iter"][place], out["n_iter"]) and np.all(big["status"] == 0)


def test_limits_sixteen_coefficients_seventy_sets():
    from pisa_amd import _lib

    x, y, sigma, truth = H.case_limit()
    p0 = np.zeros(16)
    p0[0] = 1.0
    out = _fit(x, H.FORMS_LIMIT, y, sigma, p0, log_mode=False)
    assert np.all(out["status"] == 0)
    worst_s, worst_c = _measures(H.FORMS_LIMIT, x, y, sigma, out, False)
    print("C = 16, 70 sets: stationarity %.3g, covariance %.3g" % (worst_s, worst_c))
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE
    pull = (out["coef"] - truth) / np.sqrt(np.einsum("kii->ki", out["cov"]))
    assert np.max(np.abs(pull)) < 5
    # one coefficient or one set more is refused
    with pytest.raises(_lib.PisaHipError) as err:
        _fit(np.zeros((8, 70)), ("quadratic",) * 8, y, sigma, np.zeros(17), log_mode=False)
    assert err.value.status == -1
    with pytest.raises(_lib.PisaHipError) as err:
        _fit(np.zeros((8, 129)), H.FORMS_LIMIT, np.ones((129, 2)), np.ones((129, 2)), p0, log_mode=False)
    assert err.value.status == -1


def test_bounds_and_priors(case_a):
    from scipy.optimize import least_squares

    x, y, sigma, truth, free_fit = case_a
    n = y.shape[1]
    # the first quadratic coefficient is N(0, 0.5) in truth: an upper bound of 0.1 cuts a good third of the bins
    lo, hi = H.free_box(6)
    hi[1] = 0.1
    out = _fit(x, H.FORMS_A, y, sigma, np.zeros(6), lo, hi)
    assert np.all(out["status"] == 0)
    cut = out["coef"][:, 1] == 0.1
    assert 30 <= np.count_nonzero(cut) <= 80 and np.all(out["coef"][:, 1] <= 0.1)
    assert np.array_equal(cut, free_fit["coef"][:, 1] > 0.1)
    free = np.ones((n, 6), bool)
    free[cut, 1] = False
    for k in np.flatnonzero(cut):
        assert np.all(out["cov"][k][1, :] == 0.0) and np.all(out["cov"][k][:, 1] == 0.0)
        _, g, _ = H.loss_grad_hess(H.FORMS_A, x, y[:, k], sigma[:, k], out["coef"][k], True)
        assert g[1] < 0          # descent leaves the box through the bound
    worst_s, worst_c = _measures(H.FORMS_A, x, y, sigma, out, True, free=free)
    print("bounded: stationarity %.3g, covariance %.3g, %d of %d on the bound" % (worst_s, worst_c, cut.sum(), n))
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE
    worst = -np.inf
    for k in np.flatnonzero(cut):          # every bin the bound cuts
        def parts(c):
            with np.errstate(all="ignore"):
                m, E, _ = H.model(H.FORMS_A, x, c, True, np.float64)
                return (m - y[:, k]) / sigma[:, k], (m / sigma[:, k])[:, None] * E

        def resid(c):
            r = parts(c)[0]
            return np.where(np.isfinite(r), r, 1e150)

        def jac(c):
            return np.nan_to_num(parts(c)[1], nan=0.0, posinf=1e150, neginf=-1e150)
        sp = least_squares(resid, np.zeros(6), jac=jac, bounds=(lo, hi), xtol=1e-15, ftol=1e-15, gtol=1e-15,
                           max_nfev=2000)
        worst = max(worst, (out["loss"][k] - 2.0 * sp.cost) / (2.0 * sp.cost))
    print("loss above scipy.optimize.least_squares(bounds): %.3g" % worst)
    assert worst <= LOSS
    # priors: the prior term is part of the gradient, of the Hessian and of the loss
    ips = 1.0 / np.array([0.05, 0.5, 0.5, 0.1, 0.2, 0.3])
    out = _fit(x, H.FORMS_A, y, sigma, np.zeros(6), ips=ips)
    assert np.all(out["status"] == 0)
    worst_s, worst_c = _measures(H.FORMS_A, x, y, sigma, out, True, ips=ips)
    print("priors: stationarity %.3g, covariance %.3g" % (worst_s, worst_c))
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE
    for k in (0, 77):
        want = H.loss_only(H.FORMS_A, x, y[:, k], sigma[:, k], out["coef"][k], True, ips)
        np.testing.assert_allclose(out["loss"][k], want, rtol=1e-12)
    # a fixed intercept stays where it starts, with zero rows and columns (the maps rescaled so that 0 is its truth)
    scale = np.exp(-truth[:, 0])
    y0, sigma0 = y * scale, sigma * scale
    out = _fit(x, H.FORMS_A, y0, sigma0, np.zeros(6), fix_intercept=True)
    assert np.all(out["status"] == 0)
    assert np.all(out["coef"][:, 0] == 0.0) and np.all(out["cov"][:, 0, :] == 0.0) and np.all(out["cov"][:, :, 0] == 0.0)
    free = np.ones((n, 6), bool)
    free[:, 0] = False
    worst_s, worst_c = _measures(H.FORMS_A, x, y0, sigma0, out, True, free=free)
    print("fixed intercept: stationarity %.3g, covariance %.3g" % (worst_s, worst_c))
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE


def test_data_rules_on_the_device(case_a):
    from pisa_amd import _lib

    x, y, sigma, _, clean = case_a
    y, sigma = y[:, :12].copy(), sigma[:, :12].copy()
    y[4, 3] = np.nan                                  # NaN in a used set: not fitted
    y[5, 6], sigma[5, 6] = 0.0, 0.0                   # an empty set: ignored, chi2 inf
    y[9, 6], sigma[9, 6] = np.nan, 0.0                # an unused set may hold anything: chi2 NaN
    sigma[5:, 9] = 0.0                                # 5 used sets for 6 coefficients
    out = _fit(x, H.FORMS_A, y, sigma, np.zeros(6))
    assert out["status"][3] == _lib.HSFIT_NOT_FITTED
    assert out["status"][9] == _lib.HSFIT_NOT_FITTED | _lib.HSFIT_UNDERDETERMINED
    for k in (3, 9):
        assert np.all(np.isnan(out["coef"][k])) and np.all(np.isnan(out["cov"][k])) and np.isnan(out["loss"][k])
        assert np.all(np.isnan(out["chi2"][:, k])) and out["n_iter"][k] == 0
    assert out["status"][6] == 0
    assert np.isinf(out["chi2"][5, 6]) and np.isnan(out["chi2"][9, 6])
    used = np.ones(16, bool)
    used[[5, 9]] = False
    assert np.all(np.isfinite(out["chi2"][used, 6]))
    worst_s, worst_c = _measures(H.FORMS_A, x, np.nan_to_num(y), sigma, out, True, which=[6])
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE
    np.testing.assert_allclose(out["loss"][6], np.sum(out["chi2"][used, 6]), rtol=1e-12)
    others = [k for k in range(12) if k not in (3, 6, 9)]
    for key in ("coef", "cov", "loss"):
        assert _same_bits(out[key][others], clean[key][others]), key
    assert _same_bits(out["chi2"][:, others], clean["chi2"][:, others])
    # an unused set may also lie where the model has no value (1 + m x <= 0 for the logarithmic form): it adds
    # exact zeros to every chain, so the fit is the fit without it, bit for bit
    x17 = np.concatenate([x, [[0.0], [0.0], [-50.0]]], axis=1)
    y17 = np.concatenate([case_a[1][:, :12], np.full((1, 12), 3.0)])
    s17 = np.concatenate([case_a[2][:, :12], np.zeros((1, 12))])
    far = _fit(x17, H.FORMS_A, y17, s17, np.zeros(6))
    assert np.all(far["status"] == 0)
    for key in ("coef", "cov", "loss"):
        assert _same_bits(far[key], clean[key][:12]), key
    assert _same_bits(far["chi2"][:16], clean["chi2"][:, :12]) and np.all(np.isnan(far["chi2"][16]))
    # too few trial points: flagged, the coefficients are still numbers
    short = _fit(x, H.FORMS_A, y[:, :3].copy(), sigma[:, :3].copy(), np.zeros(6), max_iter=2)
    assert np.all(short["status"] & _lib.HSFIT_NOT_CONVERGED) and np.all(np.isfinite(short["coef"]))


# ------------------------------------------------------------------ the families of tests/hsfit_cases.py
@functools.lru_cache(maxsize=None)
def _dev(name):
    """the device's result on a family, one launch per session"""
    f = H.get(name)
    return _fit(f["x"], f["forms"], f["y"], f["sigma"], f["p0"], f["lo"], f["hi"], f["ips"], f["log_mode"],
                f["fix_intercept"], f["max_iter"])


def _fam_measures(fam, out, which=None):
    return _measures(fam["forms"], fam["x"], fam["y"], fam["sigma"], out, fam["log_mode"], fam["ips"],
                     H.free_mask(fam, out["coef"]), which)


@pytest.mark.parametrize("name", H.WELL_POSED)
def test_well_posed_families_meet_the_measures(name):
    fam, out, ref = H.get(name), _dev(name), H.reference(name)
    assert np.all(out["status"] == 0), np.bincount(out["status"])
    worst_s, worst_c = _fam_measures(fam, out)
    excess = np.max((out["loss"] - ref["loss"]) / ref["loss"])
    print("%s: stationarity %.3g, covariance %.3g, loss above the restatement's %.3g, trial points <= %d"
          % (name, worst_s, worst_c, excess, out["n_iter"].max()))
    assert worst_s <= STATIONARITY
    assert worst_c <= COVARIANCE
    assert excess <= LOSS
    # the same coefficients end on a bound as in the restatement
    assert np.array_equal(H.free_mask(fam, out["coef"]), H.free_mask(fam, ref["coef"]))


def _anchor(name, out, coef, cov, loss):
    sd = np.sqrt(np.einsum("kii->ki", cov))
    worst_c = np.max(np.abs(out["coef"] - coef) / sd)
    worst_v = max(H.cov_error(out["cov"][k], cov[k]) for k in range(len(loss)))
    worst_l = np.max(np.abs(out["loss"] - loss) / loss)
    print("%s against the exact solution: coefficients %.3g of their error, covariance %.3g, loss %.3g"
          % (name, worst_c, worst_v, worst_l))
    assert worst_c <= STATIONARITY
    assert worst_v <= COVARIANCE
    assert worst_l <= LOSS


@pytest.mark.parametrize("name, key", [("lin-plain", "f_lin/plain"), ("lin-prior", "f_lin/prior"),
                                       ("lin-up30", "f_lin/plain"), ("lin-down30", "f_lin/plain"),
                                       ("ill-twin_prior", "f_ill/twin_prior")])
def test_exact_anchor(name, key):
    """coefficients, covariance and loss against the 40-digit solution of the normal equations
    (oracle/gen_hsfit_exact.py), which no minimiser had a part in"""
    g = np.load(H.EXACT_FILE, allow_pickle=False)
    s = H.LIN_SCALE.get(name[4:], 1.0)      # a power of two: the exact answer scales exactly
    out = _dev(name)
    assert np.all(out["status"] == 0)
    _anchor(name, out, g[key + "/coef"] * s, g[key + "/cov"] * (s * s), g[key + "/loss"])
    if s != 1.0:
        np.testing.assert_allclose(out["loss"], _dev("lin-plain")["loss"], rtol=1e-12)


def _scipy_loss(fam, k):
    """2 x cost of scipy.optimize.least_squares(bounds=...) on problem k; a pinned coefficient is substituted"""
    from scipy.optimize import least_squares

    forms, x, y, sigma, log_mode = fam["forms"], fam["x"], fam["y"][:, k], fam["sigma"][:, k], fam["log_mode"]
    var = fam["lo"] < fam["hi"]
    start = np.clip(fam["p0"], fam["lo"], fam["hi"])

    def full(v):
        c = start.copy()
        c[var] = v
        return c

    def parts(v):
        with np.errstate(all="ignore"):
            m, E, _ = H.model(forms, x, full(v), log_mode, np.float64)
            return (m - y) / sigma, ((m if log_mode else np.ones_like(m)) / sigma)[:, None] * E[:, var]

    def resid(v):
        r = parts(v)[0]
        return np.where(np.isfinite(r), r, 1e150)

    def jac(v):
        return np.nan_to_num(parts(v)[1], nan=0.0, posinf=1e150, neginf=-1e150)
    sp = least_squares(resid, start[var], jac=jac, bounds=(fam["lo"][var], fam["hi"][var]), xtol=1e-15, ftol=1e-15,
                       gtol=1e-15, max_nfev=2000)
    return 2.0 * sp.cost


@pytest.mark.parametrize("variant", H.BOX_VARIANTS)
def test_bound_shapes(variant):
    """(the measures on the free block: test_well_posed_families_meet_the_measures)"""
    fam, out = H.get("box-" + variant), _dev("box-" + variant)
    coef, lo, hi = out["coef"], fam["lo"], fam["hi"]
    assert np.all(coef >= lo) and np.all(coef <= hi)
    on = ~H.free_mask(fam, coef)
    worst = -np.inf
    for k in range(coef.shape[0]):
        _, g, _ = H.loss_grad_hess(fam["forms"], fam["x"], fam["y"][:, k], fam["sigma"][:, k], coef[k],
                                    fam["log_mode"], fam["ips"])
        for i in np.flatnonzero(on[k]):
            assert np.all(out["cov"][k][i, :] == 0.0) and np.all(out["cov"][k][:, i] == 0.0)
            if lo[i] < hi[i]:          # descent leaves the box through the bound
                assert (g[i] > 0) if coef[k, i] == lo[i] else (g[i] < 0)
        if on[k].any():                # every problem a bound cuts
            sp = _scipy_loss(fam, k)
            worst = max(worst, (out["loss"][k] - sp) / sp)
    print("box-%s: on the lower bound %s, on the upper %s of %d; loss above scipy.optimize.least_squares(bounds) %.3g"
          % (variant, (coef == lo).sum(0), (coef == hi).sum(0), coef.shape[0], worst))
    assert worst <= LOSS
    n = coef.shape[0]
    if variant == "lower":
        assert 4 <= on[:, 1].sum() <= n - 4
    elif variant == "two_sided":
        assert np.sum(coef[:, 2] == -0.3) >= 4 and np.sum(coef[:, 2] == 0.3) >= 4 and np.sum(~on[:, 2]) >= 4
    elif variant == "pinned":
        assert np.all(coef[:, 3] == 0.05)
    elif variant == "outside":
        assert on[:, 1].sum() >= 4 and on[:, 5].sum() >= 1
    elif variant == "intercept":
        assert 4 <= on[:, 0].sum() <= n - 4
    else:                              # the start sits on two bounds the minimum is inside of
        assert worst == -np.inf and not on.any()
        assert np.all(coef[:, 4] > lo[4]) and np.all(coef[:, 1] < hi[1])


def _launch(fam, sel):
    return _fit(fam["x"], fam["forms"], fam["y"][:, sel].copy(), fam["sigma"][:, sel].copy(), fam["p0"], fam["lo"],
                fam["hi"], fam["ips"], fam["log_mode"], fam["fix_intercept"], fam["max_iter"])


def _same_result(a, b):
    for key in ("coef", "cov", "loss"):
        assert _same_bits(a[key], b[key]), key
    assert _same_bits(a["chi2"], b["chi2"])
    assert np.array_equal(a["n_iter"], b["n_iter"]) and np.array_equal(a["status"], b["status"])


def _pick(out, sel):
    return {k: (v[:, sel] if k == "chi2" else v[sel]) for k, v in out.items()}


def test_more_problems_than_workgroups():
    """4096 + 70 problems: the workgroups of the first 70 take a second problem, in LDS the first one left behind,
    also where the first one was not fitted or ended as NOT_POSDEF (and the other way round)"""
    from pisa_amd import _lib

    fam, source = H.f_many()
    n = source.size
    assert n == H.MANY_FIRST + H.MANY_EXTRA
    one = _launch(fam, np.arange(n))
    first, rest = _launch(fam, np.arange(H.MANY_FIRST)), _launch(fam, np.arange(H.MANY_FIRST, n))
    _same_result(one, {k: np.concatenate([first[k], rest[k]], axis=1 if k == "chi2" else 0) for k in one})
    _same_result(one, _pick(_launch(fam, np.arange(n)[::-1]), np.arange(n)[::-1]))
    want = {"nan": _lib.HSFIT_NOT_FITTED, "few": _lib.HSFIT_NOT_FITTED | _lib.HSFIT_UNDERDETERMINED,
            "flat": _lib.HSFIT_NOT_POSDEF}
    partners = []
    for i, kind in H.MANY_BAD:
        assert one["status"][i] == want[kind], (i, kind, one["status"][i])
        assert np.all(np.isnan(one["cov"][i]))
        if kind == "flat":
            assert np.all(np.isfinite(one["coef"][i])) and np.isfinite(one["loss"][i]) and one["coef"][i, 2] == 0.0
        else:
            assert np.all(np.isnan(one["coef"][i])) and np.isnan(one["loss"][i]) and one["n_iter"][i] == 0
            assert np.all(np.isnan(one["chi2"][:, i]))
        partners.append(i + H.MANY_FIRST if i < H.MANY_FIRST else i - H.MANY_FIRST)
    good = np.flatnonzero(source >= 0)
    assert np.all(one["status"][good] == 0) and np.all(source[partners] >= 0)
    # every good problem is one of the pool's 64: all copies equal the pool's own launch bit for bit, the partners
    # of the bad problems among them, and the pool meets the measures
    pool = _dev("many-pool")
    _same_result(_pick(one, good), _pick(pool, source[good]))
    worst_s, worst_c = _fam_measures(fam, one, partners)
    print("the %d problems sharing a workgroup with a bad one: stationarity %.3g, covariance %.3g"
          % (len(partners), worst_s, worst_c))
    assert worst_s <= STATIONARITY and worst_c <= COVARIANCE


def test_flags():
    from pisa_amd import _lib

    NC, NP = _lib.HSFIT_NOT_CONVERGED, _lib.HSFIT_NOT_POSDEF
    g = np.load(H.EXACT_FILE, allow_pickle=False)
    # two identical derivative rows: singular Hessian, unique minimum loss
    out = _dev("ill-twin")
    print("ill-twin: status %s" % np.bincount(out["status"]))
    assert np.all(out["status"] & NP) and np.all(np.isnan(out["cov"])) and np.all(np.isfinite(out["coef"]))
    exact = g["f_ill/twin/loss"]
    assert np.max(np.abs(out["loss"] - exact) / exact) <= LOSS
    # a start point without a value: every trial point is refused until lambda has run out
    fam, out = H.get("ill-nan_start"), _dev("ill-nan_start")
    bad = np.zeros(fam["y"].shape[1], bool)
    bad[list(H.ILL_NAN)] = True
    print("ill-nan_start: trial points %s" % out["n_iter"][bad])
    assert np.all(out["status"][bad] & NC) and np.all(out["n_iter"][bad] <= H.LAMBDA_DECADES + 1)
    assert np.all(out["coef"][bad] == np.clip(fam["p0"], fam["lo"], fam["hi"]))
    _same_result(_pick(out, ~bad), _launch(fam, ~bad))
    assert np.all(out["status"][~bad] == 0)
    # the minimum at infinity
    fam, out = H.get("ill-valley"), _dev("ill-valley")
    start = [H.loss_only(fam["forms"], fam["x"], fam["y"][:, k], fam["sigma"][:, k], fam["p0"], True)
             for k in range(fam["y"].shape[1])]
    assert np.all(out["status"] & NC) and np.all(np.isfinite(out["coef"])) and np.all(out["loss"] <= start)
    assert np.all(out["coef"][:, 0] == 0.0)
    # no trial point at all: the start point, flagged, with the covariance of the Hessian there
    for f, lm in H.MAX_ITER_0:
        name = "no-iter-%s-%s" % (f, "log" if lm else "identity")
        fam, out = H.get(name), _dev(name)
        assert np.all(out["status"] == NC) and np.all(out["n_iter"] == 0) and np.all(out["coef"] == fam["p0"])
        worst_c = _fam_measures(fam, out)[1]
        print("%s: covariance at the start point %.3g" % (name, worst_c))
        assert worst_c <= COVARIANCE


def test_status_zero_means_converged():
    """Over every problem of every family, the flag families and a scan of exponential_scaled + linear with
    unconstrained truths in both links (the 4096 + 70 problems are copies of the `many-pool` family, bit for bit:
    test_more_problems_than_workgroups): status 0 implies the stationarity gate; a flagged problem keeps finite
    coefficients.  The scan's flagged share may exceed the restatement's (H.SCAN_FLAGGED, measured by
    tests/test_host_hsfit.py: 31 / 256 in log mode, 34 / 256 with the identity link) by two percentage points:
    device and host part on borderline problems by rounding."""
    from pisa_amd import _lib

    flagged_bits = _lib.HSFIT_NOT_CONVERGED | _lib.HSFIT_NOT_POSDEF
    for name in H.FAMILIES:
        fam, out = H.get(name), _dev(name)
        ok = np.flatnonzero(out["status"] == 0)
        flagged = np.flatnonzero(out["status"] & flagged_bits)
        assert ok.size + flagged.size == out["status"].size
        assert np.all(np.isfinite(out["coef"][flagged]))
        worst_s = _fam_measures(fam, out, ok)[0] if ok.size else 0.0
        share = flagged.size / out["status"].size
        if name in H.SCAN_FLAGGED or worst_s > STATIONARITY / 10:
            print("%s: %.1f %% flagged (the restatement %.1f %%), stationarity of the others %.3g"
                  % (name, 100 * share, 100 * H.SCAN_FLAGGED.get(name, np.nan), worst_s))
        assert worst_s <= STATIONARITY, name
        if name in H.SCAN_FLAGGED:
            assert share <= H.SCAN_FLAGGED[name] + 0.02


# ------------------------------------------------------------------ end to end
K_PLANTED = 0.8
DELTAS = (0.0, -0.2, -0.1, 0.1, 0.2)


def _write_events(path, delta, n, seed):
    """a few thousand events; the weights of the upper half of the energy range carry exp(K_PLANTED * delta)"""
    import pandas as pd

    rs = np.random.RandomState(seed)
    energy = 10.0 ** rs.uniform(0.0, 2.0, n)
    weight = rs.uniform(0.5, 1.5, n) * np.where(energy > 10.0, np.exp(K_PLANTED * delta), 1.0)
    # the lowest energy bin of the last set is starved: below minimum_mc there
    if delta == DELTAS[-1]:
        keep = (energy > 10.0 ** 0.5) | (rs.uniform(size=n) < 0.01)
        energy, weight = energy[keep], weight[keep]
    n = energy.size
    pd.DataFrame(dict(pdg=np.full(n, 14), type=np.ones(n, int), true_energy=energy,
                      true_coszen=rs.uniform(-1, 1, n), reco_energy=energy, reco_coszen=rs.uniform(-1, 1, n),
                      pid=np.zeros(n), weight=weight)).to_csv(path, index=False)


def _cfg(events_file, binning):
    cfg = OrderedDict()
    cfg["pipeline"] = OrderedDict(name="hsfit", output_binning=binning, output_key=("weights", "errors"),
                                  detector_name=None)
    data_dict = dict(true_energy="true_energy", true_coszen="true_coszen", reco_energy="reco_energy",
                     reco_coszen="reco_coszen", pid="pid", initial_weights="weight")
    cfg[("data", "csv_loader")] = OrderedDict(events_file=events_file, data_dict=data_dict, output_names=["numu_cc"],
                                              calc_mode="events", apply_mode="events")
    cfg[("utils", "hist")] = OrderedDict(calc_mode="events", apply_mode=binning, error_method="sumw2")
    return cfg


def test_fit_hypersurfaces_end_to_end(tmp_path):
    from pisa_amd.core.binning import MultiDimBinning, OneDimBinning
    from pisa_amd.core.pipeline import Pipeline
    from pisa_amd.utils import hypersurface as hs

    binning = MultiDimBinning([OneDimBinning(name="reco_energy", is_log=True, num_bins=4, domain=[1.0, 100.0],
                                             units="GeV")])
    datasets = []
    for i, delta in enumerate(DELTAS):
        path = os.path.join(str(tmp_path), "events_%d.csv" % i)
        _write_events(path, delta, 4000, 100 + i)
        datasets.append(dict(pipeline_cfg=_cfg(path, binning), sys_params=dict(dom_eff=1.0 + delta)))
    minimum_mc = 100
    out = hs.fit_hypersurfaces(datasets[0], datasets[1:], [hs.HypersurfaceParam("dom_eff", "linear")],
                               str(tmp_path), "e2e", log=True, minimum_mc=minimum_mc)
    assert os.path.basename(out) == "e2e__hypersurface_fits__1d__dom_eff.json"
    surfaces = hs.load_hypersurfaces(out, expected_binning=binning)
    assert list(surfaces) == ["numu_cc"]
    hsf = surfaces["numu_cc"]
    assert hsf.log and hsf.fit_method == hs.FIT_METHOD and hsf.params["dom_eff"].nominal_value == 1.0
    slope = hsf.params["dom_eff"].fit_coeffts[:, 0]
    sig = np.sqrt(hsf.fit_cov_mat[:, 1, 1])
    want = np.array([0.0, 0.0, K_PLANTED, K_PLANTED])
    print("slopes", slope, "+-", sig)
    assert np.all(np.isfinite(slope)) and np.all(np.abs(slope - want) <= 5 * sig) and np.all(sig < 0.2)
    # the starved bin drops the last set only: chi2 = (m - 0) / 0 there, finite for the other sets and bins
    assert np.isinf(hsf.fit_chi2[0, -1]) and np.all(np.isfinite(hsf.fit_chi2[0, :-1]))
    assert np.all(np.isfinite(hsf.fit_chi2[1:]))
    # the stage with the written file turns the nominal map into a systematic set's, within errors
    cfg = _cfg(datasets[0]["pipeline_cfg"][("data", "csv_loader")]["events_file"], binning)
    from pisa_amd.core.param import Param, ParamSet

    cfg[("discr_sys", "hypersurfaces")] = OrderedDict(
        params=ParamSet([Param(name="dom_eff", value=1.0 + DELTAS[3], prior=None, range=None, is_fixed=True)]),
        fit_results_file=out, calc_mode=binning, apply_mode=binning, error_method="sumw2")
    got = Pipeline(cfg).get_outputs()["numu_cc"]
    target = Pipeline(datasets[3]["pipeline_cfg"]).get_outputs()["numu_cc"]
    err = np.hypot(got.std_devs, target.std_devs)
    assert np.all(np.abs(got.nominal_values - target.nominal_values) <= 5 * err)
