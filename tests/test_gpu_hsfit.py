"""`pisa_hip_hypersurface_fit` on the device against the numpy restatement's two measures (tests/hsfit_cases.py):
  stationarity  |H^-1 (-g)|_i <= 1e-6 sqrt(cov_ii) for every free coefficient of every fitted problem
  covariance    |cov - cov_ref|_ij / sqrt(cov_ii cov_jj) <= 1e-10, cov_ref the inverse of the longdouble
                half-Hessian at the returned coefficients
plus: results do not depend on where a problem sits in the batch (bit for bit), the compile-time limits, bounds
and priors, the data rules (NaN, sigma = 0, too few sets), and `fit_hypersurfaces` end to end on planted events.
"""
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
