"""Hypersurface fitting without a GPU: the numpy restatement of the fit (tests/hsfit_cases.py) against its own
two measures, the argument checks of `pisa_hip_hypersurface_fit` (before any device access), and everything
`Hypersurface.fit` does around the batch solver, with the restatement handed in as the solver.  Every seeded family
that tests/test_gpu_hsfit.py holds the device to the gates on is held to a TENTH of the gates here with the
restatement (that is what "well posed" means), the golden file of exact solutions is regenerated and compared, and
the restatement's share of flagged problems in the scan is measured.

The two measures (tests/hsfit_cases.py):
  stationarity  |H^-1 (-g)|_i <= 1e-6 sqrt(cov_ii) for every free coefficient of every fitted problem
  covariance    |cov - cov_ref|_ij / sqrt(cov_ii cov_jj) <= 1e-10, cov_ref the inverse of the longdouble
                half-Hessian at the returned coefficients
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import hsfit_cases as H

from pisa_amd.utils import hypersurface as hs

STATIONARITY, COVARIANCE, LOSS = 1e-6, 1e-10, 1e-9


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", list(hs.HYPERSURFACE_PARAM_FUNCTIONS))
def test_second_derivatives_agree_with_central_differences_of_the_gradients(name):
    k, _, grad = hs.HYPERSURFACE_PARAM_FUNCTIONS[name]
    x = np.array([-0.7, -0.2, 0.3, 1.1])
    c = [0.3, 0.4][:k]
    d2 = H.second_derivatives(name, x, *c)
    h = 1e-5
    for b in range(k):
        up, dn = list(c), list(c)
        up[b] += h
        dn[b] -= h
        numeric = (grad(x, *up) - grad(x, *dn)) / (2 * h)      # [..., a]: d/dc_b of df/dc_a
        for a in range(k):
            np.testing.assert_allclose(np.broadcast_to(d2[a][b], x.shape), numeric[..., a], rtol=1e-8, atol=1e-9)


@pytest.fixture(scope="module")
def case_a():
    x, y, sigma, truth = H.case_a()
    lo, hi = H.free_box(6)
    out = H.batch_solver(x, H.FORMS_A, y, sigma, np.zeros(6), lo, hi, np.zeros(6), True, False)
    return x, y, sigma, truth, out


def test_restatement_meets_both_measures_on_the_seeded_inputs(case_a):
    x, y, sigma, _, out = case_a
    assert np.all(out["status"] == 0), np.bincount(out["status"])
    worst_s = worst_c = worst_gn = 0.0
    for k in range(y.shape[1]):
        args = (H.FORMS_A, x, y[:, k], sigma[:, k], out["coef"][k])
        worst_s = max(worst_s, H.stationarity(*args, out["cov"][k], True))
        ref = H.cov_reference(*args, True)
        worst_c = max(worst_c, H.cov_error(out["cov"][k], ref))
        gn = np.linalg.inv(H.gauss_newton(*args, True, np.zeros(6)))
        worst_gn = max(worst_gn, H.cov_error(gn, ref))
    print("stationarity %.3g, covariance %.3g, Gauss-Newton covariance %.3g, trial steps <= %d"
          % (worst_s, worst_c, worst_gn, out["n_iter"].max()))
    assert worst_s <= STATIONARITY
    assert worst_c <= COVARIANCE
    assert worst_gn > 1e-4          # the covariance bound tells the exact Hessian from J^T J


# ------------------------------------------------------------------ the families of tests/test_gpu_hsfit.py
@pytest.mark.parametrize("name", H.WELL_POSED)
def test_restatement_is_inside_a_tenth_of_the_gates_on_every_well_posed_family(name):
    """well posed: the restatement ends with status 0 within half of max_iter and meets a tenth of both gates, on
    every problem.  A family that does not is given another seed or truth distribution, never another gate."""
    fam, out = H.get(name), H.reference(name)
    assert np.all(out["status"] == 0), np.bincount(out["status"])
    assert out["n_iter"].max() <= fam["max_iter"] // 2
    worst_s, worst_c = H.measures(fam, out)
    print("%s: stationarity %.3g, covariance %.3g, trial points <= %d" % (name, worst_s, worst_c, out["n_iter"].max()))
    assert worst_s <= STATIONARITY / 10
    assert worst_c <= COVARIANCE / 10
    assert np.all(out["coef"] >= fam["lo"]) and np.all(out["coef"] <= fam["hi"])


def test_box_families_cut_release_and_pin():
    """what the box families are for happens in them: bounds cut some problems and not others, the start-on-bound
    coefficients end strictly inside"""
    on = {v: ~H.free_mask(H.get("box-" + v), H.reference("box-" + v)["coef"]) for v in H.BOX_VARIANTS}
    n = on["lower"].shape[0]
    assert 4 <= on["lower"][:, 1].sum() <= n - 4
    coef = H.reference("box-two_sided")["coef"][:, 2]
    assert np.sum(coef == -0.3) >= 4 and np.sum(coef == 0.3) >= 4 and np.sum(np.abs(coef) < 0.3) >= 4
    assert np.all(on["pinned"][:, 3]) and np.all(H.reference("box-pinned")["coef"][:, 3] == 0.05)
    assert on["outside"][:, 1].sum() >= 4 and on["outside"][:, 5].sum() >= 1
    assert 4 <= on["intercept"][:, 0].sum() <= n - 4
    assert not on["leave"].any()


def test_restatement_loss_against_the_exact_minimum():
    g = np.load(H.EXACT_FILE, allow_pickle=False)
    for name, key in (("lin-plain", "f_lin/plain"), ("lin-prior", "f_lin/prior"), ("lin-up30", "f_lin/plain"),
                      ("lin-down30", "f_lin/plain"), ("ill-twin_prior", "f_ill/twin_prior"), ("ill-twin", "f_ill/twin")):
        exact = g[key + "/loss"]
        worst = np.max(np.abs(H.reference(name)["loss"] - exact) / exact)
        print("%s: loss off the exact minimum by %.3g" % (name, worst))
        assert worst <= LOSS


def test_golden_file_is_reproduced_from_the_seeds():
    pytest.importorskip("mpmath")
    from oracle import gen_hsfit_exact

    g = np.load(H.EXACT_FILE, allow_pickle=False)
    out = gen_hsfit_exact.build()
    assert sorted(g.files) == sorted(out)
    for k in out:
        assert g[k].dtype == out[k].dtype and g[k].shape == out[k].shape and g[k].tobytes() == out[k].tobytes(), k


def test_flag_families_and_status_zero_in_the_restatement():
    """the flag families end as flagged, and over them and the scan a status of 0 implies the stationarity gate.
    The flagged shares of the scan are the figures tests/test_gpu_hsfit.py holds the device to."""
    from pisa_amd import _lib

    NC, NP = _lib.HSFIT_NOT_CONVERGED, _lib.HSFIT_NOT_POSDEF
    out = H.reference("ill-twin")
    assert np.all(out["status"] == NP) and np.all(np.isnan(out["cov"])) and np.all(np.isfinite(out["coef"]))
    fam, out = H.get("ill-nan_start"), H.reference("ill-nan_start")
    bad = np.zeros(fam["y"].shape[1], bool)
    bad[list(H.ILL_NAN)] = True
    assert np.all(out["status"][bad] & NC) and np.all(out["status"][~bad] == 0)
    assert np.all(out["n_iter"][bad] <= H.LAMBDA_DECADES + 1) and np.all(out["coef"][bad] == fam["p0"])
    out = H.reference("ill-valley")
    assert np.all(out["status"] & NC) and np.all(np.isfinite(out["coef"]))
    fam, source = H.f_many()
    want = {"nan": _lib.HSFIT_NOT_FITTED, "few": _lib.HSFIT_NOT_FITTED | _lib.HSFIT_UNDERDETERMINED, "flat": NP}
    for i, kind in H.MANY_BAD:
        res = H.lm_fit(fam["forms"], fam["x"], fam["y"][:, i], fam["sigma"][:, i], fam["p0"], fam["lo"], fam["hi"],
                       fam["ips"], True)
        assert res[4] == want[kind] and source[i] == -1
        assert source[i + H.MANY_FIRST if i < H.MANY_FIRST else i - H.MANY_FIRST] >= 0
    for f, lm in H.MAX_ITER_0:
        name = "no-iter-%s-%s" % (f, "log" if lm else "identity")
        fam, out = H.get(name), H.reference(name)
        assert np.all(out["status"] == NC) and np.all(out["n_iter"] == 0) and np.all(out["coef"] == fam["p0"])
        assert H.measures(fam, out)[1] <= COVARIANCE / 10
    for name in ("ill-nan_start", "ill-valley", "scan-log", "scan-identity"):
        fam, out = H.get(name), H.reference(name)
        ok = np.flatnonzero(out["status"] == 0)
        worst_s, _ = H.measures(fam, out, ok)
        flagged = 1.0 - ok.size / out["status"].size
        print("%s: %.1f %% flagged, stationarity of the others %.3g" % (name, 100 * flagged, worst_s))
        assert worst_s <= STATIONARITY
        assert np.all(np.isfinite(out["coef"]))
        if name in H.SCAN_FLAGGED:
            assert flagged == H.SCAN_FLAGGED[name]


# ------------------------------------------------------------------ the C entry point, no device
def test_invalid_arguments_are_refused_before_any_device_access():
    import __graft_entry__ as g

    g.build()
    from pisa_amd import _lib

    lib = _lib.lib()
    dbl = lambda v: (C.c_double * len(v))(*v)  # noqa: E731
    good = dict(x=[0.0, 0.5, -0.5, 0.0, 0.1, 0.2], form=[1, 4], n_par=2, n_sets=3, n_prob=4, p0=[0.0] * 4,
                lo=[-np.inf] * 4, hi=[np.inf] * 4, ips=[0.0] * 4, n_coef=4, max_iter=10, null=None)
    fake = C.c_void_p(64)      # never dereferenced: every call below is refused first

    def call(**change):
        a = dict(good, **change)
        ptr = lambda name: None if a["null"] == name else fake  # noqa: E731
        return lib.pisa_hip_hypersurface_fit(
            None if a["null"] == "x" else dbl(a["x"]), (C.c_int32 * len(a["form"]))(*a["form"]), a["n_par"],
            a["n_sets"], a["n_prob"], ptr("y"), ptr("sigma"), dbl(a["p0"]), dbl(a["lo"]), dbl(a["hi"]),
            dbl(a["ips"]), a["n_coef"], 1, 0, a["max_iter"], ptr("work"), ptr("coef"), ptr("cov"), ptr("chi2"),
            ptr("loss"), ptr("n_iter"), ptr("status"), None)

    bad = [dict(null=n) for n in ("x", "y", "sigma", "work", "coef", "cov", "chi2", "loss", "n_iter", "status")]
    bad += [dict(form=[1, 5]), dict(form=[-1, 4]), dict(n_coef=5), dict(n_par=0), dict(n_sets=0),
            dict(n_sets=_lib.HSFIT_MAX_SETS + 1), dict(n_prob=0), dict(n_prob=2 ** 31), dict(max_iter=-1),
            dict(lo=[0.0, 1.0, 0.0, 0.0], hi=[0.0, 0.5, 0.0, 0.0]), dict(lo=[np.nan, 0, 0, 0]),
            dict(x=[0.0, np.inf, -0.5, 0.0, 0.1, 0.2]), dict(x=[0.0, np.nan, -0.5, 0.0, 0.1, 0.2]),
            dict(p0=[np.nan, 0, 0, 0]), dict(ips=[-1.0, 0, 0, 0]), dict(ips=[np.inf, 0, 0, 0])]
    # 17 coefficients: eight quadratic parameters; 129 sets
    bad.append(dict(form=[1] * 8, n_par=8, n_coef=17, x=[0.0] * 24, p0=[0.0] * 17, lo=[-np.inf] * 17,
                    hi=[np.inf] * 17, ips=[0.0] * 17))
    bad.append(dict(n_sets=129, x=[0.0] * 258))
    for change in bad:
        assert call(**change) == -1, change
    assert _lib.HSFIT_MAX_COEFFTS == 16 and _lib.HSFIT_MAX_SETS == 128
    assert _lib.HSFIT_FORMS == tuple(hs.HYPERSURFACE_PARAM_FUNCTIONS)


# ------------------------------------------------------------------ Hypersurface.fit around the solver
def _binning(shape=(4, 3)):
    from pisa_amd.core.binning import MultiDimBinning, OneDimBinning

    return MultiDimBinning([OneDimBinning(name="reco_energy", is_log=True, num_bins=shape[0], domain=[1.0, 80.0],
                                          units="GeV"),
                            OneDimBinning(name="reco_coszen", is_lin=True, num_bins=shape[1], domain=[-1.0, 1.0])])


def _maps(log, seed=3, empty_nominal=None, zero_sigma=None):
    """nominal + 6 systematic maps of a 4 x 3 binning from a known linear (+ exponential in log mode) law"""
    from pisa_amd.core.map import Map

    rs = np.random.RandomState(seed)
    binning = _binning()
    values = [dict(dom_eff=1.0, hole_ice=25.0)] + [dict(dom_eff=v, hole_ice=25.0) for v in (0.8, 0.9, 1.1, 1.2)] \
        + [dict(dom_eff=1.0, hole_ice=v) for v in (15.0, 20.0, 30.0, 35.0)]
    nominal = rs.uniform(50.0, 200.0, binning.shape)
    k_eff = rs.normal(0.0, 0.5, binning.shape)
    k_ice = rs.normal(0.0, 0.01, binning.shape)
    maps = []
    for i, v in enumerate(values):
        eta = k_eff * (v["dom_eff"] - 1.0) + k_ice * (v["hole_ice"] - 25.0)
        expect = nominal * (np.exp(eta) if log else 1.0 + eta)
        err = 0.02 * expect
        hist = expect + err * rs.normal(size=binning.shape)
        if empty_nominal is not None and i == 0:
            hist[empty_nominal], err[empty_nominal] = 0.0, 0.0
        if zero_sigma is not None and i == zero_sigma[0]:
            hist[zero_sigma[1]], err[zero_sigma[1]] = 0.0, 0.0
        maps.append(Map("set%d" % i, hist, binning, error_hist=err))
    return binning, maps, values, (k_eff, k_ice)


def _params(**kw):
    return [hs.HypersurfaceParam("dom_eff", "linear", **kw), hs.HypersurfaceParam("hole_ice", "linear")]


def test_fit_normalises_skips_zero_sigma_sets_and_leaves_the_reference_attributes():
    binning, maps, values, (k_eff, k_ice) = _maps(log=False, empty_nominal=(0, 0), zero_sigma=(3, (2, 1)))
    hsf = hs.Hypersurface(params=_params(), initial_intercept=None, log=False)
    assert not hsf.fit_complete and hsf.intercept is None
    hsf.fit(maps[0], values[0], maps[1:], values[1:], solver=H.batch_solver, method="L-BFGS-B", ref_bin_idx=(0, 0))
    assert hsf.fit_complete and hsf.fit_info_stored and hsf.fit_method == hs.FIT_METHOD
    assert hsf.initial_intercept == 1.0 and hsf.nominal_values == dict(dom_eff=1.0, hole_ice=25.0)
    # normalisation: value and error over the nominal value, NaN where that is zero
    nominal = maps[0].nominal_values
    ok = nominal != 0
    for raw, norm in zip(hsf.fit_maps_raw, hsf.fit_maps_norm):
        np.testing.assert_array_equal(norm.nominal_values[ok], raw.nominal_values[ok] / nominal[ok])
        np.testing.assert_array_equal(norm.std_devs[ok], raw.std_devs[ok] / nominal[ok])
        assert np.all(np.isnan(norm.nominal_values[~ok])) and np.all(np.isnan(norm.std_devs[~ok]))
    # the empty nominal bin: NaN coefficients, NaN covariance
    assert hsf.fit_cov_mat.shape == (4, 3, 3, 3) and hsf.fit_chi2.shape == (4, 3, 9)
    assert np.isnan(hsf.intercept[0, 0]) and np.all(np.isnan(hsf.fit_cov_mat[0, 0]))
    assert np.all(np.isnan(hsf.params["dom_eff"].fit_coeffts[0, 0])) and hsf.fit_status[0, 0] != 0
    assert np.count_nonzero(hsf.fit_status) == 1
    # the set with sigma = 0 in bin (2, 1) is skipped there: the fit is the fit of the other eight sets ...
    x = np.array([[v["dom_eff"] - 1.0 for v in values], [v["hole_ice"] - 25.0 for v in values]])
    y = np.array([m.nominal_values[2, 1] for m in hsf.fit_maps_norm])
    sg = np.array([m.std_devs[2, 1] for m in hsf.fit_maps_norm])
    assert sg[3] == 0.0
    keep = np.arange(9) != 3
    A = np.vstack([np.ones(8), x[:, keep]]).T / sg[keep, None]
    want = np.linalg.lstsq(A, y[keep] / sg[keep], rcond=None)[0]
    got = hsf.fit_coeffts[2, 1]
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(hsf.fit_cov_mat[2, 1], np.linalg.inv(A.T @ A), rtol=1e-9)
    # ... and its chi2 is there all the same, by plain division: (m - 0) / 0 = inf
    assert np.isinf(hsf.fit_chi2[2, 1, 3]) and np.all(np.isfinite(hsf.fit_chi2[2, 1, keep]))
    assert np.all(np.isnan(hsf.fit_chi2[0, 0]))
    # sigmas are the roots of the covariance's diagonal; the planted slopes come back
    np.testing.assert_allclose(hsf.intercept_sigma[ok], np.sqrt(hsf.fit_cov_mat[..., 0, 0][ok]))
    pull = (hsf.params["dom_eff"].fit_coeffts[..., 0] - k_eff) / hsf.params["dom_eff"].fit_coeffts_sigma[..., 0]
    assert np.all(np.abs(pull[ok]) < 5)
    np.testing.assert_array_equal(hsf.params["hole_ice"].fit_param_values, [v["hole_ice"] for v in values])
    assert hsf.params["dom_eff"].fitted and hsf.num_fit_sets == 9
    hsf.drop_fit_maps()
    assert hsf.fit_maps_raw is None and hsf.fit_maps_norm is None and not hsf.fit_info_stored


def test_include_empty_gives_sigma_one_and_is_refused_in_log_mode():
    binning, maps, values, _ = _maps(log=False, zero_sigma=(3, (2, 1)))
    hsf = hs.Hypersurface(params=_params(), log=False)
    hsf.fit(maps[0], values[0], maps[1:], values[1:], include_empty=True, keep_maps=False, solver=H.batch_solver)
    assert hsf.fit_maps_raw is None and not hsf.fit_info_stored
    assert np.all(np.isfinite(hsf.fit_chi2)) and np.all(hsf.fit_status == 0)
    # the empty set takes part with value 0 and sigma 1
    predicted = hsf.evaluate(values[3])[2, 1]
    np.testing.assert_allclose(hsf.fit_chi2[2, 1, 3], predicted ** 2, rtol=1e-12)
    with pytest.raises(AssertionError, match="empty bins cannot be included in log mode"):
        hs.Hypersurface(params=_params(), log=True).fit(maps[0], values[0], maps[1:], values[1:],
                                                        include_empty=True, solver=H.batch_solver)
    with pytest.raises(Exception, match="smoothing"):
        hs.Hypersurface(params=_params(), log=True).fit(maps[0], values[0], maps[1:], values[1:],
                                                        smooth_method="gaussian_filter", solver=H.batch_solver)
    maps[2]._hist = -maps[2].nominal_values
    with pytest.raises(AssertionError, match="negative bin counts"):
        hs.Hypersurface(params=_params(), log=True).fit(maps[0], values[0], maps[1:], values[1:],
                                                        solver=H.batch_solver)


def test_fix_intercept_bounds_priors_and_mask():
    binning, maps, values, (k_eff, _) = _maps(log=True)
    hsf = hs.Hypersurface(params=_params(), log=True)
    hsf.fit(maps[0], values[0], maps[1:], values[1:], fix_intercept=True, solver=H.batch_solver)
    assert np.all(hsf.intercept == 0.0) and np.all(np.isnan(hsf.intercept_sigma))
    assert np.all(hsf.fit_cov_mat[..., 0, :] == 0.0) and np.all(hsf.fit_cov_mat[..., :, 0] == 0.0)
    assert np.all(hsf.fit_cov_mat[..., 1, 1] > 0.0)
    # a bound that cuts the planted slopes: the coefficient sits on it, with a zero row and column
    cut = float(np.median(k_eff))
    hsf = hs.Hypersurface(params=_params(bounds=(None, cut), initial_fit_coeffts=[cut - 1.0]), log=True)
    hsf.fit(maps[0], values[0], maps[1:], values[1:], solver=H.batch_solver)
    slope = hsf.params["dom_eff"].fit_coeffts[..., 0]
    assert np.all(slope <= cut) and 3 <= np.count_nonzero(slope == cut) <= 9
    assert np.all(hsf.fit_cov_mat[slope == cut][:, 1, :] == 0.0)
    assert np.all(hsf.fit_cov_mat[slope < cut][:, 1, 1] > 0.0)
    # a tight prior pulls the coefficient to zero; the reference's checks on the keywords
    hsf = hs.Hypersurface(params=_params(coeff_prior_sigma=[1e-4]), log=True)
    hsf.fit(maps[0], values[0], maps[1:], values[1:], intercept_sigma=0.5, solver=H.batch_solver)
    assert np.all(np.abs(hsf.params["dom_eff"].fit_coeffts) < 1e-3)
    with pytest.raises(AssertionError):
        hs.HypersurfaceParam("a", "quadratic", coeff_prior_sigma=[1.0])
    with pytest.raises(AssertionError):
        hs.HypersurfaceParam("a", "quadratic", initial_fit_coeffts=[1.0])
    assert hs.HypersurfaceParam("a", "quadratic", bounds=((0, 1), (None, 2)))._fit_bounds() == [(0.0, 1.0), (-np.inf, 2.0)]
    # a masked bin is not fitted
    from pisa_amd.core.binning import MultiDimBinning
    from pisa_amd.core.map import Map

    mask = np.ones(binning.shape, bool)
    mask[1, 2] = False
    masked = MultiDimBinning(binning, mask=mask)
    mm = [Map(m.name, m.nominal_values, masked, error_hist=m.std_devs) for m in maps]
    hsf = hs.Hypersurface(params=_params(), log=True)
    hsf.fit(mm[0], values[0], mm[1:], values[1:], solver=H.batch_solver)
    assert np.isnan(hsf.intercept[1, 2]) and np.count_nonzero(np.isnan(hsf.intercept)) == 1


def test_constructors_old_and_new():
    coeffts = np.arange(6.0).reshape(3, 2)
    old = hs.Hypersurface(None, [hs.HypersurfaceParam("a", "quadratic", coeffts, 0.5)], np.ones(3), True)
    assert old.log and old.fit_complete and old.params["a"].nominal_value == 0.5 and old.params["a"].fitted
    state = old.serializable_state
    assert state["initial_intercept"] is None and state["intercept_sigma"] is None and state["fit_chi2"] is None
    assert state["fit_method"] is None and state["fit_info_stored"] is False
    ps = state["params"]["a"]
    assert ps["bounds"] is None and ps["coeff_prior_sigma"] is None and ps["initial_fit_coeffts"] is None
    assert ps["fit_param_values"] is None and ps["fit_coeffts_sigma"] is None and ps["fitted"] is True
    np.testing.assert_array_equal(old.evaluate({"a": 1.0}), np.exp(1.0 + coeffts[:, 0] * 0.5 + coeffts[:, 1] * 0.25))
    new = hs.Hypersurface(params=[hs.HypersurfaceParam("a", "quadratic", initial_fit_coeffts=[0.1, 0.2],
                                                       bounds=((-1, 1), (-2, 2)), coeff_prior_sigma=[1.0, 2.0])],
                          initial_intercept=None, log=False)
    assert new.params["a"].fit_coeffts is None and not new.params["a"].fitted and not new.fit_complete
    with pytest.raises(AssertionError, match="Duplicate"):
        hs.Hypersurface(params=[hs.HypersurfaceParam("a", "linear"), hs.HypersurfaceParam("a", "linear")])
    with pytest.raises(ValueError):
        hs.HypersurfaceParam("a", "cubic")


def test_state_json_round_trip_and_file_name(tmp_path):
    from pisa_amd.utils.jsons import to_json

    binning, maps, values, _ = _maps(log=True)
    hsf = hs.Hypersurface(params=_params(bounds=(-5, 5), coeff_prior_sigma=[10.0]), log=True)
    hsf.fit(maps[0], values[0], maps[1:], values[1:], solver=H.batch_solver)
    state = hsf.serializable_state
    assert state["fit_method"] == hs.FIT_METHOD and state["fit_info_stored"] is False
    assert state["fit_maps_raw"] is None and state["fit_maps_norm"] is None and state["fit_maps_smooth"] is None
    assert np.shape(state["intercept_sigma"]) == (4, 3) and np.shape(state["fit_chi2"]) == (4, 3, 9)
    ps = state["params"]["dom_eff"]
    assert ps["bounds"] == [[-5.0, 5.0]] and ps["coeff_prior_sigma"] == [10.0] and ps["initial_fit_coeffts"] == [0.0]
    assert ps["fit_param_values"] == [v["dom_eff"] for v in values] and np.shape(ps["fit_coeffts_sigma"]) == (4, 3, 1)
    name = hs.get_hypersurface_file_name(hsf, "unit")
    assert name == "unit__hypersurface_fits__2d__dom_eff_hole_ice.json"
    path = os.path.join(str(tmp_path), name)
    to_json({"nue_cc": hsf}, path)
    back = hs.load_hypersurfaces(path, expected_binning=binning)["nue_cc"]
    at = dict(dom_eff=1.07, hole_ice=22.0)
    want, want_unc = hsf.evaluate(at, return_uncertainty=True)
    got, got_unc = back.evaluate(at, return_uncertainty=True)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_unc, want_unc)
    assert np.all(want_unc > 0)
    np.testing.assert_array_equal(back.intercept_sigma, hsf.intercept_sigma)
