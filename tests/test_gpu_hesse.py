"""The covariance of the fitted displacements on the device (csrc/profile_hesse.hip: `pisa_hip_profiled_hesse` through
`kernels.profiled_hesse`) against the exact reference in np.longdouble (tests/hesse_cases.py), inside the gate
G = 4 max(1, G_REF) in units of u = eps kappa max|exact| with G_REF measured on the CPU (tests/test_host_hesse.py), and
`covariance=True` / `pulls` of pisa_amd/analysis/ensemble.py on the device -- among them the closure test the feature
exists for: pseudo-data with truths drawn from unit priors, fitted, pulled.

Closure, measured on an MI355X (T = 4096, B = 24, J = 3, llh, means of order 1e6, seed 11; limits 5 / sqrt(T) = 0.078
and 5 sqrt(2 / T) = 0.110): the figures are printed by the test and quoted in DESIGN.md §4.
"""
import numpy as np
import pytest

from tests import hesse_cases as hc
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


def _dev(K, a, dtype=np.float64):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(K.device())


def _hesse(K, kind, f, eta, k, lower=None, upper=None):
    """`kernels.profiled_hesse` on a family's arrays -> host dict"""
    k = int(k) if np.ndim(k) == 0 else _dev(K, k, np.int32)
    out = K.profiled_hesse(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, eta), k, _dev(K, f["S2"]),
                           _dev(K, f["ips"]), _dev(K, f["c"]), _dev(K, lower), _dev(K, upper))
    T, J = eta.shape
    assert tuple(out["cov"].shape) == (T, J, J) and tuple(out["sigma"].shape) == (T, J) and tuple(out["status"].shape) == (T,)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _check(got, exact, kind, what):
    """status `==`, cov symmetric bit for bit and inside the gate -> the worst ratio"""
    assert np.array_equal(got["status"], exact["status"]), what
    cov = got["cov"]
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2), equal_nan=True), what
    none = (exact["status"] & hc.NO_COV) != 0
    assert np.isnan(cov[none]).all() and np.isfinite(cov[~none]).all(), what
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got["sigma"], np.sqrt(np.diagonal(cov, axis1=1, axis2=2)), equal_nan=True), what
    r = hc.ratio(cov, exact)
    assert r <= hc.gate(kind), (what, r)
    return r


@pytest.mark.parametrize("J", (1, 3, 8))
@pytest.mark.parametrize("kind", pc.KINDS)
def test_covariance_inside_the_gate_on_every_shape(K, kind, J):
    """(T, B, K) in {1, 63, 64, 65, 257} x {1, 15, 16, 17, 257} x {1, 3} at the point the data were drawn at: the template
    of trial t is t % K (it differs inside a wavefront), and once more one k0 for all"""
    worst = 0.0
    same = n = 0
    for n_k in (1, 3):
        for T in (1, 63, 64, 65, 257):
            for B in (1, 15, 16, 17, 257):
                f = pc.family("poisson", T, n_k, B, J)
                for k in (np.arange(T) % n_k, n_k - 1):
                    if n_k == 1 and np.ndim(k) == 0 and T > 1:
                        continue                    # (K = 1: both forms read the same rows; T = 1 keeps the k0 form)
                    exact = hc.hesse(kind, f["D"], f["E"], f["R"], f["eta0"], k, f["S2"], f["ips"], f["c"],
                                     dtype=np.longdouble)
                    assert not (exact["status"] & hc.NO_COV).any()
                    got = _hesse(K, kind, f, f["eta0"], k)
                    worst = max(worst, _check(got, exact, kind, (T, B, n_k, np.ndim(k))))
                    if T == 257 and B == 17:         # (the restatement itself: no library call lies on the way)
                        want = hc.hesse(kind, f["D"], f["E"], f["R"], f["eta0"], k, f["S2"], f["ips"], f["c"])
                        same += int(np.array_equal(got["cov"], want["cov"]))
                        n += 1
    print("%s J = %d: worst ratio %.2f of the gate's %.1f; %d of %d cases equal the restatement bit for bit"
          % (kind, J, worst, hc.gate(kind), same, n))


@pytest.mark.parametrize("kind", pc.KINDS)
def test_placement_and_fitted_points(K, kind):
    """at the fitted eta of a bounded family: inside the gate, and a permutation of the trials permutes the rows"""
    case = hc.fitted("poisson", kind, 257, 3, 17, 3, "narrow")
    f, ks, eta, lower, upper = case
    exact = hc.of_family(kind, case, np.longdouble)
    got = _hesse(K, kind, f, eta, ks, lower, upper)
    _check(got, exact, kind, "narrow")
    assert (got["status"] == hc.HELD).any() and (got["status"] == 0).any()
    perm = np.random.RandomState(3).permutation(257)
    g = dict(f, D=f["D"][perm])
    moved = _hesse(K, kind, g, eta[perm], ks[perm], lower, upper)
    for key in ("cov", "sigma", "status"):
        assert np.array_equal(moved[key], got[key][perm], equal_nan=True), key
    # a slice of the trials gives the slice of the rows
    part = _hesse(K, kind, dict(f, D=f["D"][100:170]), eta[100:170], ks[100:170], lower, upper)
    assert np.array_equal(part["cov"], got["cov"][100:170], equal_nan=True)
    # the shared response [J, B] and a box shared by all templates
    case = hc.fitted("shared", kind, 65, 3, 17, 3, "wide")
    _check(_hesse(K, kind, case[0], case[2], case[1], case[3], case[4]), hc.of_family(kind, case, np.longdouble), kind,
           "shared")


@pytest.mark.parametrize("kind", pc.KINDS)
def test_held_coordinates_and_infinite_bounds(K, kind):
    from tests.test_host_hesse import _edge_case

    f, ks, e, lower, upper = _edge_case(kind)
    got = _hesse(K, kind, f, e, ks, lower, upper)
    want = hc.hesse(kind, f["D"], f["E"], f["R"], e, ks, f["S2"], f["ips"], f["c"], lower, upper)
    assert np.array_equal(got["status"], want["status"])
    assert got["status"][0] == hc.HELD and got["status"][8] == hc.BAD_BOUNDS and np.isnan(got["cov"][8]).all()
    cov = got["cov"][0]
    assert np.all(cov[[0, 2], :] == 0.0) and np.all(cov[:, [0, 2]] == 0.0) and cov[1, 1] > 0.0
    assert np.array_equal(got["sigma"][0] == 0.0, [True, False, True])
    assert np.array_equal(got["cov"][2], got["cov"][0])                    # a point outside the box is held inside first
    assert np.all(got["cov"][1][2] == 0.0) and np.all(np.diagonal(got["cov"][1])[:2] > 0.0)
    _check(got, hc.hesse(kind, f["D"], f["E"], f["R"], e, ks, f["S2"], f["ips"], f["c"], lower, upper, np.longdouble),
           kind, "edge")
    # every bound infinite: the unbounded call, bit for bit
    f, ks, eta, _, _ = hc.fitted("poisson", kind, 65, 3, 17, 8)
    plain = _hesse(K, kind, f, eta, ks)
    inf = np.full((3, 8), np.inf)
    for lower, upper in ((-inf, inf), (-inf[0], None), (None, inf)):
        boxed = _hesse(K, kind, f, eta, ks, lower, upper)
        for key in ("cov", "sigma", "status"):
            assert np.array_equal(boxed[key], plain[key]), key
    assert not plain["status"].any()


def test_flagged_trials_and_bad_arguments(K):
    import torch

    from pisa_amd import _lib

    assert _lib.PROFILE_HELD == hc.HELD
    # as many parameters as bins and more, collinear: NOT_POSDEF, NaN
    s = pc.status_family("posdef")
    fam = dict(D=s["D"], E=s["E"], S2=s["S2"], R=s["R"], ips=None, c=None)
    for kind in pc.KINDS:
        got = _hesse(K, kind, fam, np.zeros((5, 3)), np.arange(5) % 2)
        assert np.all(got["status"] == hc.NOT_POSDEF) and np.isnan(got["cov"]).all() and np.isnan(got["sigma"]).all()
    s = pc.status_family("start")
    fam = dict(D=s["D"], E=s["E"], S2=s["S2"], R=s["R"], ips=s["ips"], c=None)
    got = _hesse(K, "poisson_llh", fam, np.zeros((4, 2)), np.arange(4) % 3)
    assert np.array_equal(got["status"], [0, hc.START_OUTSIDE, 0, 0]) and np.isnan(got["cov"][1]).all()
    assert np.isfinite(got["cov"][[0, 2, 3]]).all()
    # what the wrapper and the entry point refuse
    f = pc.family("poisson", 65, 3, 17, 3)
    d = {key: _dev(K, f[key]) for key in ("D", "E", "R", "S2", "ips", "c")}
    eta, ks = _dev(K, f["eta0"]), _dev(K, np.arange(65) % 3, np.int32)
    for call in (lambda: K.profiled_hesse("conv_llh", d["D"], d["E"], d["R"], eta, ks, d["S2"]),
                 lambda: K.profiled_hesse("mod_chi2", d["D"], d["E"], d["R"], eta, ks),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta[:, :2], ks),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta.float(), ks),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, ks[:64]),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, ks.long()),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, 3),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, -1),
                 lambda: K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, ks, lower=_dev(K, np.zeros(2))),
                 lambda: K.profiled_hesse("llh", -d["D"], d["E"], d["R"], eta, ks)):            # negative data
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_lib.PisaHipError) as err:                  # a template index outside the templates, on the device
        K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, _dev(K, np.arange(65) % 4, np.int32))
    assert err.value.status == -1
    lib = _lib.lib()
    cov = torch.full((65, 3, 3), -1.0, dtype=torch.float64, device=eta.device)
    st = torch.full((65,), -7, dtype=torch.int32, device=eta.device)
    status = torch.zeros(1, dtype=torch.int32, device=eta.device)
    p = {key: None if v is None else v.data_ptr() for key, v in d.items()}

    def raw(kind=0, D=p["D"], E=p["E"], S2=p["S2"], R=p["R"], r_stride=3 * 17, lower=None, upper=None, b_stride=0, J=3,
            T=65, n_k=3, B=17, k=ks.data_ptr(), k0=0, eta=eta.data_ptr(), cov=cov.data_ptr(), st=st.data_ptr(),
            status=status.data_ptr()):
        return lib.pisa_hip_profiled_hesse(kind, D, E, S2, R, r_stride, p["ips"], p["c"], lower, upper, b_stride, J, T,
                                           n_k, B, k, k0, eta, cov, st, status, None)

    for kw in (dict(kind=-1), dict(kind=4), dict(J=0), dict(J=9), dict(T=0), dict(n_k=0), dict(B=0), dict(T=2 ** 31),
               dict(D=None), dict(E=None), dict(R=None), dict(status=None), dict(eta=None), dict(cov=None),
               dict(st=None), dict(kind=3, S2=None), dict(r_stride=3 * 17 - 1), dict(lower=p["ips"], b_stride=2),
               dict(k=None, k0=3), dict(k=None, k0=-1)):
        assert raw(**kw) == -1, kw
    torch.cuda.synchronize()
    assert np.all(cov.cpu().numpy() == -1.0) and np.all(st.cpu().numpy() == -7) and int(status.item()) == 0
    assert raw(k=None, k0=2) == 0
    torch.cuda.synchronize()
    want = K.profiled_hesse("llh", d["D"], d["E"], d["R"], eta, 2, d["S2"], d["ips"], d["c"])
    assert np.array_equal(cov.cpu().numpy(), want["cov"].cpu().numpy()) and int(status.item()) == 0


def _maker(free):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    return dm


def test_delta_metric_returns_the_direct_calls_on_the_config_pipeline(K):
    """the 3-point theta23 grid of example_hip.cfg with aeff_scale and delta_index in a bounded response: with eta from
    `profiled_metric_matrix_best`, `delta_metric(return_info=True, covariance=True)` returns the arrays of the direct
    calls of `kernels.profiled_hesse`, and `pulls` is formed of them"""
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    dm = _maker(("theta23", "aeff_scale", "delta_index"))
    th = dm.params["theta23"].value
    grid = en.TemplateGrid.from_maker(dm, en.grid_points(dm, {"theta23": [th * 0.85, th, th * 1.12]}), metric)
    names = ["aeff_scale", "delta_index"]
    resp = en.NuisanceResponse.from_maker(dm, grid, names, {"aeff_scale": (-0.05, 0.05), "delta_index": (-0.05, 0.05)},
                                          bounded=True)
    T, k0, seed = 200, 1, 7
    data, truth = en.pseudo_data(grid, k0, T, seed, generator="device", response=resp, nuisance="prior", return_truth=True)
    plain, info0 = en.delta_metric(data, grid, metric, k0, response=resp, return_info=True)
    delta, info = en.delta_metric(data, grid, metric, k0, response=resp, return_info=True, covariance=True)
    assert np.array_equal(delta, plain)
    for key in info0:
        assert np.array_equal(info[key], info0[key]), key
    fit = K.profiled_metric_matrix_best(metric, data, grid.hist, resp.response, None, _dev(K, resp.inv_prior_sigma),
                                        _dev(K, resp.center), _dev(K, resp.offset(grid)), k0, lower=_dev(K, resp.lower),
                                        upper=_dev(K, resp.upper))
    assert np.array_equal(fit["eta_at"].cpu().numpy(), info["eta_at"])
    for which, k in (("best", fit["arg"]), ("at", k0)):
        direct = K.profiled_hesse(metric, data, grid.hist, resp.response, fit["eta_" + which], k, None,
                                  _dev(K, resp.inv_prior_sigma), _dev(K, resp.center), _dev(K, resp.lower),
                                  _dev(K, resp.upper))
        assert np.array_equal(info["cov_" + which], direct["cov"].cpu().numpy(), equal_nan=True)
        assert np.array_equal(info["sigma_" + which], direct["sigma"].cpu().numpy(), equal_nan=True)
        assert not (direct["status"].cpu().numpy() & hc.NO_COV).any()
    assert np.isfinite(info["cov_at"]).all() and np.mean(info["sigma_at"] > 0) > 0.9
    pulls = en.pulls(data, grid, metric, k0, resp, truth)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(info["sigma_at"] > 0, (info["eta_at"] - truth.cpu().numpy()) / info["sigma_at"], np.nan)
    assert np.array_equal(pulls, want, equal_nan=True)
    # delta_index is drawn from its prior and fitted with it: its pulls are of order 1
    assert 0.5 < np.nanstd(pulls[:, 1]) < 1.5 and abs(np.nanmean(pulls[:, 1])) < 0.5


def test_closure_of_the_pulls(K):
    """T = 4096 pseudo-experiments of 24 bins with means of order 1e6 (Poisson skewness and the clip far below the
    statistical error), three parameters with unit priors, truths drawn by `fluctuate_linear`, fitted by
    `profiled_metric_matrix_best`, covariance by `profiled_hesse`: per parameter the pulls' mean within 5 / sqrt(T) of
    0 and their variance within 5 sqrt(2 / T) of 1 (tests/test_host_hesse.py shows the numpy solver inside the same
    limits at this seed); every status word 0"""
    en, grid, resp, T, seed = hc.closure_inputs()
    grid = en.TemplateGrid(_dev(K, grid.hist), None, grid.points, None, None, "llh")
    resp = en.NuisanceResponse(resp.names, _dev(K, resp.response), resp.inv_prior_sigma, resp.center,
                               resp.prior_at_point, resp.values)
    data, truth = en.pseudo_data(grid, 0, T, seed, generator="device", response=resp, nuisance="prior", return_truth=True)
    _, info = en.delta_metric(data, grid, "llh", 0, response=resp, return_info=True, covariance=True)
    assert not info["status"].any() and not np.any(info["hesse_status"]) and info["flagged"] == 0
    pulls = en.pulls(data, grid, "llh", 0, resp, truth)
    assert pulls.shape == (T, 3) and np.isfinite(pulls).all()
    mean, var = pulls.mean(axis=0), pulls.var(axis=0)
    lim_mean, lim_var = hc.closure_limits(T)
    print("pulls: mean %s variance %s (limits %.3f, %.3f); sigma_at %s" % (mean, var, lim_mean, lim_var,
                                                                           info["sigma_at"].mean(axis=0)))
    assert np.all(np.abs(mean) <= lim_mean) and np.all(np.abs(var - 1.0) <= lim_var)
