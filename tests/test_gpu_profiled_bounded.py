"""The bounded profiled trial ensembles on the device (csrc/profile_bounded.hip: `pisa_hip_profiled_metric_matrix_bounded`,
`pisa_hip_profiled_metric_matrix_best_bounded` through the `lower=` / `upper=` of `kernels.profiled_metric_matrix` /
`profiled_metric_matrix_best`) and the bounded `response=` paths of pisa_amd/analysis/ensemble.py on example_hip.cfg.

The gate (tests/profile_bounded_cases.py): |got - exact| <= G eps S per entry, G = 4 max(1, G_REF_B[kind]) with G_REF_B
the worst ratio of the numpy restatement, measured on the CPU (tests/test_host_profiled_bounded.py).  Status, n_iter
and the set of coordinates on a bound are compared with `==` against the restatement; infinite bounds against the
unbounded entry points, pinned parameters against the direct form, placement and the reduced output with `==`.
`pytest -s` prints the kernels' own worst ratios before each assertion.
"""
import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc
from tests.test_host_profiled_bounded import check_status_family

pytestmark = pytest.mark.gpu

_RESTATED = {}


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


def _dev(K, a):
    import torch

    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(K.device())


def _host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _pick_bound(b, cols):
    return b if b is None or cols is None or np.ndim(b) == 1 else b[cols]


def _run(K, kind, f, lower, upper, rows=None, cols=None, max_iter=pc.MAX_ITER, **kw):
    d = f["D"] if rows is None else f["D"][rows]
    pick = (lambda a: a) if cols is None else (lambda a: None if a is None else a[cols])
    r = f["R"] if f["R"].ndim == 2 else pick(f["R"])
    return _host(K.profiled_metric_matrix(kind, _dev(K, d), _dev(K, pick(f["E"])), _dev(K, r), _dev(K, pick(f["S2"])),
                                          _dev(K, f["ips"]), _dev(K, pick(f["c"])), max_iter=max_iter,
                                          lower=_dev(K, _pick_bound(lower, cols)),
                                          upper=_dev(K, _pick_bound(upper, cols)), **kw))


def _best(K, kind, f, lower, upper, offset=None, k0=0):
    return _host(K.profiled_metric_matrix_best(
        kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, f["S2"]), _dev(K, f["ips"]), _dev(K, f["c"]),
        _dev(K, offset), k0, lower=_dev(K, lower), upper=_dev(K, upper)))


def _restated(name, bx, shape, kind):
    key = (name, bx, shape, kind)
    if key not in _RESTATED:
        f = pc.family(name, *shape)
        lower, upper = bc.box(bx, shape[1], shape[3])
        _RESTATED[key] = bc.solve_bounded(kind, f["D"], f["E"], f["R"], lower, upper, f["S2"], f["ips"], f["c"])
    return _RESTATED[key]


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("bx", bc.BOXES)
@pytest.mark.parametrize("fam", pc.GATED)
def test_every_entry_within_the_gate_of_the_exact_value(K, fam, bx, kind):
    """every shape of the family under the box: all pairs inside the gate; status, n_iter and the coordinates on a
    bound are the restatement's, and a coordinate on a bound holds the bound's own double"""
    worst, where, steps = 0.0, None, 0
    for shape in pc.shapes_of(fam):
        f = pc.family(fam, *shape)
        lower, upper = bc.box(bx, shape[1], shape[3])
        ex = bc.exact_bounded(fam, bx, kind, *shape)
        want = _restated(fam, bx, shape, kind)
        got = _run(K, kind, f, lower, upper)
        what = "%s %s %s %s" % (fam, bx, kind, shape)
        assert np.array_equal(got["status"], want["status"]) and not got["status"].any(), what
        assert np.array_equal(got["n_iter"], want["n_iter"]), what
        on = bc.on_bound(got["eta"], lower, upper)
        assert np.array_equal(on, bc.on_bound(want["eta"], lower, upper)), what
        assert np.array_equal(got["eta"][on != 0], want["eta"][on != 0]), what
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, shape
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], bc.g_of(kind), what)
        eta = ex["eta"].astype(np.float64)
        assert np.all(np.abs(got["eta"] - eta) <= 1e-9 * (1.0 + np.abs(eta))), what
    print("%s %s %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps" % (fam, bx, kind, worst, where,
                                                                                   bc.g_of(kind), steps))


CASES_EQ = [("poisson", (65, 3, 65, 8)), ("prior", (64, 17, 64, 5)), ("shared", (63, 3, 3, 2)), ("low", (63, 17, 65, 1))]


@pytest.mark.parametrize("kind", pc.KINDS)
def test_infinite_bounds_are_the_unbounded_entry_points_bit_for_bit(K, kind):
    for fam, shape in CASES_EQ + [("poisson", pc.TILE_SHAPE), ("poisson", pc.STRIP_SHAPE)]:
        f = pc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        args = [_dev(K, f[n]) for n in ("D", "E", "R", "S2", "ips", "c")]
        want = _host(K.profiled_metric_matrix(kind, *args))
        rs = np.random.RandomState(2)
        offset = rs.randn(Kn)
        want_best = _host(K.profiled_metric_matrix_best(kind, *args, _dev(K, offset), Kn // 2))
        for lower, upper in ((np.full(J, -np.inf), np.full(J, np.inf)), (np.full((Kn, J), -np.inf), None),
                             (None, np.full((Kn, J), np.inf))):
            got = _run(K, kind, f, lower, upper)
            for key in ("value", "eta", "n_iter", "status"):
                assert np.array_equal(got[key], want[key]), (fam, shape, kind, key)
            got = _best(K, kind, f, lower, upper, offset, Kn // 2)
            for key in ("best", "arg", "at", "eta_best", "eta_at", "status"):
                assert np.array_equal(got[key], want_best[key]), (fam, shape, kind, key)
    # the unbounded status families keep their flags
    for name in pc.STATUS_FAMILIES:
        f = pc.status_family(name)
        if f["kind"] != kind:
            continue
        args = [_dev(K, f[n]) for n in ("D", "E", "R", "S2", "ips", "c")]
        want = _host(K.profiled_metric_matrix(kind, *args, max_iter=f["max_iter"]))
        got = _run(K, kind, f, None, np.full(f["R"].shape[-2], np.inf), max_iter=f["max_iter"])
        for key in ("value", "eta", "n_iter", "status"):
            assert np.array_equal(got[key], want[key]), (name, key)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_pinned_at_zero_is_the_direct_form_plus_the_prior_chain(K, kind):
    for fam, shape in CASES_EQ:
        f = pc.family(fam, *shape)
        T, Kn, _, J = shape
        got = _run(K, kind, f, np.zeros(J), np.zeros((Kn, J)))
        assert not got["status"].any() and not got["n_iter"].any() and not got["eta"].any()
        m = K.metric_matrix(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"]), form="direct").cpu().numpy()
        ips = np.zeros(J) if f["ips"] is None else f["ips"]
        c = np.zeros((Kn, J)) if f["c"] is None else f["c"]
        want = pc.join_priors(kind, m, np.zeros((T, Kn, J)), ips, c)
        assert np.array_equal(got["value"], want), (fam, shape, kind)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_one(K, kind):
    # few strips: the templates of a strip are split over workgroups and joined (300, 5, 17 ranges); one template, or
    # 2048 strips and more: a strip's workgroup walks them all.  [K, J] bounds that differ from row to row
    cases = [("poisson", pc.TILE_SHAPE), ("poisson", pc.STRIP_SHAPE), ("prior", (64, 17, 64, 5)),
             ("poisson", (257, 1, 130, 8)), ("poisson", (2048 * 64 + 1, 3, 3, 2))]
    for fam, shape in cases:
        f = pc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        for lower, upper in (bc.own_rows_box(Kn, J), bc.box("wide", Kn, J)):
            full = _run(K, kind, f, lower, upper)
            if np.ndim(lower) == 2 and Kn >= 3:
                # every template is fitted in its own row's box: row 1 is pinned at 0.01, row 2 has no upper bound
                lo, hi = bc.full_bounds(lower, upper, Kn, J)
                assert np.all(full["eta"] >= lo[None]) and np.all(full["eta"] <= hi[None])
                assert np.all(full["eta"][:, 1] == 0.01) and np.any(full["eta"][:, 0] == lo[0][None])
                assert np.any(full["eta"][:, 2] > hi[0][None])
            rs = np.random.RandomState(3)
            for offset, k0 in ((None, 0), (rs.randn(Kn), Kn - 1), (rs.randn(Kn), Kn // 2)):
                want = pc.reduce_profiled(kind, full, offset, k0)
                got = _best(K, kind, f, lower, upper, offset, k0)
                for key in ("best", "arg", "at", "eta_best", "eta_at", "status"):
                    assert np.array_equal(got[key], want[key]), (fam, shape, kind, key, k0)
    # the flags of both columns reach the trial: template 1 of `bad` carries BAD_BOUNDS
    f = bc.status_family("bad")
    for k0, flagged in ((1, True), (0, False)):
        got = _best(K, f["kind"], f, f["lower"], f["upper"], None, k0)
        full = _run(K, f["kind"], f, f["lower"], f["upper"])
        assert np.array_equal(got["status"], pc.reduce_profiled(f["kind"], full, None, k0)["status"])
        if flagged:
            assert np.all(got["status"] & bc.BAD_BOUNDS)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_placement_changes_no_bit(K, kind):
    for fam, shape in (("poisson", (65, 3, 65, 8)), ("prior", (64, 17, 64, 5)), ("shared", (257, 3, 64, 2))):
        f = pc.family(fam, *shape)
        T, Kn, _, J = shape
        lower, upper = bc.own_rows_box(Kn, J)
        full = _run(K, kind, f, lower, upper)
        rs = np.random.RandomState(5)
        pt, pk = rs.permutation(T), rs.permutation(Kn)
        got = _run(K, kind, f, lower, upper, rows=pt, cols=pk)
        for key in ("value", "eta", "n_iter", "status"):
            assert np.array_equal(got[key], full[key][pt][:, pk]), (fam, kind, key)
        for n in (2, 3):
            parts = [_run(K, kind, f, lower, upper, rows=p) for p in np.array_split(np.arange(T), n)]
            for key in ("value", "eta", "status"):
                assert np.array_equal(np.concatenate([p[key] for p in parts]), full[key]), (fam, kind, key, n)
            parts = [_run(K, kind, f, lower, upper, cols=p) for p in np.array_split(np.arange(Kn), n)]
            for key in ("value", "eta", "status"):
                assert np.array_equal(np.concatenate([p[key] for p in parts], axis=1), full[key]), (fam, kind, key, n)
        assert _run(K, kind, f, lower, upper, want_eta=False)["eta"] is None


@pytest.mark.parametrize("name", bc.STATUS_FAMILIES)
def test_status_families(K, name):
    f = bc.status_family(name)
    want = bc.solve_bounded(f["kind"], f["D"], f["E"], f["R"], f["lower"], f["upper"], f["S2"], f["ips"], f["c"],
                            f["max_iter"])
    got = _run(K, f["kind"], f, f["lower"], f["upper"], max_iter=f["max_iter"])
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["n_iter"], want["n_iter"])
    check_status_family(name, f, got)
    val, scale = pc.exact_value(f["kind"], f["D"], f["E"], f["R"], f["S2"], got["eta"].astype(np.longdouble),
                                f["ips"], f["c"])
    ec.check(got["value"], val, scale, bc.g_of(f["kind"]), name)


def test_status_and_argument_checks(K):
    import torch

    from pisa_amd import _lib

    assert _lib.PROFILE_BAD_BOUNDS == bc.BAD_BOUNDS == 16
    f = pc.family("poisson", 63, 3, 3, 2)
    d, e, r, s2 = (_dev(K, f[n]) for n in ("D", "E", "R", "S2"))
    lo, hi = _dev(K, np.array([-0.1, -0.2])), _dev(K, np.array([0.1, 0.2]))
    lo2, hi2 = lo.expand(3, 2).contiguous(), hi.expand(3, 2).contiguous()
    # lower alone, upper alone, [J] and [K, J], and one of each: the same fit where the boxes are the same
    both = _host(K.profiled_metric_matrix("llh", d, e, r, lower=lo, upper=hi))
    for kw in (dict(lower=lo2, upper=hi2), dict(lower=lo, upper=hi2), dict(lower=lo2, upper=hi)):
        got = _host(K.profiled_metric_matrix("llh", d, e, r, **kw))
        for key in ("value", "eta", "n_iter", "status"):
            assert np.array_equal(got[key], both[key]), (key, kw.keys())
    only_lo = _host(K.profiled_metric_matrix("llh", d, e, r, lower=lo))
    only_hi = _host(K.profiled_metric_matrix("llh", d, e, r, upper=hi2))
    assert np.all(only_lo["eta"] >= np.array([-0.1, -0.2])) and np.any(only_lo["eta"] > np.array([0.1, 0.2]))
    assert np.all(only_hi["eta"] <= np.array([0.1, 0.2])) and np.any(only_hi["eta"] < np.array([-0.1, -0.2]))
    assert not only_lo["status"].any() and not only_hi["status"].any()
    assert K.profiled_metric_matrix_best("llh", d, e, r, lower=lo)["best"].shape == (63,)
    f4 = torch.float32
    for call in (lambda: K.profiled_metric_matrix("llh", d, e, r, lower=lo[:1].contiguous()),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, upper=hi2[:2].contiguous()),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, lower=lo.to(f4)),
                 lambda: K.profiled_metric_matrix_best("llh", d, e, r, upper=torch.zeros((3, 3), dtype=torch.float64, device=d.device)),
                 lambda: K.profiled_metric_matrix("barlow_llh", d, e, r, lower=lo),
                 lambda: K.profiled_metric_matrix("mod_chi2", d, e, r, lower=lo)):
        with pytest.raises(ValueError):
            call()
    # a negative datum is reported by the bounded form as by the unbounded one
    bad = f["D"].copy()
    bad[1, 2] = -1.0
    with pytest.raises(ValueError):
        K.profiled_metric_matrix("llh", _dev(K, bad), e, r, lower=lo)
    lib = _lib.lib()
    p = d.data_ptr()
    # a bound stride that is neither 0 nor >= J, NULL pointers and bad counts are refused before any device access
    ok = (0, p, p, None, p, 0, None, None)
    assert lib.pisa_hip_profiled_metric_matrix_bounded(*ok, p, p, 1, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_bounded(*ok, p, p, -2, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_bounded(*ok, None, None, 1, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_bounded(*ok, p, p, 0, 9, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_bounded(*ok, p, p, 0, 2, 32, 4, 4, 4, p, None, None, None, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_bounded(0, None, None, None, None, 0, None, None, None, None, 0, 2, 32, 4, 4, 4, None, None, None, None, None, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_best_bounded(*ok, p, p, 1, None, 0, 2, 32, 4, 4, 4, p, p, p, p, p, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_best_bounded(*ok, p, p, 0, None, 4, 2, 32, 4, 4, 4, p, p, p, p, p, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_best_bounded(*ok, p, p, 0, None, 0, 2, 32, 4, 4, 4, p, p, p, None, p, p, p, None) == -1


# ------------------------------------------------------------------ config pipeline
def _maker(free):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    return dm


def test_bounded_response_and_feldman_cousins_on_the_config_pipeline(K):
    """the 3-point theta23 grid of tests/test_gpu_profiled.py with aeff_scale and delta_index profiled inside their
    ranges (`NuisanceResponse.from_maker(bounded=True)`), the range of aeff_scale narrowed so that it binds for part
    of the trials: values + eta stays inside the range and sits exactly on its edge for some trials, the bounded
    profiled distance lies between the unbounded one and the unprofiled one, and `feldman_cousins` on the device
    equals the numpy solver's result within the gate"""
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    dm = _maker(("theta23", "aeff_scale", "delta_index"))
    prm = dm.params["aeff_scale"]
    scale0 = float(prm.value.m_as(prm._units))
    # the statistical error of the normalisation of a pseudo-data map is about 1 / sqrt(N): the range of aeff_scale
    # becomes a third of it to either side, before the grid is made (the grid's points are rescaled by the ranges)
    n_tot = float(np.asarray(dm.get_outputs(return_sum=True)["total"].nominal_values).sum())
    half = 0.3 * scale0 / np.sqrt(n_tot)
    prm.range = [(scale0 - half) * prm.value.units, (scale0 + half) * prm.value.units]
    th = dm.params["theta23"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.85, th, th * 1.12]})
    start = [p.value for p in dm.params.free]
    grid = en.TemplateGrid.from_maker(dm, pts, metric)
    names = ["aeff_scale", "delta_index"]
    tv = {"aeff_scale": (-0.5 * half, 0.5 * half), "delta_index": (-0.05, 0.05)}
    free = en.NuisanceResponse.from_maker(dm, grid, names, tv)
    assert not free.bounded and free.lower is None and free.upper is None and free.bounds() == {}
    resp = en.NuisanceResponse.from_maker(dm, grid, names, tv, bounded=True)
    assert [p.value for p in dm.params.free] == start
    assert resp.bounded and resp.lower.shape == resp.upper.shape == (3, 2)
    for j, name in enumerate(names):
        p = dm.params[name]
        r0, r1 = (float(x.m_as(p._units)) for x in p.range)
        assert np.array_equal(resp.lower[:, j], r0 - resp.values[:, j])
        assert np.array_equal(resp.upper[:, j], r1 - resp.values[:, j])
    assert np.array_equal(free.response.cpu().numpy(), resp.response.cpu().numpy())
    lo_edge, hi_edge = (float(x.m_as(prm._units)) for x in prm.range)
    solver = en.DeviceSolver()
    T, cl, seed = 64, (0.6827, 0.90), 7
    data = solver.draw(grid.hist[1], T, seed, stream=1)
    host_data = data.cpu().numpy()
    out = _host(solver.profiled_matrix(metric, data, grid.hist, resp.response, None, resp.inv_prior_sigma, resp.center,
                                       resp.max_iter, **resp.bounds()))
    assert not out["status"].any()
    value = resp.values[None, :, 0] + out["eta"][:, :, 0]
    assert np.all(value >= lo_edge) and np.all(value <= hi_edge)
    at_edge = (out["eta"][:, :, 0] == resp.lower[None, :, 0]) | (out["eta"][:, :, 0] == resp.upper[None, :, 0])
    assert at_edge.any() and not at_edge.all()
    print("aeff_scale on the edge of its range in %d of %d pairs" % (np.count_nonzero(at_edge), at_edge.size))
    # the device against the numpy solver, pair by pair
    R = resp.response.cpu().numpy()
    want = bc.restated_bounded(metric, host_data, grid.host("hist"), R, resp.lower, resp.upper, None,
                               resp.inv_prior_sigma, resp.center)
    assert np.array_equal(out["status"], want["status"]) and np.array_equal(out["n_iter"], want["n_iter"])
    assert np.array_equal(out["eta"] == resp.lower[None], want["eta"] == resp.lower[None])
    assert np.array_equal(out["eta"] == resp.upper[None], want["eta"] == resp.upper[None])
    _, S = pc.exact_value(metric, host_data, grid.host("hist"), R, None, want["eta"].astype(np.longdouble),
                          resp.inv_prior_sigma, resp.center)
    tol = (bc.g_of(metric) + pc.g_of(metric)) * pc.EPS * S        # (device and restatement each within their gate)
    assert np.all(np.abs(out["value"] - want["value"]) <= tol)
    # unbounded >= bounded >= unprofiled (llh: larger is better), entry by entry up to the gate
    m_free = _host(solver.profiled_matrix(metric, data, grid.hist, free.response, None, free.inv_prior_sigma,
                                          free.center, free.max_iter))["value"]
    pinned = en.NuisanceResponse(names, resp.response, resp.inv_prior_sigma, resp.center, resp.prior_at_point,
                                 resp.values, lower=np.zeros(2), upper=np.zeros(2))
    m_pin = _host(solver.profiled_matrix(metric, data, grid.hist, pinned.response, None, pinned.inv_prior_sigma,
                                         pinned.center, pinned.max_iter, **pinned.bounds()))["value"]
    assert np.all(m_free - out["value"] >= -tol) and np.any(m_free - out["value"] > 1e-6)
    assert np.all(out["value"] - m_pin >= -tol) and np.any(out["value"] - m_pin > 1e-6)
    # feldman_cousins on the device against the numpy solver, within the gate of every distance
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=resp)
    assert crit.shape == (3, 2) and info["flagged"].shape == (3,) and not info["flagged"].any()

    class _Numpy(bc.NumpyBoundedProfileSolver):
        def draw(self, mu, n_trials, seed, stream, first_trial=0):
            return solver.draw(mu, n_trials, seed, stream, first_trial).cpu().numpy()

    host_grid = en.TemplateGrid(grid.host("hist"), grid.host("sumw2"), grid.points, None, grid.penalty, metric)
    host_resp = en.NuisanceResponse(names, R, resp.inv_prior_sigma, resp.center, resp.prior_at_point, resp.values,
                                    resp.max_iter, resp.lower, resp.upper)
    want_crit, _ = en.feldman_cousins(host_grid, metric, T, cl, seed, solver=_Numpy(), generator="device",
                                      response=host_resp)
    # a critical value is one of the distances best - at: two entries, each within its gate
    assert np.all(np.abs(crit - want_crit) <= 2 * tol.max()), (crit, want_crit)
    for k0 in range(3):
        d = solver.draw(grid.hist[k0], T, seed, stream=k0)
        delta, inf = en.delta_metric(d, grid, metric, k0, solver, resp, return_info=True)
        assert np.array_equal(en.critical_values(delta, cl), crit[k0]) and np.all(delta >= 0)
        d_free = en.delta_metric(d, grid, metric, k0, solver, free)
        assert inf["eta_at"].shape == (T, 2) and d_free.shape == delta.shape
    dm.set_free_params(start)
