"""The profiled trial ensembles on the device (csrc/profile.hip: `pisa_hip_profiled_metric_matrix`,
`pisa_hip_profiled_metric_matrix_best` through `kernels.profiled_metric_matrix` / `profiled_metric_matrix_best`) and
the `response=` paths of pisa_amd/analysis/ensemble.py on example_hip.cfg.

The gate (tests/profile_cases.py): |got - exact| <= G eps S per entry, G = 4 max(1, G_REF[kind]) with G_REF the worst
ratio of the numpy restatement, measured on the CPU (tests/test_host_profiled.py).  Status flags are compared with
`==` against the restatement, the value with `==` against the direct form of `kernels.metric_matrix` on the pair's own
template row mu(eta_hat), placement and the reduced output with `==`.  `pytest -s` prints the kernels' own worst
ratios before each assertion.
"""
import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu


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


def _run(K, kind, f, rows=None, cols=None, max_iter=pc.MAX_ITER, **kw):
    d = f["D"] if rows is None else f["D"][rows]
    pick = (lambda a: a) if cols is None else (lambda a: None if a is None else a[cols])
    r = f["R"] if f["R"].ndim == 2 else pick(f["R"])
    return _host(K.profiled_metric_matrix(kind, _dev(K, d), _dev(K, pick(f["E"])), _dev(K, r), _dev(K, pick(f["S2"])),
                                          _dev(K, f["ips"]), _dev(K, pick(f["c"])), max_iter=max_iter, **kw))


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("fam", pc.GATED)
def test_every_entry_within_the_gate_of_the_exact_value(K, fam, kind):
    """every shape of the family: all pairs with status 0 and inside the gate; the fitted eta at the exact one"""
    worst, where, steps = 0.0, None, 0
    for shape in pc.shapes_of(fam):
        f = pc.family(fam, *shape)
        ex = pc.exact(fam, kind, *shape)
        got = _run(K, kind, f)
        what = "%s %s %s" % (fam, kind, shape)
        assert not got["status"].any(), (what, np.unique(got["status"]))
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, shape
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], pc.g_of(kind), what)
        eta = ex["eta"].astype(np.float64)
        assert np.all(np.abs(got["eta"] - eta) <= 1e-9 * (1.0 + np.abs(eta))), what
    print("%s %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps" % (fam, kind, worst, where,
                                                                                 pc.g_of(kind), steps))


@pytest.mark.parametrize("name", pc.STATUS_FAMILIES)
def test_flags_are_the_restatements(K, name):
    f = pc.status_family(name)
    want = pc.solve(f["kind"], f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
    got = _run(K, f["kind"], f, max_iter=f["max_iter"])
    assert want["status"].any()
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["n_iter"], want["n_iter"])
    assert np.all(np.isfinite(got["value"]))
    # a flagged pair holds the metric at its last accepted eta
    val, scale = pc.exact_value(f["kind"], f["D"], f["E"], f["R"], f["S2"], got["eta"].astype(np.longdouble),
                                f["ips"], f["c"])
    ec.check(got["value"], val, scale, pc.g_of(f["kind"]), name)


CASES_EQ = [("poisson", (65, 3, 65, 8)), ("prior", (64, 17, 64, 5)), ("shared", (63, 3, 3, 2)), ("asimov", (257, 3, 64, 2)),
            ("low", (63, 17, 65, 1))]


@pytest.mark.parametrize("kind", pc.KINDS)
def test_value_is_the_direct_form_on_the_fitted_template(K, kind):
    """value == `metric_matrix(form="direct")` of the data row against the ONE template row mu(eta_hat), recomputed on
    the host from the returned eta in the stated order, then the prior terms joined in ascending j"""
    for fam, shape in CASES_EQ:
        f = pc.family(fam, *shape)
        got = _run(K, kind, f)
        T, Kn, J = got["eta"].shape
        mu = pc._mu(f["E"], f["R"], got["eta"])                       # [T, K, B]
        ips = np.zeros(J) if f["ips"] is None else f["ips"]
        c = np.zeros((Kn, J)) if f["c"] is None else f["c"]
        for k in range(min(Kn, 3)):
            # row t of the data against row t of the templates mu[:, k]: the diagonal of a T x T matrix
            s2 = np.broadcast_to(f["S2"][k], mu[:, k].shape)
            m = K.metric_matrix(kind, _dev(K, f["D"]), _dev(K, mu[:, k]), _dev(K, s2), form="direct").cpu().numpy()
            want = pc.join_priors(kind, np.diagonal(m)[:, None], got["eta"][:, k:k + 1], ips, c[k:k + 1])[:, 0]
            assert np.array_equal(got["value"][:, k], want), (fam, shape, kind, k)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_placement_changes_no_bit(K, kind):
    for fam, shape in (("poisson", (65, 3, 65, 8)), ("prior", (64, 17, 64, 5)), ("shared", (257, 3, 64, 2))):
        f = pc.family(fam, *shape)
        T, Kn = shape[:2]
        full = _run(K, kind, f)
        rs = np.random.RandomState(5)
        pt, pk = rs.permutation(T), rs.permutation(Kn)
        got = _run(K, kind, f, rows=pt, cols=pk)
        for key in ("value", "eta", "n_iter", "status"):
            assert np.array_equal(got[key], full[key][pt][:, pk]), (fam, kind, key)
        for n in (2, 3):
            if T >= n:
                parts = [_run(K, kind, f, rows=p) for p in np.array_split(np.arange(T), n)]
                for key in ("value", "eta", "status"):
                    assert np.array_equal(np.concatenate([p[key] for p in parts]), full[key]), (fam, kind, key, n)
            if Kn >= n:
                parts = [_run(K, kind, f, cols=p) for p in np.array_split(np.arange(Kn), n)]
                for key in ("value", "eta", "status"):
                    assert np.array_equal(np.concatenate([p[key] for p in parts], axis=1), full[key]), (fam, kind, key, n)
        assert _run(K, kind, f, want_eta=False)["eta"] is None


@pytest.mark.parametrize("kind", pc.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_one(K, kind):
    # with few strips of trials the templates of a strip are split over workgroups and joined by a second launch (300,
    # 5, 17 and 3 ranges here); one template, or 2048 strips and more, and a strip's workgroup walks them all
    cases = [("poisson", pc.TILE_SHAPE), ("poisson", pc.STRIP_SHAPE), ("prior", (64, 17, 64, 5)),
             ("shared", (63, 3, 1, 5)), ("poisson", (257, 1, 130, 8)), ("poisson", (2048 * 64 + 1, 3, 3, 2))]
    for fam, shape in cases:
        f = pc.family(fam, *shape)
        Kn = shape[1]
        full = _run(K, kind, f)
        rs = np.random.RandomState(3)
        for offset, k0 in ((None, 0), (rs.randn(Kn), Kn - 1), (rs.randn(Kn), Kn // 2)):
            want = pc.reduce_profiled(kind, full, offset, k0)
            got = _host(K.profiled_metric_matrix_best(
                kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, f["S2"]), _dev(K, f["ips"]),
                _dev(K, f["c"]), _dev(K, offset), k0))
            for key in ("best", "arg", "at", "eta_best", "eta_at", "status"):
                assert np.array_equal(got[key], want[key]), (fam, shape, kind, key, k0)
    # the flags of both columns reach the trial: template 1 of `start` starts outside the domain
    f = pc.status_family("start")
    args = [_dev(K, f[n]) for n in ("D", "E", "R", "S2", "ips", "c")]
    for k0, flagged in ((1, True), (0, False)):
        got = _host(K.profiled_metric_matrix_best(f["kind"], *args, None, k0))
        full = _run(K, f["kind"], f)
        assert np.array_equal(got["status"], pc.reduce_profiled(f["kind"], full, None, k0)["status"])
        if flagged:
            assert np.all(got["status"] & pc.START_OUTSIDE)


def test_status_and_argument_checks(K):
    import torch

    from pisa_amd import _lib

    assert (_lib.PROFILE_NOT_CONVERGED, _lib.PROFILE_BOUNDARY, _lib.PROFILE_NOT_POSDEF, _lib.PROFILE_START_OUTSIDE) == (
        pc.NOT_CONVERGED, pc.BOUNDARY, pc.NOT_POSDEF, pc.START_OUTSIDE) and _lib.PROFILE_MAX_PARAMS == pc.MAX_PARAMS
    f = pc.family("poisson", 63, 3, 3, 2)
    for kind in pc.KINDS:
        for which in ("D", "E"):
            bad = dict(f)
            a = f[which].copy()
            a[1, 2] = -1.0
            bad[which] = a
            with pytest.raises(ValueError):
                _run(K, kind, bad)
            with pytest.raises(ValueError):
                K.profiled_metric_matrix_best(kind, _dev(K, bad["D"]), _dev(K, bad["E"]), _dev(K, f["R"]),
                                              _dev(K, f["S2"]))
    d, e, r, s2 = (_dev(K, f[n]) for n in ("D", "E", "R", "S2"))
    for call in (lambda: K.profiled_metric_matrix("barlow_llh", d, e, r),
                 lambda: K.profiled_metric_matrix("mod_chi2", d, e, r),
                 lambda: K.profiled_metric_matrix("llh", d, e, r[:, :, :2].contiguous()),
                 lambda: K.profiled_metric_matrix("llh", d, e, r[:2].contiguous()),
                 lambda: K.profiled_metric_matrix("llh", d, e, torch.zeros((3, 9, 3), dtype=torch.float64, device=d.device)),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, inv_prior_sigma=torch.ones(3, dtype=torch.float64, device=d.device)),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, center=torch.ones((2, 2), dtype=torch.float64, device=d.device)),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, max_iter=-1),
                 lambda: K.profiled_metric_matrix_best("llh", d, e, r, offset=torch.ones(2, dtype=torch.float64, device=d.device))):
        with pytest.raises(ValueError):
            call()
    # bins that do not match, k0 outside the templates, too many iterations: INVALID, nothing launched
    with pytest.raises(ValueError, match="bins"):
        K.profiled_metric_matrix("llh", d[:, :2].contiguous(), e, r)
    for call in (lambda: K.profiled_metric_matrix_best("llh", d, e, r, k0=3),
                 lambda: K.profiled_metric_matrix_best("llh", d, e, r, k0=-1),
                 lambda: K.profiled_metric_matrix("llh", d, e, r, max_iter=10 ** 6)):
        with pytest.raises(_lib.PisaHipError) as err:
            call()
        assert err.value.status == -1
    lib = _lib.lib()
    p = d.data_ptr()
    # NULL pointers, bad kinds, counts and sizes are refused before any device access
    assert lib.pisa_hip_profiled_metric_matrix(0, None, None, None, None, 0, None, None, 2, 32, 4, 4, 4, None, None, None, None, None, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(7, p, p, None, p, 0, None, None, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 0, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 9, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 2, 32, 0, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 2, 32, 4, 4, 2 ** 31, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 3, None, None, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    # more (strip, template) pairs than a grid holds workgroups of 64 lanes
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 2, 32, 64 * 2 ** 16, 2 ** 10 + 1, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(3, p, p, None, p, 0, None, None, 2, 32, 4, 4, 4, p, None, None, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix(0, p, p, None, p, 0, None, None, 2, 32, 4, 4, 4, p, None, None, None, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_best(0, p, p, None, p, 0, None, None, None, 0, 2, 32, 4, 4, 4, p, p, p, None, p, p, p, None) == -1
    assert lib.pisa_hip_profiled_metric_matrix_best(0, p, p, None, p, 0, None, None, None, 4, 2, 32, 4, 4, 4, p, p, p, p, p, p, p, None) == -1


# ------------------------------------------------------------------ config pipeline
def _maker(free):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    return dm


def test_nuisance_response_and_feldman_cousins_on_the_config_pipeline(K):
    """a 3-point theta23 grid of example_hip.cfg with aeff_scale and delta_index profiled through
    `NuisanceResponse.from_maker`.  With aeff_scale alone the template is exactly linear in the parameter, so the
    profiled llh of a pseudo-data map agrees inside the gate with `Map.metric_total` of the template the pipeline
    makes at the fitted value; `feldman_cousins(generator="device", response=...)` equals the loop over
    `delta_metric`."""
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    dm = _maker(("theta23", "aeff_scale", "delta_index"))
    th = dm.params["theta23"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.85, th, th * 1.12]})
    start = [p.value for p in dm.params.free]
    grid = en.TemplateGrid.from_maker(dm, pts, metric)
    one = en.NuisanceResponse.from_maker(dm, grid, ["aeff_scale"], {"aeff_scale": (-0.1, 0.1)})
    assert [p.value for p in dm.params.free] == start
    assert tuple(one.response.shape) == (3, 1, grid.n_bins) and one.names == ("aeff_scale",)
    prm = dm.params["aeff_scale"]
    prior_kind = "uniform" if prm.prior is None else prm.prior.kind
    assert (one.inv_prior_sigma[0] > 0) == (prior_kind == "gaussian")
    scale0 = float(prm.value.m_as(prm._units))
    assert np.all(one.values[:, 0] == scale0)
    # linear in aeff_scale: the response is the template per unit of the scale
    resp = one.response.cpu().numpy()[:, 0]
    assert np.allclose(resp * scale0, grid.host("hist"), rtol=1e-9, atol=1e-12 * grid.host("hist").max())
    # the pipeline's own template at the fitted value
    data = en.pseudo_data(grid, 1, 4, 11)
    out = K.profiled_metric_matrix(metric, K.to_device(data), grid.hist, one.response, None,
                                   K.to_device(one.inv_prior_sigma), K.to_device(one.center))
    out = _host(out)
    assert not out["status"].any()
    from pisa_amd.core.map import Map

    w = pc.w_of(metric)
    for t in range(2):
        for k in (0, 2):
            eta = float(out["eta"][t, k, 0])
            dm._set_rescaled_free_params(pts[k])
            dm.params["aeff_scale"].value = (scale0 + eta) * prm.value.units
            total = dm.get_outputs(return_sum=True)["total"]
            dmap = Map(name="data", hist=data[t].reshape(total.hist.shape), binning=total.binning)
            prior = w * (one.inv_prior_sigma[0] * (eta + one.center[k, 0])) ** 2
            want = dmap.metric_total(total, metric) - prior
            mu = total.nominal_values.ravel()
            # the gate's S on the kept bins (d > 0), the pipeline's template standing for mu
            kept = data[t] > 0
            slope = np.abs(1.0 - data[t] / np.maximum(mu, pc.SMALL_POS))
            S = float(ec.scale_fp64(metric, data[t:t + 1], mu[None, :])[0, 0]) + float(
                np.sum((slope * (np.abs(grid.host("hist")[k]) + np.abs(resp[k] * eta)))[kept])) + prior
            tol = pc.g_of(metric) * pc.EPS * S
            print("t %d k %d: eta %.6f profiled %.12g pipeline %.12g diff %.3g gate %.3g" % (
                t, k, eta, out["value"][t, k], want, abs(out["value"][t, k] - want), tol))
            assert abs(out["value"][t, k] - want) <= tol, (t, k)
    dm.set_free_params(start)
    # two parameters, the second with its Gaussian prior: no prior twice, the drivers against their own loop
    both = en.NuisanceResponse.from_maker(dm, grid, ["aeff_scale", "delta_index"],
                                          {"aeff_scale": (-0.1, 0.1), "delta_index": (-0.05, 0.05)})
    assert [p.value for p in dm.params.free] == start
    # every parameter's gradient is taken with the others at the point's own values: aeff_scale's is what it was alone
    assert np.array_equal(both.response.cpu().numpy()[:, 0], one.response.cpu().numpy()[:, 0])
    dm._set_rescaled_free_params(pts[1])
    alone = dm._fisher_templates(["delta_index"], {"delta_index": [dm.params["delta_index"].value + d * dm.params[
        "delta_index"].value.units for d in (-0.05, 0.05)]})["grad"].reshape(-1)
    assert np.array_equal(both.response.cpu().numpy()[1, 1], alone)
    dm.set_free_params(start)
    di = dm.params["delta_index"]
    assert both.inv_prior_sigma[1] == 1.0 / float(di.prior.stddev.magnitude)
    for k in range(3):
        dm._set_rescaled_free_params(pts[k])
        assert both.prior_at_point[k] == sum(dm.params[n].prior_penalty(metric) for n in both.names)
    dm.set_free_params(start)
    T, cl, seed = 64, (0.6827, 0.90), 7
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, generator="device", response=both)
    assert crit.shape == (3, 2) and info["flagged"].shape == (3,)
    solver = en.DeviceSolver()
    for k0 in range(3):
        data = solver.draw(grid.hist[k0], T, seed, stream=k0)
        delta, inf = en.delta_metric(data, grid, metric, k0, solver, both, return_info=True)
        assert np.array_equal(en.critical_values(delta, cl), crit[k0]) and inf["flagged"] == info["flagged"][k0]
        assert np.all(delta >= 0) and inf["eta_at"].shape == (T, 2)
    with pytest.raises(ValueError, match="not a free parameter"):
        en.NuisanceResponse.from_maker(dm, grid, ["nutau_norm_not_here"], {})
