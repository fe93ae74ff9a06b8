"""The wide form of the profiled trial ensembles on the device (csrc/profile_wide.hip:
`pisa_hip_profiled_metric_matrix_wide`, `pisa_hip_profiled_metric_matrix_best_wide` through
`kernels.profiled_metric_matrix_wide` / `profiled_metric_matrix_best_wide`) and the `wide=` paths of
pisa_amd/analysis/ensemble.py with `DeviceSolver`.

Up to 8 parameters every output `==` that of the narrow kernels (profile.hip, profile_bounded.hip).  Above, the
comparison is that of tests/test_gpu_profiled.py and tests/test_gpu_profiled_bounded.py against the numpy restatements:
status, n_iter and the coordinates on a bound with `==`, the value inside the gate |got - exact| <= G eps S with G from
G_REF_W / G_REF_WB of tests/profile_wide_cases.py (measured on the CPU).  `pytest -s` prints the kernels' own worst
ratios before each assertion.
"""
import ctypes

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc
from tests import profile_wide_cases as wc

pytestmark = pytest.mark.gpu

FULL_KEYS = ("value", "eta", "n_iter", "status")
BEST_KEYS = ("best", "arg", "at", "eta_best", "eta_at", "status")
SPLIT_BELOW = 4096             # PFW_FILL_BLOCKS: with fewer trials the templates of the reduced output are split


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


def _run(K, kind, f, lower=None, upper=None, rows=None, cols=None, max_iter=pc.MAX_ITER, wide=True, **kw):
    d = f["D"] if rows is None else f["D"][rows]
    pick = (lambda a: a) if cols is None else (lambda a: None if a is None else a[cols])
    r = f["R"] if f["R"].ndim == 2 else pick(f["R"])
    fn = K.profiled_metric_matrix_wide if wide else K.profiled_metric_matrix
    return _host(fn(kind, _dev(K, d), _dev(K, pick(f["E"])), _dev(K, r), _dev(K, pick(f["S2"])), _dev(K, f["ips"]),
                    _dev(K, pick(f["c"])), max_iter=max_iter, lower=_dev(K, _pick_bound(lower, cols)),
                    upper=_dev(K, _pick_bound(upper, cols)), **kw))


def _best(K, kind, f, lower=None, upper=None, offset=None, k0=0, rows=None, max_iter=pc.MAX_ITER, wide=True):
    fn = K.profiled_metric_matrix_best_wide if wide else K.profiled_metric_matrix_best
    d = f["D"] if rows is None else f["D"][rows]
    return _host(fn(kind, _dev(K, d), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, f["S2"]), _dev(K, f["ips"]),
                    _dev(K, f["c"]), _dev(K, offset), k0, max_iter=max_iter, lower=_dev(K, lower),
                    upper=_dev(K, upper)))


def _same(got, want, keys, what):
    for key in keys:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


# --------------------------------------------------------------------------- 1. wide == narrow up to 8 parameters
def _narrow_cases():
    cases = [("poisson", s) for s in pc.SHAPES + (pc.STRIP_SHAPE, pc.TILE_SHAPE)]
    cases += [("prior", (64, 17, 64, 5)), ("prior", (65, 3, 65, 8)), ("shared", (63, 3, 3, 2)), ("shared", (63, 3, 1, 5)),
              ("asimov", (257, 3, 64, 2)), ("low", (63, 17, 65, 1)), ("far", (65, 1, 3, 1))]
    return cases


@pytest.mark.parametrize("kind", pc.KINDS)
def test_wide_is_narrow_bit_for_bit_up_to_8_parameters(K, kind):
    n = 0
    for fam, shape in _narrow_cases():
        f = pc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        rs = np.random.RandomState(7)
        offset, k0 = rs.randn(Kn), Kn // 2
        boxes = [(None, None)] + [bc.box(bx, Kn, J) for bx in bc.BOXES] + [bc.own_rows_box(Kn, J)]
        for lower, upper in boxes:
            what = (fam, shape, kind, None if lower is None else np.shape(lower))
            _same(_run(K, kind, f, lower, upper), _run(K, kind, f, lower, upper, wide=False), FULL_KEYS, what)
            _same(_best(K, kind, f, lower, upper, offset, k0), _best(K, kind, f, lower, upper, offset, k0, wide=False),
                  BEST_KEYS, what)
            n += 1
    for name in pc.STATUS_FAMILIES:
        f = pc.status_family(name)
        if f["kind"] == kind:
            want = _run(K, kind, f, max_iter=f["max_iter"], wide=False)
            assert want["status"].any()
            _same(_run(K, kind, f, max_iter=f["max_iter"]), want, FULL_KEYS, name)
            n += 1
    for name in bc.STATUS_FAMILIES:
        f = bc.status_family(name)
        if f["kind"] == kind:
            args = (f["lower"], f["upper"])
            k0 = min(1, f["E"].shape[0] - 1)
            _same(_run(K, kind, f, *args, max_iter=f["max_iter"]),
                  _run(K, kind, f, *args, max_iter=f["max_iter"], wide=False), FULL_KEYS, name)
            _same(_best(K, kind, f, *args, None, k0, max_iter=f["max_iter"]),
                  _best(K, kind, f, *args, None, k0, max_iter=f["max_iter"], wide=False), BEST_KEYS, name)
            n += 1
    print("%s: %d cases, every output of the wide form equal to the narrow one" % (kind, n))


# ------------------------------------------------------------------ 2. against the restatement above 8 parameters
@pytest.mark.parametrize("kind", pc.KINDS)
def test_every_entry_within_the_gate_of_the_exact_value(K, kind):
    worst, where, steps = 0.0, None, 0
    for fam, shape in wc.GATED:
        f = pc.family(fam, *shape)
        ex = pc.exact(fam, kind, *shape)
        want = wc.restated(fam, kind, shape)
        got = _run(K, kind, f)
        what = "%s %s %s" % (fam, kind, shape)
        assert np.array_equal(got["status"], want["status"]) and not got["status"].any(), (what, np.unique(got["status"]))
        assert np.array_equal(got["n_iter"], want["n_iter"]), what
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, (fam, shape)
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], wc.g_of(kind), what)
        eta = ex["eta"].astype(np.float64)
        assert np.all(np.abs(got["eta"] - eta) <= 1e-9 * (1.0 + np.abs(eta))), what
    print("wide %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps" % (kind, worst, where, wc.g_of(kind),
                                                                                  steps))


@pytest.mark.parametrize("kind", pc.KINDS)
def test_every_bounded_entry_within_the_gate_of_the_exact_value(K, kind):
    worst, where, steps = 0.0, None, 0
    for fam, bx, shape in wc.GATED_BOUNDED:
        f = pc.family(fam, *shape)
        lower, upper = wc.bounds(bx, shape[1], shape[3])
        ex = bc.exact_bounded(fam, bx, kind, *shape)
        want = wc.restated(fam, kind, shape, bx)
        got = _run(K, kind, f, lower, upper)
        what = "%s %s %s %s" % (fam, bx, kind, shape)
        assert np.array_equal(got["status"], want["status"]) and not got["status"].any(), what
        assert np.array_equal(got["n_iter"], want["n_iter"]), what
        on = bc.on_bound(got["eta"], lower, upper)
        assert np.array_equal(on, bc.on_bound(want["eta"], lower, upper)) and (on != 0).any(), what
        assert np.array_equal(got["eta"][on != 0], want["eta"][on != 0]), what
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, (fam, bx, shape)
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], wc.g_of(kind, True), what)
        eta = ex["eta"].astype(np.float64)
        assert np.all(np.abs(got["eta"] - eta) <= 1e-9 * (1.0 + np.abs(eta))), what
    print("wide bounded %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps"
          % (kind, worst, where, wc.g_of(kind, True), steps))


@pytest.mark.parametrize("kind", pc.KINDS)
def test_flagged_pairs_are_the_restatements(K, kind):
    """the J > B shape: status and n_iter `==` the restatement, eta `==` where the pair is flagged in neither (a
    flagged pair's last eta is compared through its value), every value inside the gate around the exact value at the
    returned eta"""
    for fam, shape in wc.UNGATED:
        f = pc.family(fam, *shape)
        want = wc.restated(fam, kind, shape)
        got = _run(K, kind, f)
        what = "%s %s %s" % (fam, kind, shape)
        print("%s: statuses %s, at most %d Newton steps" % (what, dict(zip(*np.unique(got["status"], return_counts=True))),
                                                           got["n_iter"].max()))
        assert np.array_equal(got["status"], want["status"]), what
        assert np.array_equal(got["n_iter"], want["n_iter"]), what
        assert np.all(np.isfinite(got["value"]))
        val, scale = pc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], got["eta"].astype(np.longdouble), f["ips"],
                                    f["c"])
        ec.check(got["value"], val, scale, wc.g_of(kind), what)


# ----------------------------------------------------------------------------- 3. pinned parameters, 4. no bounds
@pytest.mark.parametrize("kind", pc.KINDS)
def test_32_parameters_pinned_at_zero_are_the_direct_form_plus_the_prior_chain(K, kind):
    for fam, shape in (("poisson", (2, 2, 130, 32)), ("prior", (66, 2, 20, 32))):
        f = pc.family(fam, *shape)
        T, Kn, _, J = shape
        got = _run(K, kind, f, np.zeros(J), np.zeros((Kn, J)))
        assert not got["status"].any() and not got["n_iter"].any() and not got["eta"].any()
        m = K.metric_matrix(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"]), form="direct").cpu().numpy()
        c = np.zeros((Kn, J)) if f["c"] is None else f["c"]
        want = pc.join_priors(kind, m, np.zeros((T, Kn, J)), f["ips"], c)
        assert np.array_equal(got["value"], want), (fam, shape, kind)


@pytest.mark.parametrize("kind", pc.KINDS)
def test_infinite_bounds_are_the_call_without_bounds_bit_for_bit(K, kind):
    for fam, shape in (("poisson", (3, 2, 64, 16)), ("prior", (2, 3, 63, 17)), ("prior", (66, 2, 20, 32)),
                       ("poisson", (8, 300, 12, 12)), ("poisson", (65, 3, 65, 8))):
        f = pc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        want = _run(K, kind, f)
        offset = np.random.RandomState(2).randn(Kn)
        want_best = _best(K, kind, f, None, None, offset, Kn // 2)
        for lower, upper in ((np.full(J, -np.inf), np.full(J, np.inf)), (np.full((Kn, J), -np.inf), None),
                             (None, np.full((Kn, J), np.inf))):
            _same(_run(K, kind, f, lower, upper), want, FULL_KEYS, (fam, shape, kind))
            _same(_best(K, kind, f, lower, upper, offset, Kn // 2), want_best, BEST_KEYS, (fam, shape, kind))


# --------------------------------------------------------------------------------- 5. the reduced output
@pytest.mark.parametrize("kind", pc.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_one(K, kind):
    # fewer than 4096 trials: the templates of a trial are split over workgroups and joined by a second launch; one
    # template, or 4096 trials and more: the trial's workgroup walks them all
    big = pc.family("poisson", SPLIT_BELOW + 1, 3, 3, 2)
    cases = [("poisson", (8, 300, 12, 12), None), ("prior", (66, 2, 20, 32), None), ("poisson", (2, 3, 63, 17), None),
             ("poisson", (1, 1, 1, 9), None), ("poisson", (SPLIT_BELOW + 1, 3, 3, 2), None),
             ("poisson", (SPLIT_BELOW + 1, 3, 3, 2), np.arange(SPLIT_BELOW - 1)),
             ("poisson", (SPLIT_BELOW + 1, 3, 3, 2), np.arange(SPLIT_BELOW))]
    assert big["D"].shape[0] == SPLIT_BELOW + 1
    for fam, shape, rows in cases:
        f = pc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        for lower, upper in ((None, None), bc.own_rows_box(Kn, J)):
            full = _run(K, kind, f, lower, upper, rows=rows)
            rs = np.random.RandomState(3)
            for offset, k0 in ((None, 0), (rs.randn(Kn), Kn - 1), (rs.randn(Kn), Kn // 2)):
                want = pc.reduce_profiled(kind, full, offset, k0)
                got = _best(K, kind, f, lower, upper, offset, k0, rows=rows)
                _same(got, want, BEST_KEYS, (fam, shape, kind, k0, None if rows is None else rows.size))
    # placement changes no bit: permutations and splits of the trials and of the templates
    fam, shape = "poisson", (8, 300, 12, 12)
    f = pc.family(fam, *shape)
    T, Kn = shape[:2]
    full = _run(K, kind, f)
    rs = np.random.RandomState(5)
    pt, pk = rs.permutation(T), rs.permutation(Kn)
    got = _run(K, kind, f, rows=pt, cols=pk)
    for key in FULL_KEYS:
        assert np.array_equal(got[key], full[key][pt][:, pk]), key
    for n in (2, 3):
        parts = [_run(K, kind, f, rows=p) for p in np.array_split(np.arange(T), n)]
        for key in FULL_KEYS:
            assert np.array_equal(np.concatenate([p[key] for p in parts]), full[key]), (key, n)
        parts = [_run(K, kind, f, cols=p) for p in np.array_split(np.arange(Kn), n)]
        for key in FULL_KEYS:
            assert np.array_equal(np.concatenate([p[key] for p in parts], axis=1), full[key]), (key, n)
    # ties keep the smallest template: every template the same row
    tie = dict(f, E=np.tile(f["E"][:1], (Kn, 1)), S2=np.tile(f["S2"][:1], (Kn, 1)), R=np.tile(f["R"][:1], (Kn, 1, 1)))
    got = _best(K, kind, tie, None, None, None, Kn - 1)
    assert not got["arg"].any() and np.array_equal(got["best"], got["at"])
    assert _run(K, kind, f, want_eta=False)["eta"] is None


# --------------------------------------------------------------------------------- 6. the raw entry points
def test_raw_entry_points_refuse_before_any_launch_and_junk_stays_in_its_pair(K):
    import torch

    from pisa_amd import _lib

    assert _lib.PROFILE_WIDE_MAX_PARAMS == wc.MAX_PARAMS == 32 and _lib.PROFILE_MAX_PARAMS == 8
    lib = _lib.lib()
    T, Kn, B, J = 3, 2, 40, 9
    f = pc.family("poisson", T, Kn, B, J)
    dev = K.device()
    d, e, r, s2 = (_dev(K, f[n]) for n in ("D", "E", "R", "S2"))
    poison = 12345.0
    value = torch.full((T, Kn), poison, dtype=torch.float64, device=dev)
    pst = torch.full((T, Kn), -7, dtype=torch.int32, device=dev)
    best, at = (torch.full((T,), poison, dtype=torch.float64, device=dev) for _ in range(2))
    eb, ea = (torch.full((T, J), poison, dtype=torch.float64, device=dev) for _ in range(2))
    arg, tst = (torch.full((T,), -7, dtype=torch.int32, device=dev) for _ in range(2))
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def full(n_params=J, data=d, expected=e, response=r, out=value, pair=pst, st=status, max_iter=32, kind=0):
        return lib.pisa_hip_profiled_metric_matrix_wide(kind, p(data), p(expected), p(s2), p(response), J * B, None,
                                                        None, None, None, 0, n_params, max_iter, T, Kn, B, p(out), None,
                                                        None, p(pair), p(st), None)

    def reduced(n_params=J, data=d, b=best, a=arg, at_=at, eb_=eb, ea_=ea, ts=tst, st=status, k0=0):
        return lib.pisa_hip_profiled_metric_matrix_best_wide(0, p(data), p(e), p(s2), p(r), J * B, None, None, None, None,
                                                             0, None, k0, n_params, 32, T, Kn, B, p(b), p(a), p(at_),
                                                             p(eb_), p(ea_), p(ts), p(st), None)

    for rc in (full(n_params=0), full(n_params=33), full(data=None), full(expected=None), full(response=None),
               full(out=None), full(pair=None), full(st=None), full(max_iter=-1), full(max_iter=4097), full(kind=9),
               reduced(n_params=0), reduced(n_params=33), reduced(data=None), reduced(b=None), reduced(a=None),
               reduced(at_=None), reduced(eb_=None), reduced(ea_=None), reduced(ts=None), reduced(st=None),
               reduced(k0=Kn), reduced(k0=-1)):
        assert rc == -1
    torch.cuda.synchronize()
    assert (value == poison).all() and (pst == -7).all() and (best == poison).all() and (arg == -7).all()
    assert (eb == poison).all() and (ea == poison).all() and not status.any()
    assert full() == 0 and reduced() == 0
    torch.cuda.synchronize()
    assert not (value == poison).any() and not pst.any() and not (best == poison).any()
    # the Python wrappers refuse 0 and 33 parameters by name, the narrow ones 9
    for n in (0, 33):
        with pytest.raises(ValueError, match="1 to 32"):
            K.profiled_metric_matrix_wide("llh", d, e, torch.zeros((Kn, n, B), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="1 to 8"):
        K.profiled_metric_matrix("llh", d, e, r)
    with pytest.raises(ValueError):
        bad = f["D"].copy()
        bad[1, 2] = -1.0
        _run(K, "llh", dict(f, D=bad))
    # junk in one pair stays there
    clean = _run(K, "llh", f)
    D = f["D"].copy()
    D[1, 5] = np.nan
    got = _run(K, "llh", dict(f, D=D))
    want = pc.restated("llh", D, f["E"], f["R"], f["S2"], f["ips"], f["c"])
    for key in FULL_KEYS:
        assert np.array_equal(got[key][[0, 2]], clean[key][[0, 2]]), key
    assert np.array_equal(got["eta"], want["eta"]) and np.array_equal(got["status"], want["status"])
    assert np.all(np.isfinite(got["value"])) and not np.array_equal(got["value"][1], clean["value"][1])
    lower, upper = np.tile(-np.ones(J), (Kn, 1)), np.tile(np.ones(J), (Kn, 1))
    boxed = _run(K, "llh", f, lower, upper)
    lower[1, 3] = 2.0
    got = _run(K, "llh", f, lower, upper)
    assert np.all(got["status"][:, 1] == bc.BAD_BOUNDS) and not got["eta"][:, 1].any() and not got["n_iter"][:, 1].any()
    for key in FULL_KEYS:
        assert np.array_equal(got[key][:, 0], boxed[key][:, 0]), key
    E = f["E"].copy()
    E[0, 7] = 1e-11
    got = _run(K, "llh", dict(f, E=E))
    assert np.all(got["status"][:, 0] == pc.START_OUTSIDE) and not got["eta"][:, 0].any()
    for key in FULL_KEYS:
        assert np.array_equal(got[key][:, 1], clean[key][:, 1]), key


# ------------------------------------------------------------------------------- 7. end to end on the device
@pytest.mark.parametrize("metric", ("llh", "chi2"))
def test_drivers_with_a_12_parameter_response_on_the_device(K, metric):
    from pisa_amd.analysis import ensemble as en
    from tests import test_host_profiled_wide as hw

    grid, resp, other = hw.toy(metric, 12)
    dev, ref = en.DeviceSolver(), hw._WideSolver()
    data = en.pseudo_data(grid, 4, 10, 3)
    s2 = grid.sigma2_for(metric)
    group = "llh" if metric in pc.LLH_KINDS else metric
    ex = pc.solve(group, data, grid.hist, resp.response, s2, resp.inv_prior_sigma, resp.center, max_iter=200,
                  dtype=np.longdouble, stop=1e-30)
    assert not ex["status"].any()
    val, scale = pc.exact_value(metric, data, grid.hist, resp.response, s2, ex["eta"], resp.inv_prior_sigma, resp.center)
    m = en.metric_matrix(data, grid, metric, False, dev, resp).cpu().numpy()
    r = ec.check(m, val, scale, wc.g_of(metric), "toy %s" % metric)
    print("toy grid, 12 parameters, %s: worst %.3f eps S (gate %.3g)" % (metric, r, wc.g_of(metric)))
    tol = 2 * (wc.g_of(metric) + pc.G_HOST) * pc.EPS * scale.max()
    for k0 in (0, 4):
        got, gi = en.delta_metric(data, grid, metric, k0, dev, resp, return_info=True)
        want, wi = en.delta_metric(data, grid, metric, k0, ref, resp, return_info=True)
        assert np.array_equal(gi["arg"], wi["arg"]) and gi["flagged"] == wi["flagged"] == 0
        assert np.all(np.abs(got - want) <= tol) and np.all(got >= 0)
        assert np.all(np.abs(gi["eta_at"] - wi["eta_at"]) <= 1e-9 * (1.0 + np.abs(wi["eta_at"])))
    crit = np.full(len(grid), float(np.median(want)))
    observed = hw.observed_map(grid)
    assert np.array_equal(en.accepted(observed, grid, metric, crit, dev, resp),
                          en.accepted(observed, grid, metric, crit, ref, resp))
    if metric == "llh":
        for nuisance in ("fixed", "profiled"):
            want, wi = hw.host_fc(nuisance)
            got, gi = en.feldman_cousins(grid, metric, hw.FC_TRIALS, random_state=hw.FC_SEED, true_points=hw.FC_POINTS,
                                         solver=dev, response=resp, nuisance=nuisance,
                                         observed=observed if nuisance == "profiled" else None)
            assert np.all(np.abs(got - want) <= tol) and np.array_equal(gi["flagged"], wi["flagged"])
    # what stays limited to 8 parameters is refused before any launch, by name
    with pytest.raises(ValueError, match="limited to 8 nuisance parameters"):
        en.delta_metric(data, grid, metric, 4, dev, resp, return_info=True, covariance=True)
