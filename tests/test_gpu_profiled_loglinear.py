"""The log-linear response of the profiled trial ensembles on the device (csrc/profile_loglinear.hip:
`pisa_hip_profiled_metric_matrix_wide_form`, `pisa_hip_profiled_metric_matrix_best_wide_form` through
`kernels.profiled_metric_matrix_wide(..., form=)` / `profiled_metric_matrix_best_wide(..., form=)`) and the `form=`
paths of pisa_amd/analysis/ensemble.py with `DeviceSolver`.

With the form linear every output `==` that of the `_wide` entry points.  With the form log-linear the comparison is
against the numpy restatement and the longdouble reference of tests/profile_loglinear_cases.py: the value inside the
gate |got - exact| <= G eps S with G from G_REF_L / G_REF_LB (measured on the CPU), status 0, at most one Newton step
more than the restatement's most (a stop decision may move with the last bit of the device's exp), eta within 1e-9 (1 +
|eta|) of the restatement's, the coordinates on a bound the restatement's and equal to the bound.  `pytest -s` prints
the kernels' own worst ratios before each assertion.
"""
import ctypes

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc
from tests import profile_loglinear_cases as lc

pytestmark = pytest.mark.gpu

FULL_KEYS = ("value", "eta", "n_iter", "status")
BEST_KEYS = ("best", "arg", "at", "eta_best", "eta_at", "status")


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


def _run(K, kind, f, lower=None, upper=None, max_iter=lc.MAX_ITER, form="loglinear", **kw):
    return _host(K.profiled_metric_matrix_wide(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]),
                                               _dev(K, f["S2"]), _dev(K, f["ips"]), _dev(K, f["c"]), max_iter=max_iter,
                                               lower=_dev(K, lower), upper=_dev(K, upper), form=form, **kw))


def _best(K, kind, f, lower=None, upper=None, offset=None, k0=0, max_iter=lc.MAX_ITER, form="loglinear"):
    return _host(K.profiled_metric_matrix_best_wide(kind, _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]),
                                                    _dev(K, f["S2"]), _dev(K, f["ips"]), _dev(K, f["c"]),
                                                    _dev(K, offset), k0, max_iter=max_iter, lower=_dev(K, lower),
                                                    upper=_dev(K, upper), form=form))


def _same(got, want, keys, what):
    for key in keys:
        assert np.array_equal(got[key], want[key], equal_nan=True), (what, key)


# ------------------------------------------------------------------------- 1. form = LINEAR is the _wide call
class _Raw:
    """the four entry points called through ctypes on one case: every output tensor poisoned before the call"""

    def __init__(self, K, kind, f, lower, upper, offset, k0):
        import torch

        from pisa_amd import _lib

        self.lib, self.torch = _lib.lib(), torch
        self.kind = pc.KINDS.index(kind)
        self.T, self.B = f["D"].shape
        self.Kn, self.J = f["E"].shape[0], f["R"].shape[-2]
        self.k0 = k0
        self.dev = K.device()
        self.inputs = [_dev(K, a) for a in (f["D"], f["E"], f["S2"], f["R"], f["ips"], f["c"], lower, upper, offset)]

    @staticmethod
    def p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def _head(self, form):
        d, e, s2, r, ips, c, lo, hi, _ = self.inputs
        head = [self.kind] + ([] if form is None else [form])
        return head + [self.p(d), self.p(e), self.p(s2), self.p(r), self.J * self.B if r.dim() == 3 else 0, self.p(ips),
                       self.p(c), self.p(lo), self.p(hi), 0]

    def full(self, form):
        """form None: `_wide`; else `_wide_form` -> (return code, outputs)"""
        torch, T, Kn, J = self.torch, self.T, self.Kn, self.J
        value = torch.full((T, Kn), 12345.0, dtype=torch.float64, device=self.dev)
        eta = torch.full((T, Kn, J), 12345.0, dtype=torch.float64, device=self.dev)
        n_iter, pst = (torch.full((T, Kn), -7, dtype=torch.int32, device=self.dev) for _ in range(2))
        status = torch.zeros(2, dtype=torch.int32, device=self.dev)
        fn = self.lib.pisa_hip_profiled_metric_matrix_wide if form is None else (
            self.lib.pisa_hip_profiled_metric_matrix_wide_form)
        rc = fn(*self._head(form), J, lc.MAX_ITER, T, Kn, self.B, self.p(value), self.p(eta), self.p(n_iter),
                self.p(pst), self.p(status), None)
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in dict(value=value, eta=eta, n_iter=n_iter, status=pst,
                                                        word=status).items()}

    def best(self, form):
        torch, T, J = self.torch, self.T, self.J
        best, at = (torch.full((T,), 12345.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        eb, ea = (torch.full((T, J), 12345.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        arg, tst = (torch.full((T,), -7, dtype=torch.int32, device=self.dev) for _ in range(2))
        status = torch.zeros(2, dtype=torch.int32, device=self.dev)
        fn = self.lib.pisa_hip_profiled_metric_matrix_best_wide if form is None else (
            self.lib.pisa_hip_profiled_metric_matrix_best_wide_form)
        rc = fn(*self._head(form), self.p(self.inputs[8]), self.k0, J, lc.MAX_ITER, T, self.Kn, self.B, self.p(best),
                self.p(arg), self.p(at), self.p(eb), self.p(ea), self.p(tst), self.p(status), None)
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in dict(best=best, arg=arg, at=at, eta_best=eb, eta_at=ea, status=tst,
                                                        word=status).items()}


@pytest.mark.parametrize("kind", pc.KINDS)
def test_form_linear_is_the_wide_entry_point_bit_for_bit(K, kind):
    for shape in ((2, 2, 65, 9), (1, 2, 130, 32)):
        f = pc.family("poisson", *shape)
        Kn, J = shape[1], shape[3]
        offset = np.random.RandomState(4).randn(Kn)
        for lower, upper in ((None, None), bc.box("wide", Kn, J)):
            raw = _Raw(K, kind, f, lower, upper, offset, Kn - 1)
            for call, keys in ((raw.full, FULL_KEYS), (raw.best, BEST_KEYS)):
                rc_w, want = call(None)
                rc_f, got = call(lc.LINEAR)
                assert rc_w == rc_f == 0 and not want["word"].any()
                _same(got, want, keys + ("word",), (kind, shape, lower is not None))
                assert not (want[keys[0]] == 12345.0).any()
            # any other value than the two forms: refused before any device access, nothing written
            for form in (2, -1):
                for call, keys in ((raw.full, FULL_KEYS), (raw.best, BEST_KEYS)):
                    rc, got = call(form)
                    assert rc == -1 and (got[keys[0]] == 12345.0).all() and (got["status"] == -7).all()
                    assert not got["word"].any()


# --------------------------------------------------------------------------------------------- 2. the gate
@pytest.mark.parametrize("kind", lc.KINDS)
def test_every_entry_within_the_gate_of_the_exact_value(K, kind):
    worst, where, steps = 0.0, None, 0
    for fam, shape in lc.gated_cases():
        f = lc.family(fam, *shape)
        ex, want = lc.exact(fam, kind, shape), lc.restated_case(fam, kind, shape)
        got = _run(K, kind, f)
        what = "%s %s %s" % (fam, kind, shape)
        assert not got["status"].any(), (what, np.unique(got["status"]))
        assert np.all(got["n_iter"] <= lc.MOST_STEPS_L + 1), (what, got["n_iter"].max())
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, (fam, shape)
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], lc.g_of(kind), what)
        assert np.all(np.abs(got["eta"] - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"]))), what
    print("log-linear %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps"
          % (kind, worst, where, lc.g_of(kind), steps))


@pytest.mark.parametrize("kind", lc.KINDS)
def test_every_bounded_entry_within_the_gate_of_the_exact_value(K, kind):
    worst, where, steps = 0.0, None, 0
    for fam, bx, shape in lc.gated_bounded_cases():
        f = lc.family(fam, *shape)
        lower, upper = bc.box(bx, shape[1], shape[3])
        ex, want = lc.exact(fam, kind, shape, bx), lc.restated_case(fam, kind, shape, bx)
        got = _run(K, kind, f, lower, upper)
        what = "%s %s %s %s" % (fam, bx, kind, shape)
        assert not got["status"].any(), (what, np.unique(got["status"]))
        assert np.all(got["n_iter"] <= lc.MOST_STEPS_L + 1), (what, got["n_iter"].max())
        on = bc.on_bound(got["eta"], lower, upper)
        assert np.array_equal(on, bc.on_bound(want["eta"], lower, upper)), what
        assert np.array_equal(got["eta"][on != 0], want["eta"][on != 0]), what
        r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
        if r > worst:
            worst, where = r, (fam, bx, shape)
        steps = max(steps, int(got["n_iter"].max()))
        ec.check(got["value"], ex["value"], ex["scale"], lc.g_of(kind, True), what)
        assert np.all(np.abs(got["eta"] - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"]))), what
    print("log-linear bounded %s: worst %.3f eps S at %s (gate %.3g), at most %d Newton steps"
          % (kind, worst, where, lc.g_of(kind, True), steps))


# ------------------------------------------------------------------------------------------ 3. closed forms
@pytest.mark.parametrize("kind", lc.KINDS)
def test_closed_forms(K, kind):
    for shape in lc.ONE_PARAMETER_SHAPES:
        T, Kn = shape[:2]
        rows, own = np.arange(T), np.arange(T) % Kn
        for fam, want in (("far", np.log(3.0)), ("low", -np.log(4.0))):
            eta = _run(K, kind, lc.family(fam, *shape))["eta"]
            assert np.all(np.abs(eta[rows, own, 0] - want) <= 1e-9 * (1.0 + abs(want))), (fam, kind, shape)
        if kind in lc.LLH_KINDS:
            f = lc.family("norm", *shape)
            want = np.log(f["D"].sum(axis=1)[:, None] / f["E"].sum(axis=1)[None, :])
            eta = _run(K, kind, f)["eta"][:, :, 0]
            assert np.all(np.abs(eta - want) <= 1e-9 * (1.0 + np.abs(want))), (kind, shape)


# ------------------------------------------------------------------------------------- 4. the reduced output
@pytest.mark.parametrize("kind", lc.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_one(K, kind):
    # (2, 300, 12, 12): two trials, so the 300 templates are split over workgroups and joined by a second launch
    for fam, shape in (("poisson", (2, 300, 12, 12)), ("shared", (8, 30, 12, 12)), ("prior", (2, 2, 64, 17)),
                       ("poisson", (1, 1, 1, 9)), ("far", (65, 1, 3, 1))):
        f = lc.family(fam, *shape)
        Kn, J = shape[1], shape[3]
        for lower, upper in ((None, None), bc.own_rows_box(Kn, J)):
            full = _run(K, kind, f, lower, upper)
            rs = np.random.RandomState(3)
            for offset, k0 in ((None, 0), (rs.randn(Kn), Kn - 1), (rs.randn(Kn), Kn // 2)):
                want = pc.reduce_profiled(kind, full, offset, k0)
                got = _best(K, kind, f, lower, upper, offset, k0)
                _same(got, want, BEST_KEYS, (fam, shape, kind, k0, lower is not None))
    assert _run(K, kind, lc.family("poisson", 1, 1, 1, 9), want_eta=False)["eta"] is None


# --------------------------------------------------------------------------------------- 5. status families
def test_status_families_carry_the_restatements_flags(K):
    for name in lc.STATUS_FAMILIES:
        f = lc.status_family(name)
        for kind in (lc.KINDS if name == "overflow" else (f["kind"],)):
            want = lc.restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
            got = _run(K, kind, f, max_iter=f["max_iter"])
            assert np.array_equal(got["status"], want["status"]), (name, kind)
            for key in FULL_KEYS:
                assert np.all(np.isfinite(got[key])), (name, kind, key)
            if name == "overflow":
                assert not got["status"].any() and np.all(got["n_iter"] <= want["n_iter"] + 1)
                assert np.all(np.abs(got["eta"] - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"])))
                val, scale = lc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], got["eta"].astype(np.longdouble),
                                            None, None)
                ec.check(got["value"], val, scale, lc.g_of(kind), name)
                red = _best(K, kind, f, k0=0)
                _same(red, pc.reduce_profiled(kind, got, None, 0), BEST_KEYS, (name, kind))
            else:
                assert got["status"].any(), name
                assert np.all(np.abs(got["n_iter"] - want["n_iter"]) <= (got["status"] == 0)), name
    start = lc.status_family("start")
    got = _run(K, start["kind"], start)
    assert np.all(got["status"][:, 1] == pc.START_OUTSIDE) and not got["eta"][:, 1].any()
    assert not got["status"][:, [0, 2]].any()


def test_bad_data_and_unknown_forms(K):
    import torch

    shape = (2, 2, 65, 9)
    f = lc.family("poisson", *shape)
    clean = _run(K, "llh", f)
    # a negative datum: PISA_HIP_ERR_NEGATIVE
    bad = f["D"].copy()
    bad[1, 2] = -1.0
    with pytest.raises(ValueError):
        _run(K, "llh", dict(f, D=bad))
    # a NaN datum: its bin is skipped in its trial, the other trial does not change
    D = f["D"].copy()
    D[1, 5] = np.nan
    got = _run(K, "llh", dict(f, D=D))
    want = lc.restated("llh", D, f["E"], f["R"], f["S2"], f["ips"], f["c"])
    for key in FULL_KEYS:
        assert np.array_equal(got[key][0], clean[key][0]), key
        assert np.all(np.isfinite(got[key])), key
    assert not got["status"].any() and np.array_equal(got["status"], want["status"])
    assert np.all(np.abs(got["eta"] - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"])))
    assert not np.array_equal(got["value"][1], clean["value"][1])
    kept = np.ones(shape[2], dtype=bool)
    kept[5] = False
    sub = dict(f, D=f["D"][1:, kept], E=f["E"][:, kept], S2=f["S2"][:, kept], R=f["R"][:, :, kept])
    val, scale = lc.exact_value("llh", sub["D"], sub["E"], sub["R"], sub["S2"], got["eta"][1:].astype(np.longdouble),
                                f["ips"], f["c"])
    ec.check(got["value"][1:], val, scale, lc.g_of("llh"), "NaN datum")
    # a bin with E = 0, or without any rho, does not respond: it is a constant, whatever its rho or E
    E = f["E"].copy()
    E[:, 7] = 0.0
    R = f["R"].copy()
    R[:, :, 11] = 0.0
    got = _run(K, "poisson_llh", dict(f, E=E, R=R))
    want = lc.restated("poisson_llh", f["D"], E, R, f["S2"], f["ips"], f["c"])
    assert not got["status"].any() and not want["status"].any()
    assert np.all(np.abs(got["eta"] - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"])))
    val, scale = lc.exact_value("poisson_llh", f["D"], E, R, f["S2"], got["eta"].astype(np.longdouble), f["ips"],
                                f["c"])
    ec.check(got["value"], val, scale, lc.g_of("poisson_llh"), "bins that do not respond")
    # an unknown form raises before any launch, and names the two choices
    for fn in (lambda form: _run(K, "llh", f, form=form), lambda form: _best(K, "llh", f, form=form)):
        with pytest.raises(ValueError, match="'linear', 'loglinear'"):
            fn("exponential")
    with pytest.raises(ValueError, match="1 to 32"):
        K.profiled_metric_matrix_wide("llh", _dev(K, f["D"]), _dev(K, f["E"]),
                                      torch.zeros((2, 33, 65), dtype=torch.float64, device=K.device()),
                                      form="loglinear")
    # bad bounds are flagged as in the linear form
    lower, upper = np.tile(-np.ones(9), (2, 1)), np.tile(np.ones(9), (2, 1))
    lower[1, 3] = 2.0
    got = _run(K, "llh", f, lower, upper)
    assert np.all(got["status"][:, 1] == bc.BAD_BOUNDS) and not got["eta"][:, 1].any() and not got["n_iter"][:, 1].any()
    assert not got["status"][:, 0].any()


# ------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("kind", lc.KINDS[::3])
def test_two_launches_are_equal(K, kind):
    for fam, shape in (("poisson", (1, 2, 130, 32)), ("poisson", (2, 300, 12, 12))):
        f = lc.family(fam, *shape)
        _same(_run(K, kind, f), _run(K, kind, f), FULL_KEYS, (fam, shape))
        offset = np.random.RandomState(1).randn(shape[1])
        _same(_best(K, kind, f, None, None, offset, 1), _best(K, kind, f, None, None, offset, 1), BEST_KEYS,
              (fam, shape))


# ------------------------------------------------------------------------------- 7. end to end on the device
@pytest.mark.parametrize("metric", ("llh", "chi2"))
def test_drivers_with_12_loglinear_parameters_on_the_device(K, metric):
    from pisa_amd.analysis import ensemble as en
    from tests import test_host_profiled_loglinear as hl

    grid, resp, other = lc.toy(metric, 12)
    dev, ref = en.DeviceSolver(), hl._FormSolver()
    data = en.pseudo_data(grid, 4, 10, 3)
    s2 = grid.sigma2_for(metric)
    rho = np.asarray(resp.response)
    group = "llh" if metric in lc.LLH_KINDS else metric
    ex = lc.solve(group, data, grid.hist, rho, s2, resp.inv_prior_sigma, resp.center, max_iter=200,
                  dtype=np.longdouble, stop=1e-30)
    assert not ex["status"].any()
    val, scale = lc.exact_value(metric, data, np.asarray(grid.hist), rho, s2, ex["eta"], resp.inv_prior_sigma,
                                resp.center)
    m = en.metric_matrix(data, grid, metric, False, dev, resp).cpu().numpy()
    r = ec.check(m, val, scale, lc.g_of(metric), "toy %s" % metric)
    print("toy grid, 12 log-linear parameters, %s: worst %.3f eps S (gate %.3g)" % (metric, r, lc.g_of(metric)))
    tol = 2 * (lc.g_of(metric) + pc.G_HOST) * pc.EPS * scale.max()
    for k0 in (0, 4):
        got, gi = en.delta_metric(data, grid, metric, k0, dev, resp, return_info=True)
        want, wi = en.delta_metric(data, grid, metric, k0, ref, resp, return_info=True)
        assert np.array_equal(gi["arg"], wi["arg"]) and gi["flagged"] == wi["flagged"] == 0
        assert np.all(np.abs(got - want) <= tol) and np.all(got >= 0)
        assert np.all(np.abs(gi["eta_at"] - wi["eta_at"]) <= 1e-9 * (1.0 + np.abs(wi["eta_at"])))
    crit = np.full(len(grid), float(np.median(want)))
    observed = hl.observed_map(grid)
    assert np.array_equal(en.accepted(observed, grid, metric, crit, dev, resp),
                          en.accepted(observed, grid, metric, crit, ref, resp))
    if metric == "llh":
        for nuisance in ("fixed", "profiled"):
            want, wi = hl.host_fc(nuisance)
            got, gi = en.feldman_cousins(grid, metric, hl.FC_TRIALS, random_state=hl.FC_SEED, true_points=hl.FC_POINTS,
                                         solver=dev, response=resp, nuisance=nuisance,
                                         observed=observed if nuisance == "profiled" else None)
            assert np.all(np.abs(got - want) <= tol) and np.array_equal(gi["flagged"], wi["flagged"])
    # what reads a linear kernel is refused before any launch, by name
    with pytest.raises(ValueError, match="log-linear"):
        en.delta_metric(data, grid, metric, 4, dev, resp, return_info=True, covariance=True)
