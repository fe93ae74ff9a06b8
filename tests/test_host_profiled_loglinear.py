"""The log-linear response of the profiled trial ensembles without a GPU: the constants of its gate measured again
(tests/profile_loglinear_cases.py), the wide solver's own source (csrc/profile_wide_device.hpp) compiled for the host
under the sanitizers and run lane by lane in both forms, and the `form=` paths of pisa_amd/analysis/ensemble.py with a
numpy solver.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_bounded_cases as pbc
from tests import profile_cases as pc
from tests import profile_loglinear_cases as lc
from tests import profile_wide_cases as wc

_WORST = {}


def _worst(bounded):
    """(worst ratio per kind, most Newton steps) of the restatement over the gated cases; every pair of every case has
    status 0 in the exact reference and in the restatement (bounded: and the same coordinates on a bound), so no pair
    is left out of a gated comparison"""
    if bounded not in _WORST:
        worst, steps = {k: 0.0 for k in lc.KINDS}, 0
        cases = lc.gated_bounded_cases() if bounded else [(fam, None, shape) for fam, shape in lc.gated_cases()]
        for fam, bx, shape in cases:
            for kind in lc.KINDS:
                what = "%s %s %s %s" % (fam, bx, shape, kind)
                ex = lc.exact(fam, kind, shape, bx)
                got = lc.restated_case(fam, kind, shape, bx)
                assert not ex["status"].any(), (what, np.unique(ex["status"]))
                assert not got["status"].any(), (what, np.unique(got["status"]))
                if bounded:
                    lower, upper = pbc.box(bx, shape[1], shape[3])
                    assert np.array_equal(pbc.on_bound(got["eta"], lower, upper),
                                          pbc.on_bound(ex["eta"], lower, upper)), what
                worst[kind] = max(worst[kind], ec.check(got["value"], ex["value"], ex["scale"], pc.G_HOST, what))
                steps = max(steps, int(got["n_iter"].max()))
        _WORST[bounded] = (worst, steps)
    return _WORST[bounded]


def test_the_recorded_constants_are_the_measured_ones():
    most = 0
    for bounded in (False, True):
        worst, steps = _worst(bounded)
        recorded = lc.G_REF_LB if bounded else lc.G_REF_L
        print("bounded %s: measured %s, recorded %s, at most %d Newton steps" % (bounded, worst, recorded, steps))
        assert set(recorded) == set(lc.KINDS)
        for kind in lc.KINDS:
            assert worst[kind] <= recorded[kind] <= worst[kind] + 0.02, (bounded, kind, worst[kind])
            assert lc.g_of(kind, bounded) == pc.mc.KERNEL_FACTOR * max(1.0, recorded[kind])
        most = max(most, steps)
    assert most == lc.MOST_STEPS_L <= lc.MAX_ITER // 2


def test_the_shapes_and_families_of_the_issue_are_all_there():
    assert set(lc.SHAPES) == {(1, 1, 1, 1), (1, 1, 1, 9), (2, 3, 63, 4), (2, 3, 64, 5), (2, 2, 65, 9), (1, 2, 130, 16),
                              (2, 2, 64, 17), (1, 2, 130, 31), (1, 2, 130, 32), (2, 2, 20, 32), (8, 30, 12, 12),
                              (2, 300, 12, 12)}
    assert set(lc.ONE_PARAMETER_SHAPES) == {(3, 2, 3, 1), (65, 1, 3, 1), (2, 3, 130, 1)}
    assert set(lc.BOUNDED_SHAPES) == {(2, 3, 64, 5), (1, 2, 130, 32), (3, 2, 3, 1)}
    cases = lc.gated_cases()
    for shape in lc.SHAPES:                  # every shape is fitted by the two families that have priors everywhere
        assert ("poisson", shape) in cases and ("shared", shape) in cases
    for fam in lc.ONE_PARAMETER:
        assert [s for f, s in cases if f == fam] == list(lc.ONE_PARAMETER_SHAPES)
    assert {f for f, _ in cases} == set(lc.GATED) == {"poisson", "shared", "asimov", "prior", "norm", "far", "low"}
    bounded = lc.gated_bounded_cases()
    assert {bx for _, bx, _ in bounded} == set(pbc.BOXES) and {s for _, _, s in bounded} == set(lc.BOUNDED_SHAPES)
    f = lc.family("poisson", 2, 3, 63, 4)
    assert np.array_equal(f["R"], 0.1 * pc._cosines(3, 4, 63)) and np.array_equal(f["ips"], np.ones(4))
    assert lc.family("shared", 2, 3, 63, 4)["R"].ndim == 2
    a = lc.family("asimov", 2, 3, 63, 4)
    mu = lc.mu_of(a["E"], a["R"], np.broadcast_to(a["eta0"][:, None, :], (2, 3, 4)))[0]
    assert a["ips"] is None and np.array_equal(a["D"], mu[np.arange(2), np.arange(2) % 3])
    for fam, factor in (("far", 3.0), ("low", 0.25)):
        f = lc.family(fam, 3, 2, 3, 1)
        assert np.array_equal(f["D"], factor * f["E"][np.arange(3) % 2]) and np.all(f["R"] == 1.0)


@pytest.mark.parametrize("kind", lc.KINDS)
def test_closed_forms_of_the_restatement(kind):
    for fam, want in (("far", np.log(3.0)), ("low", -np.log(4.0))):
        for shape in lc.ONE_PARAMETER_SHAPES:
            T, K = shape[:2]
            eta = lc.restated_case(fam, kind, shape)["eta"]
            own = eta[np.arange(T), np.arange(T) % K, 0]
            assert np.all(np.abs(own - want) <= 1e-12), (fam, kind, shape)
    if kind in lc.LLH_KINDS:
        for shape in lc.ONE_PARAMETER_SHAPES:
            f = lc.family("norm", *shape)
            want = np.log(f["D"].sum(axis=1)[:, None] / f["E"].sum(axis=1)[None, :])
            assert np.all(np.abs(lc.restated_case("norm", kind, shape)["eta"][:, :, 0] - want) <= 1e-12)


def test_status_families_of_the_restatement():
    out = {}
    for name in lc.STATUS_FAMILIES:
        f = lc.status_family(name)
        out[name] = lc.restated(f["kind"], f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
    assert np.all(out["start"]["status"][:, 1] == pc.START_OUTSIDE) and not out["start"]["status"][:, [0, 2]].any()
    assert not out["start"]["eta"][:, 1].any()
    assert np.all(out["posdef"]["status"] == pc.NOT_POSDEF)
    assert np.all(out["maxiter"]["status"] == pc.NOT_CONVERGED) and np.all(out["maxiter"]["n_iter"] == 1)
    f = lc.status_family("overflow")
    for kind in lc.KINDS:
        o = lc.restated(kind, f["D"], f["E"], f["R"], f["S2"], None, None)
        assert not o["status"].any() and np.all(np.isfinite(o["value"])) and np.all(np.isfinite(o["eta"]))
        assert o["n_iter"].max() == (6 if kind in lc.LLH_KINDS else 12), (kind, o["n_iter"])
        # the llh kinds' first full step, about 5000, leaves exp's range: taken whole it would be a NaN
        if kind in lc.LLH_KINDS:
            with lc._state_machine():
                _, _, _, _, g, H = pc._sweep(kind, f["D"], f["E"], f["S2"], f["R"], np.zeros((2, 1, 1)))
            assert np.all(np.abs(g[:, :, 0] / H[(0, 0)]) > 1000.0)
        assert np.all(np.abs(o["eta"][:, 0, 0]) > 8.0) and o["eta"][0, 0, 0] > 0 > o["eta"][1, 0, 0]


# ------------------------------------------------------------- the kernel's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through the phases of profile_wide_device.hpp as the kernel strings them together,
// with a loop over the lanes where the kernel has its wavefront: nine int64 (kind, T, K, B, J, shared response,
// max_iter, bounded, form), then D [T][B], E and S2 [K][B], R [K or 1][J][B], ips [J], c [K][J], lo and hi [K][J]; per
// case value [T][K], eta [T][K][J], then n_iter and status as doubles.  Every pair is run twice, the lanes of a phase
// in ascending and in descending order: a phase in which a lane reads what another lane writes would differ.
#include "profile_wide_device.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace pisa;
struct Case {
    int64_t kind, T, K, B, J, shared, max_iter, bounded, form;
    std::vector<double> D, E, S2, R, ips, c, lo, hi;
};
template <bool UP>
struct HostLanes {
    template <class F>
    void each(F f) {
        if (UP)
            for (int l = 0; l < PFW_LANES; l++) f(l);
        else
            for (int l = PFW_LANES - 1; l >= 0; l--) f(l);
    }
};
struct Pair {
    double value;
    std::vector<double> eta;
    int32_t n_iter, status;
};
static void stage(const Case &q, PfwShared &S, double *R, int64_t t, int64_t k, int64_t c0, int lane) {
    const int64_t b = c0 + lane;
    const bool in = b < q.B;
    const int J = (int)q.J;
    S.cD[lane] = in ? q.D[t * q.B + b] : 0.0;
    S.cE[lane] = in ? q.E[k * q.B + b] : 0.0;
    S.cS2[lane] = in ? q.S2[k * q.B + b] : 0.0;
    const double *r = &q.R[q.shared ? 0 : k * J * q.B];
    for (int j = 0; j < J; j++) R[j * PFW_LD + lane] = in ? r[j * q.B + b] : 0.0;
}
template <int KIND, int FORM, class X>
static Pair run_pair(const Case &q, int64_t t, int64_t k) {
    const int J = (int)q.J;
    // the state and the response chunk behind it, sized as the kernel sizes its LDS: the sanitizer sees the end
    std::vector<double> mem(sizeof(PfwShared) / sizeof(double) + pfw_chunk_doubles(J));
    PfwShared &S = *reinterpret_cast<PfwShared *>(mem.data());
    double *R = mem.data() + sizeof(PfwShared) / sizeof(double);
    X x;
    for (int j = J; j < pfw_padded(J); j++)
        for (int l = 0; l < PFW_LANES; l++) R[j * PFW_LD + l] = 0.0;
    x.each([&](int l) {
        if (l >= J) return;
        S.ips[l] = q.ips[l];
        S.cen[l] = q.c[k * J + l];
        S.lo[l] = q.lo[k * J + l];
        S.hi[l] = q.hi[k * J + l];
    });
    pfw_init(S, x, J, q.bounded != 0, true);
    while (!S.done) {
        x.each([&](int l) { pfw_sweep_begin(S, l); });
        for (int64_t c0 = 0; c0 < q.B; c0 += PFW_CHUNK) {
            const int nb = (int)(q.B - c0 < PFW_CHUNK ? q.B - c0 : PFW_CHUNK);
            x.each([&](int l) { stage(q, S, R, t, k, c0, l); });
            x.each([&](int l) { pfw_bins<KIND, FORM>(S, R, l, nb); });
            x.each([&](int l) { pfw_chains(S, R, l, nb); });
        }
        pfw_decide<KIND>(S, x, (int32_t)q.max_iter);
    }
    x.each([&](int l) { pfw_value_begin(S, l); });
    for (int64_t c0 = 0; c0 < q.B; c0 += PFW_CHUNK) {
        const int nb = (int)(q.B - c0 < PFW_CHUNK ? q.B - c0 : PFW_CHUNK);
        x.each([&](int l) { stage(q, S, R, t, k, c0, l); });
        x.each([&](int l) { pfw_value_bins<KIND, FORM>(S, R, l, nb); });
        x.each([&](int l) { pfw_value_chain(S, l, nb); });
    }
    x.each([&](int l) { pfw_value_end<KIND>(S, l); });
    Pair p;
    p.value = S.value;
    p.eta.assign(S.eta, S.eta + J);
    p.n_iter = S.n_iter;
    p.status = pfw_status(S);
    return p;
}
static int n_order = 0;
template <int KIND, int FORM>
static void run(const Case &q, FILE *out) {
    const int J = (int)q.J;
    std::vector<double> value(q.T * q.K), eta(q.T * q.K * J), iters(q.T * q.K), status(q.T * q.K);
    for (int64_t t = 0; t < q.T; t++)
        for (int64_t k = 0; k < q.K; k++) {
            const Pair a = run_pair<KIND, FORM, HostLanes<true>>(q, t, k),
                       b = run_pair<KIND, FORM, HostLanes<false>>(q, t, k);
            if (memcmp(&a.value, &b.value, 8) || memcmp(a.eta.data(), b.eta.data(), 8 * J) || a.n_iter != b.n_iter ||
                a.status != b.status)
                n_order++;
            const int64_t o = t * q.K + k;
            value[o] = a.value;
            for (int j = 0; j < J; j++) eta[o * J + j] = a.eta[j];
            iters[o] = a.n_iter;
            status[o] = a.status;
        }
    fwrite(value.data(), 8, value.size(), out);
    fwrite(eta.data(), 8, eta.size(), out);
    fwrite(iters.data(), 8, iters.size(), out);
    fwrite(status.data(), 8, status.size(), out);
}
template <int FORM>
static void run_kind(const Case &q, FILE *out) {
    switch (q.kind) {
    case PF_LLH: run<PF_LLH, FORM>(q, out); break;
    case PF_POISSON_LLH: run<PF_POISSON_LLH, FORM>(q, out); break;
    case PF_CHI2: run<PF_CHI2, FORM>(q, out); break;
    default: run<PF_MOD_CHI2, FORM>(q, out);
    }
}
static bool take(FILE *in, std::vector<double> &v, int64_t n) {
    v.resize(n);
    return fread(v.data(), 8, n, in) == (size_t)n;
}
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t head[9];
    int n_cases = 0;
    while (fread(head, 8, 9, in) == 9) {
        Case q;
        q.kind = head[0], q.T = head[1], q.K = head[2], q.B = head[3], q.J = head[4], q.shared = head[5];
        q.max_iter = head[6], q.bounded = head[7], q.form = head[8];
        if (q.J < 1 || q.J > PFW_MAX_PARAMS) return 3;
        if (q.form != PFW_LINEAR && q.form != PFW_LOGLINEAR) return 3;
        if (!take(in, q.D, q.T * q.B) || !take(in, q.E, q.K * q.B) || !take(in, q.S2, q.K * q.B) ||
            !take(in, q.R, (q.shared ? 1 : q.K) * q.J * q.B) || !take(in, q.ips, q.J) || !take(in, q.c, q.K * q.J) ||
            !take(in, q.lo, q.K * q.J) || !take(in, q.hi, q.K * q.J))
            return 3;
        if (q.form == PFW_LINEAR)
            run_kind<PFW_LINEAR>(q, out);
        else
            run_kind<PFW_LOGLINEAR>(q, out);
        n_cases++;
    }
    fclose(out);
    printf("%d %d\n", n_cases, n_order);
    return 0;
}
"""

# the linear form's three shapes: unbounded below and above 8 parameters and under a box (tests/profile_wide_cases.py)
LINEAR_CASES = (("poisson", None, (3, 2, 40, 9)), ("prior", None, (2, 3, 63, 17)), ("poisson", "wide", (3, 2, 64, 16)))


def _cases():
    """(form, name, shape or None, box or None, f with kind / max_iter / lower / upper)"""
    cases = []
    for fam, bx, shape in LINEAR_CASES:
        f = pc.family(fam, *shape)
        lower, upper = (None, None) if bx is None else wc.bounds(bx, shape[1], shape[3])
        for kind in pc.KINDS:
            cases.append((lc.LINEAR, fam, shape, bx, dict(f, kind=kind, max_iter=wc.MAX_ITER, lower=lower, upper=upper)))
    for fam, shape in lc.gated_cases():
        f = lc.family(fam, *shape)
        for kind in lc.KINDS:
            cases.append((lc.LOGLINEAR, fam, shape, None, dict(f, kind=kind, max_iter=lc.MAX_ITER, lower=None,
                                                               upper=None)))
    for fam, bx, shape in lc.gated_bounded_cases():
        f = lc.family(fam, *shape)
        lower, upper = pbc.box(bx, shape[1], shape[3])
        for kind in lc.KINDS:
            cases.append((lc.LOGLINEAR, fam, shape, bx, dict(f, kind=kind, max_iter=lc.MAX_ITER, lower=lower,
                                                             upper=upper)))
    for name in lc.STATUS_FAMILIES:
        f = lc.status_family(name)
        for kind in (lc.KINDS if name == "overflow" else (f["kind"],)):
            cases.append((lc.LOGLINEAR, name, None, None, dict(f, kind=kind, lower=None, upper=None)))
    return cases


def test_the_wide_source_on_the_host_in_both_forms(tmp_path):
    """csrc/profile_wide_device.hpp compiled with g++ under ASan + UBSan and run as a program of its own, a loop over
    the lanes in the kernel's place.  The order of the lanes within a phase changes no bit, in either form.  Form
    linear: eta, n_iter and status `==` the existing restatements, and so is the value of the chi2 kinds; the value of
    the llh kinds, which the program forms with libm's log and lgamma where the restatement has numpy's and scipy's
    (they differ in the last bit: -194.36602941 against -194.3660294 on `poisson` (3, 2, 40, 9)), lies inside the
    wide form's gate around the exact reference, as in tests/test_host_profiled_wide.py.
    Form log-linear: every gated value inside the gate around the exact reference with status 0, at most one Newton
    step more than the restatement's most, eta
    within 1e-9 (1 + |eta|) of the restatement's and the same coordinates on a bound holding the bound's own doubles
    (libm's exp is not numpy's: no `==`); the status families carry the restatement's flags."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "profile_loglinear_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = _cases()
    with open(tmp_path / "cases.bin", "wb") as fh:
        for form, _, _, _, f in cases:
            T, B = f["D"].shape
            K = f["E"].shape[0]
            J = f["R"].shape[-2]
            bounded = f["lower"] is not None or f["upper"] is not None
            lo, hi = pbc.full_bounds(f["lower"], f["upper"], K, J)
            fh.write(np.array([pc.KINDS.index(f["kind"]), T, K, B, J, int(f["R"].ndim == 2), f["max_iter"],
                               int(bounded), form], dtype=np.int64).tobytes())
            for a in (f["D"], f["E"], f["S2"], f["R"], np.zeros(J) if f["ips"] is None else f["ips"],
                      np.zeros((K, J)) if f["c"] is None else f["c"], lo, hi):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.split() == [str(len(cases)), "0"], res.stdout
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    worst = {False: {k: 0.0 for k in lc.KINDS}, True: {k: 0.0 for k in lc.KINDS}}
    steps = 0
    for form, name, shape, bx, f in cases:
        T, K, J = f["D"].shape[0], f["E"].shape[0], f["R"].shape[-2]
        n = T * K
        value = got_all[at:at + n].reshape(T, K)
        eta = got_all[at + n:at + n + n * J].reshape(T, K, J)
        n_iter = got_all[at + n + n * J:at + 2 * n + n * J].reshape(T, K)
        status = got_all[at + 2 * n + n * J:at + 3 * n + n * J].reshape(T, K)
        at += 3 * n + n * J
        kind = f["kind"]
        bounded = f["lower"] is not None or f["upper"] is not None
        what = "%s %s %s %s %s" % (("linear", "loglinear")[form], name, shape, bx, kind)
        if form == lc.LINEAR:
            want = wc.restated(name, kind, shape, bx)
            for key, got in (("eta", eta), ("n_iter", n_iter), ("status", status)):
                assert np.array_equal(got, want[key]), (what, key)
            if kind in lc.LLH_KINDS:     # (the value of the llh kinds goes through libm's log and lgamma, not numpy's)
                ex = pbc.exact_bounded(name, bx, kind, *shape) if bounded else pc.exact(name, kind, *shape)
                ec.check(value, ex["value"], ex["scale"], wc.g_of(kind, bounded), what)
            else:
                assert np.array_equal(value, want["value"]), (what, "value")
            continue
        if shape is None:
            want = lc.restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
            assert np.array_equal(status, want["status"]), what
            assert np.all(np.isfinite(value)) and np.all(np.isfinite(eta)), what
            if name == "overflow":
                assert not status.any() and np.all(n_iter <= want["n_iter"] + 1), what
            continue
        ex, want = lc.exact(name, kind, shape, bx), lc.restated_case(name, kind, shape, bx)
        assert not status.any(), (what, np.unique(status))
        assert np.all(n_iter <= lc.MOST_STEPS_L + 1), (what, n_iter.max())
        steps = max(steps, int(n_iter.max()))
        assert np.all(np.abs(eta - want["eta"]) <= 1e-9 * (1.0 + np.abs(want["eta"]))), what
        if bounded:
            on = pbc.on_bound(eta, f["lower"], f["upper"])
            assert np.array_equal(on, pbc.on_bound(want["eta"], f["lower"], f["upper"])), what
            assert np.array_equal(eta[on != 0], want["eta"][on != 0]), what
        r = ec.check(value, ex["value"], ex["scale"], lc.g_of(kind, bounded), what)
        worst[bounded][kind] = max(worst[bounded][kind], r)
    assert at == got_all.size
    print("the log-linear form on the host: worst ratios %s, at most %d Newton steps" % (worst, steps))


# --------------------------------------------------------------------------- the ensemble's plumbing
class _FormSolver(lc.NumpyFormSolver):
    def hesse(self, *args, **kw):
        raise AssertionError("a refused call reached the solver")

    posterior = draw_linear = draw_linear_mvn = draw_linear_at = hesse

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        from tests import fluctuate_cases as fc

        return fc.block(mu, n_trials, seed, stream, first_trial)[0]


class _ToyMaker:
    """what `NuisanceResponse.from_maker` asks of a maker, with a template that is known in closed form:
    T_b(norm, tilt) = base_b norm (1 + tilt x_b), two bins of the base empty"""

    def __init__(self):
        from pisa_amd.core.param import Param, ParamSet

        self.params = ParamSet(Param("norm", 1.0, prior=None, range=[0.5, 1.5], is_fixed=False),
                               Param("tilt", 0.1, prior=None, range=[-0.5, 0.5], is_fixed=False))
        self._pipelines = []
        self.x = np.linspace(-1.0, 1.0, 10)
        self.base = 30.0 + 10.0 * np.cos(2.0 * self.x)
        self.base[[2, 7]] = 0.0

    def template(self):
        norm, tilt = (float(self.params[n].value.magnitude) for n in ("norm", "tilt"))
        return self.base * norm * (1.0 + tilt * self.x)

    def _set_rescaled_free_params(self, point):
        for p, u in zip(self.params.free, point):
            lo, hi = (r.magnitude for r in p.range)
            p.value = (lo + float(u) * (hi - lo)) * p.value.units

    def set_free_params(self, values):
        for p, v in zip(self.params.free, values):
            p.value = v

    def _fisher_templates(self, names, test_vals):
        (name,) = names
        lo, hi = test_vals[name]
        saved = self.params[name].value
        maps = []
        for v in (lo, hi):
            self.params[name].value = v
            maps.append(self.template())
        self.params[name].value = saved
        return {"grad": (maps[1] - maps[0]) / float((hi - lo).magnitude)}


def test_from_maker_divides_the_gradients_by_the_points_own_template(monkeypatch):
    from pisa_amd import kernels
    from pisa_amd.analysis import ensemble as en

    monkeypatch.setattr(kernels, "to_device", lambda a: a)       # (no device here: the response stays a host array)
    maker = _ToyMaker()
    points = np.array([[0.5, 0.6], [0.2, 0.3], [0.9, 0.5]])
    hist = []
    for pt in points:
        maker._set_rescaled_free_params(pt)
        hist.append(maker.template())
    maker._set_rescaled_free_params([0.5, 0.6])
    hist = np.array(hist)
    grid = en.TemplateGrid(hist, 0.3 * hist, points, None, np.zeros(3), "llh")
    tv = {"norm": (-0.05, 0.05), "tilt": (-0.02, 0.02)}
    lin = en.NuisanceResponse.from_maker(maker, grid, ["norm", "tilt"], tv)
    log = en.NuisanceResponse.from_maker(maker, grid, ["norm", "tilt"], tv, form="loglinear")
    assert lin.form == "linear" and not lin.wide and lin.fit_keywords() == {}
    assert log.form == "loglinear" and log.wide and log.fit_keywords() == {"wide": True, "form": "loglinear"}
    grad, rho = np.asarray(lin.response), np.asarray(log.response)
    has = hist > 0
    assert (~has).sum() == 6 and grad.shape == rho.shape == (3, 2, 10)
    for j in range(2):
        assert np.array_equal(rho[:, j][has], (grad[:, j] / np.where(has, hist, 1.0))[has])
        assert not rho[:, j][~has].any()
    # the logarithmic derivatives of the closed form: 1 / norm and x / (1 + tilt x)
    norm = 0.5 + points[:, 0]
    tilt = -0.5 + points[:, 1]
    assert np.allclose(rho[:, 0][has], np.broadcast_to(1.0 / norm[:, None], hist.shape)[has], rtol=1e-12)
    assert np.allclose(rho[:, 1][has], (maker.x[None] / (1.0 + tilt[:, None] * maker.x[None]))[has], rtol=1e-12)
    assert np.array_equal(log.values, lin.values) and float(maker.params["norm"].value.magnitude) == 1.0
    with pytest.raises(ValueError, match="'linear', 'loglinear'"):
        en.NuisanceResponse.from_maker(maker, grid, ["norm"], tv, form="exp")
    # 9 names are taken without wide=: a log-linear response is wide by definition
    with pytest.raises(ValueError, match="is not a free parameter"):
        en.NuisanceResponse.from_maker(maker, grid, ["norm"] + ["n%d" % j for j in range(8)], tv, form="loglinear")
    with pytest.raises(ValueError, match="1 to 32"):
        en.NuisanceResponse.from_maker(maker, grid, ["n%d" % j for j in range(33)], tv, form="loglinear")


def test_a_loglinear_response_is_wide_and_carries_its_form():
    from pisa_amd.analysis import ensemble as en

    for n in (1, 9, 32):
        r = en.NuisanceResponse(tuple("n%d" % j for j in range(n)), np.zeros((9, n, 24)), form="loglinear")
        assert r.wide and r.form == "loglinear" and r.fit_keywords() == {"wide": True, "form": "loglinear"}
    for n in (0, 33):
        with pytest.raises(ValueError, match="1 to 32"):
            en.NuisanceResponse(tuple("n%d" % j for j in range(n)), np.zeros((9, n, 24)), form="loglinear")
    with pytest.raises(ValueError, match="'linear', 'loglinear'"):
        en.NuisanceResponse(("a",), np.zeros((9, 1, 24)), form="exponential")
    boxed = en.NuisanceResponse(("a",), np.zeros((1, 24)), lower=[-1.0], upper=[1.0], form="loglinear", wide=False)
    assert boxed.wide and set(boxed.fit_keywords()) == {"lower", "upper", "wide", "form"}
    assert en.NuisanceResponse(("a",), np.zeros((1, 24))).fit_keywords() == {}
    assert en.NuisanceResponse(("a",), np.zeros((1, 24)), wide=True).fit_keywords() == {"wide": True}
    assert "32" in en.NuisanceResponse.__doc__ and "log-linear" in en.NuisanceResponse.__doc__.lower()


def test_the_host_generators_mean_is_the_forms_own():
    from pisa_amd.analysis import ensemble as en

    grid, resp, _ = lc.toy("llh", 12)
    hist = np.asarray(grid.hist)
    rs = np.random.RandomState(5)
    eta = 0.2 * rs.randn(12)
    rho = np.asarray(resp.response)[4]
    mu = en._loglinear_mean(hist[4], rho, eta)
    want = lc.mu_of(hist[4:5], rho[None], eta[None, None, :])[0][0, 0]
    assert np.array_equal(mu, want) and np.all(mu > 0)
    assert np.allclose(mu, hist[4] * np.exp(np.einsum("jb,j->b", rho, eta)), rtol=1e-14)
    # a bin that does not respond keeps its mean exactly; a NaN stays; an overflow is no NaN
    mu0, r = hist[4].copy(), rho.copy()
    mu0[3], mu0[5] = 0.0, np.nan
    r[:, 7] = 0.0
    got = en._loglinear_mean(mu0, r, eta)
    assert got[3] == 0.0 and np.isnan(got[5]) and got[7] == mu0[7]
    assert en._mean_of(resp) is en._loglinear_mean and en._mean_of(lc.toy("llh", 3, "linear")[1]) is en._linear_mean
    # truths= on the host generator: trial t is drawn at E exp(rho . truths[t]), on the stream the linear form uses
    truths = 0.1 * rs.randn(5, 12)
    data = en.pseudo_data(grid, 4, 5, 7, response=resp, truths=truths, solver=_FormSolver())
    stream = np.random.RandomState(7)
    for t in range(5):
        row = en._host_row(en._loglinear_mean(hist[4], rho, truths[t]), None, "poisson", stream)
        assert np.array_equal(data[t], row)
    # nuisance="prior" draws truths from the priors and the data at the exponential mean
    data, truth = en.pseudo_data(grid, 4, 6, 3, response=resp, nuisance="prior", return_truth=True, solver=_FormSolver())
    stream = np.random.RandomState(3)
    _, scale, shift, lower, upper = en._truth_priors(resp, 4)
    for t in range(6):
        e = en._host_truths(scale, shift, lower, upper, stream)
        assert np.array_equal(truth[t], e)
        assert np.array_equal(data[t], en._host_row(en._loglinear_mean(hist[4], rho, e), None, "poisson", stream))


def test_form_reaches_the_solver_only_for_loglinear_responses():
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    for n_j, form in ((12, "loglinear"), (3, "loglinear"), (12, "linear")):
        grid, resp, _ = lc.toy(metric, n_j, form)
        solver = _FormSolver()
        data = en.pseudo_data(grid, 4, 6, 3)
        en.metric_matrix(data, grid, metric, True, solver, resp)
        en.delta_metric(data, grid, metric, 4, solver, resp)
        en.accepted(data[:1], grid, metric, np.zeros(len(grid)), solver, resp)
        en.fit_observed(data[:1], grid, metric, resp, solver)
        en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[2], solver=solver, response=resp)
        en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[2], solver=solver, response=resp,
                           nuisance="profiled", observed=data[:1])
        flags = [c[1:] for c in solver.calls if c[0] == "form"]
        assert len(flags) == 7 and all(f == (form, True) for f in flags), (n_j, form, solver.calls)
    # a solver that knows nothing of the keyword: refused by name for a log-linear response, serving every other one
    old = _WideOnly()
    grid, resp, _ = lc.toy(metric, 3)
    data = en.pseudo_data(grid, 4, 6, 3)
    for call in (lambda: en.metric_matrix(data, grid, metric, True, old, resp),
                 lambda: en.delta_metric(data, grid, metric, 4, old, resp),
                 lambda: en.fit_observed(data[:1], grid, metric, resp, old),
                 lambda: en.accepted(data[:1], grid, metric, np.zeros(len(grid)), old, resp),
                 lambda: en.feldman_cousins(grid, metric, 4, random_state=1, solver=old, response=resp)):
        with pytest.raises(ValueError, match="form="):
            call()
    assert not old.calls
    assert en._takes_form(_FormSolver().profiled_matrix) and not en._takes_form(old.profiled_best)
    grid, lin, _ = lc.toy(metric, 3, "linear")
    assert en.metric_matrix(data, grid, metric, True, old, lin).shape == (6, len(grid))


class _WideOnly(pbc.NumpyBoundedProfileSolver):
    """the numpy solver as it was before the form existed: bounds and wide=, no form="""

    def profiled_matrix(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                        max_iter=pc.MAX_ITER, lower=None, upper=None, wide=False):
        return super().profiled_matrix(kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter,
                                       lower, upper)

    def profiled_best(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                      offset=None, k0=0, max_iter=pc.MAX_ITER, lower=None, upper=None, wide=False):
        return super().profiled_best(kind, data, expected, response, sigma2, inv_prior_sigma, center, offset, k0,
                                     max_iter, lower, upper)


def _refused_calls(en, grid, resp, solver, metric):
    data = en.pseudo_data(grid, 4, 6, 3)
    truth = np.zeros((6, len(resp.names)))
    truths = {4: truth}
    return {
        "covariance": lambda: en.delta_metric(data, grid, metric, 4, solver, resp, return_info=True, covariance=True),
        "fit_observed covariance": lambda: en.fit_observed(data[:1], grid, metric, resp, solver, covariance=True),
        "pulls": lambda: en.pulls(data, grid, metric, 4, resp, truth, solver),
        "fitted": lambda: en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[4], solver=solver,
                                             response=resp, nuisance="fitted", observed=data[:1]),
        "posterior": lambda: en.posterior_sample(data[:1], grid, metric, resp, points=[4], n_keep=2, n_walkers=64,
                                                 thin=1, n_burn=1, random_state=1, solver=solver),
        "device prior": lambda: en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[4], solver=solver,
                                                   generator="device", response=resp, nuisance="prior"),
        "device profiled": lambda: en.pseudo_data(grid, 4, 4, 1, generator="device", solver=solver, response=resp,
                                                  nuisance="profiled", observed=data[:1]),
        "device truths": lambda: en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[4], solver=solver,
                                                    generator="device", response=resp, truths=truths),
    }


@pytest.mark.parametrize("n_j", (3, 12))
def test_what_reads_a_linear_kernel_is_refused_for_a_loglinear_response_whatever_j(n_j):
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    grid, resp, _ = lc.toy(metric, n_j)
    solver = _FormSolver()      # (its hesse, posterior and draw_linear* raise AssertionError: no call gets that far)
    for name, call in _refused_calls(en, grid, resp, solver, metric).items():
        with pytest.raises(ValueError, match="log-linear"):
            call()
    assert not solver.calls, solver.calls
    # the device generator with the nuisances left fixed needs no kernel beyond the fit
    crit, _ = en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[4], solver=solver, generator="device",
                                 response=resp)
    assert crit.shape == (1, 2)
    # the same calls with the linear response of 3 parameters get as far as the solver's method
    if n_j == 3:
        grid, lin, _ = lc.toy(metric, 3, "linear")
        for name, call in _refused_calls(en, grid, lin, _FormSolver(), metric).items():
            with pytest.raises(AssertionError, match="reached the solver"):
                call()


@pytest.mark.parametrize("metric", ("llh", "chi2"))
def test_a_linear_response_gives_every_driver_the_numbers_it_gave_before(metric):
    """the solver that takes form= against the solver as it was, on a linear response (wide and bounded): the form
    never reaches either, and every driver returns the same bits"""
    from pisa_amd.analysis import ensemble as en

    for n_j, bounded in ((12, False), (5, True)):
        grid, resp, _ = lc.toy(metric, n_j, "linear", bounded)
        assert "form" not in resp.fit_keywords()
        new, old = _FormSolver(), _WideOnly()
        data = en.pseudo_data(grid, 4, 8, 3)
        assert np.array_equal(en.metric_matrix(data, grid, metric, True, new, resp),
                              en.metric_matrix(data, grid, metric, True, old, resp))
        a, ai = en.delta_metric(data, grid, metric, 4, new, resp, return_info=True)
        b, bi = en.delta_metric(data, grid, metric, 4, old, resp, return_info=True)
        assert np.array_equal(a, b) and np.array_equal(ai["arg"], bi["arg"]) and np.array_equal(ai["eta_at"], bi["eta_at"])
        crit = np.full(len(grid), float(np.median(a)))
        assert np.array_equal(en.accepted(data[:1], grid, metric, crit, new, resp),
                              en.accepted(data[:1], grid, metric, crit, old, resp))
        fa, fb = (en.fit_observed(data[:1], grid, metric, resp, s) for s in (new, old))
        assert np.array_equal(fa["eta"], fb["eta"]) and np.array_equal(fa["value"], fb["value"])
        for nuisance in ("fixed", "prior", "profiled"):
            kw = dict(random_state=1, true_points=[2, 6], response=resp, nuisance=nuisance,
                      observed=data[:1] if nuisance == "profiled" else None)
            ca, _ = en.feldman_cousins(grid, metric, 6, solver=new, **kw)
            cb, _ = en.feldman_cousins(grid, metric, 6, solver=old, **kw)
            assert np.array_equal(ca, cb), (metric, n_j, nuisance)
        assert all(c[1] == "linear" for c in new.calls if c[0] == "form")


FC_TRIALS, FC_SEED, FC_POINTS = 12, 1, [2, 6]
_FC = {}


def observed_map(grid):
    from pisa_amd.analysis import ensemble as en

    return en.pseudo_data(grid, 4, 1, 9)


def host_fc(nuisance, metric="llh"):
    """`feldman_cousins` with the 12-parameter log-linear toy response, the host generator and the numpy solver: what
    the device run of tests/test_gpu_profiled_loglinear.py is compared with"""
    from pisa_amd.analysis import ensemble as en

    if (nuisance, metric) not in _FC:
        grid, resp, _ = lc.toy(metric, 12)
        _FC[(nuisance, metric)] = en.feldman_cousins(
            grid, metric, FC_TRIALS, random_state=FC_SEED, true_points=FC_POINTS, solver=_FormSolver(), response=resp,
            nuisance=nuisance, observed=observed_map(grid) if nuisance == "profiled" else None)
    return _FC[(nuisance, metric)]


@pytest.mark.parametrize("nuisance", ("fixed", "prior", "profiled"))
def test_feldman_cousins_with_12_loglinear_parameters_on_the_host_generator(nuisance):
    from pisa_amd.analysis import ensemble as en

    crit, info = host_fc(nuisance)
    assert crit.shape == (2, 2) and np.all(crit >= 0) and not info["flagged"].any()
    grid, resp, _ = lc.toy("llh", 12)
    got, _ = en.feldman_cousins(grid, "llh", FC_TRIALS, random_state=FC_SEED, true_points=FC_POINTS,
                                solver=_FormSolver(), response=resp, nuisance=nuisance,
                                observed=observed_map(grid) if nuisance == "profiled" else None,
                                chunk_bytes=5 * 8 * grid.n_bins)
    assert np.array_equal(got, crit)
