"""The wide form of the profiled trial ensembles without a GPU: the constants of its gate measured again
(tests/profile_wide_cases.py), the wide solver's own source (csrc/profile_wide_device.hpp: every cooperative phase a
function of (shared state, lane)) compiled for the host under the sanitizers and run lane by lane against the numpy
restatements, and the `wide=` paths of pisa_amd/analysis/ensemble.py with a numpy solver.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import profile_bounded_cases as pbc
from tests import profile_cases as pc
from tests import profile_wide_cases as wc

_WORST = {}


def _worst(bounded):
    """(worst ratio per kind, most Newton steps) of the restatement over the gated wide cases; every pair of every case
    has status 0 in the exact reference and in the restatement (bounded: and the same coordinates on a bound)"""
    if bounded not in _WORST:
        worst, steps = {k: 0.0 for k in pc.KINDS}, 0
        cases = [(fam, bx, shape) for fam, bx, shape in wc.GATED_BOUNDED] if bounded else [
            (fam, None, shape) for fam, shape in wc.GATED]
        for fam, bx, shape in cases:
            for kind in pc.KINDS:
                what = "%s %s %s %s" % (fam, bx, shape, kind)
                ex = pbc.exact_bounded(fam, bx, kind, *shape) if bounded else pc.exact(fam, kind, *shape)
                got = wc.restated(fam, kind, shape, bx)
                assert not ex["status"].any(), (what, np.unique(ex["status"]))
                assert not got["status"].any(), (what, np.unique(got["status"]))
                if bounded:
                    lower, upper = wc.bounds(bx, shape[1], shape[3])
                    assert np.array_equal(pbc.on_bound(got["eta"], lower, upper),
                                          pbc.on_bound(ex["eta"], lower, upper)), what
                worst[kind] = max(worst[kind], ec.check(got["value"], ex["value"], ex["scale"], pc.G_HOST, what))
                steps = max(steps, int(got["n_iter"].max()))
        _WORST[bounded] = (worst, steps)
    return _WORST[bounded]


@pytest.mark.parametrize("bounded", (False, True))
def test_g_ref_w_is_the_measured_worst_ratio_of_the_restatement(bounded):
    worst, steps = _worst(bounded)
    recorded = wc.G_REF_WB if bounded else wc.G_REF_W
    print("bounded %s: measured %s, recorded %s, at most %d Newton steps" % (bounded, worst, recorded, steps))
    assert set(recorded) == set(pc.KINDS)
    for kind in pc.KINDS:
        assert worst[kind] <= pc.G_HOST
        assert worst[kind] <= recorded[kind] <= worst[kind] + 0.02, kind
        assert wc.g_of(kind, bounded) == pc.mc.KERNEL_FACTOR * max(1.0, recorded[kind])
    assert steps <= wc.MOST_STEPS <= wc.MAX_ITER // 2


def test_every_edge_of_the_issue_is_among_the_shapes():
    shapes = [s for _, s in wc.GATED + wc.UNGATED]
    assert {1, 8, 9, 16, 17, 31, 32} <= {s[3] for s in shapes}
    assert {1, 3, wc.CHUNK - 1, wc.CHUNK, wc.CHUNK + 1, 130} <= {s[2] for s in shapes}
    assert {1, 2} <= {s[0] for s in shapes} and (8, 300, 12, 12) in shapes and (66, 2, 20, 32) in shapes
    assert ("poisson", (1, 1, 1, 9)) in wc.GATED           # B = 1, J = 9: priors on every parameter
    assert pc.family("poisson", 1, 1, 1, 9)["ips"].all()
    assert {bx for _, bx, _ in wc.GATED_BOUNDED} == set(pbc.BOXES)
    assert ("poisson", "wide", (3, 2, 64, 16)) in wc.GATED_BOUNDED
    # the J > B shape is ungated because the restatement flags pairs of it
    for fam, shape in wc.UNGATED:
        assert any(wc.restated(fam, kind, shape)["status"].any() for kind in pc.KINDS)


# ------------------------------------------------------------- the kernel's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through the phases of profile_wide_device.hpp as the kernel strings them together,
// with a loop over the lanes where the kernel has its wavefront: eight int64 (kind, T, K, B, J, shared response,
// max_iter, bounded), then D [T][B], E and S2 [K][B], R [K or 1][J][B], ips [J], c [K][J], lo and hi [K][J]; per
// case value [T][K], eta [T][K][J], then n_iter and status as doubles.  Every pair is run twice, the lanes of a phase
// in ascending and in descending order: a phase in which a lane reads what another lane writes would differ.
#include "profile_wide_device.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace pisa;
struct Case {
    int64_t kind, T, K, B, J, shared, max_iter, bounded;
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
template <int KIND, class X>
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
            x.each([&](int l) { pfw_bins<KIND>(S, R, l, nb); });
            x.each([&](int l) { pfw_chains(S, R, l, nb); });
        }
        pfw_decide<KIND>(S, x, (int32_t)q.max_iter);
    }
    x.each([&](int l) { pfw_value_begin(S, l); });
    for (int64_t c0 = 0; c0 < q.B; c0 += PFW_CHUNK) {
        const int nb = (int)(q.B - c0 < PFW_CHUNK ? q.B - c0 : PFW_CHUNK);
        x.each([&](int l) { stage(q, S, R, t, k, c0, l); });
        x.each([&](int l) { pfw_value_bins<KIND>(S, R, l, nb); });
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
template <int KIND>
static void run(const Case &q, FILE *out) {
    const int J = (int)q.J;
    std::vector<double> value(q.T * q.K), eta(q.T * q.K * J), iters(q.T * q.K), status(q.T * q.K);
    for (int64_t t = 0; t < q.T; t++)
        for (int64_t k = 0; k < q.K; k++) {
            const Pair a = run_pair<KIND, HostLanes<true>>(q, t, k), b = run_pair<KIND, HostLanes<false>>(q, t, k);
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
static bool take(FILE *in, std::vector<double> &v, int64_t n) {
    v.resize(n);
    return fread(v.data(), 8, n, in) == (size_t)n;
}
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int64_t head[8];
    int n_cases = 0;
    while (fread(head, 8, 8, in) == 8) {
        Case q;
        q.kind = head[0], q.T = head[1], q.K = head[2], q.B = head[3], q.J = head[4], q.shared = head[5];
        q.max_iter = head[6], q.bounded = head[7];
        if (q.J < 1 || q.J > PFW_MAX_PARAMS) return 3;
        if (!take(in, q.D, q.T * q.B) || !take(in, q.E, q.K * q.B) || !take(in, q.S2, q.K * q.B) ||
            !take(in, q.R, (q.shared ? 1 : q.K) * q.J * q.B) || !take(in, q.ips, q.J) || !take(in, q.c, q.K * q.J) ||
            !take(in, q.lo, q.K * q.J) || !take(in, q.hi, q.K * q.J))
            return 3;
        switch (q.kind) {
        case PF_LLH: run<PF_LLH>(q, out); break;
        case PF_POISSON_LLH: run<PF_POISSON_LLH>(q, out); break;
        case PF_CHI2: run<PF_CHI2>(q, out); break;
        default: run<PF_MOD_CHI2>(q, out);
        }
        n_cases++;
    }
    fclose(out);
    printf("%d %d\n", n_cases, n_order);
    return 0;
}
"""


def _cases():
    """(name, shape or None, box or None, f with kind / max_iter / lower / upper, the restatement's outputs)"""
    cases = []

    def add(name, shape, bx, f, want):
        cases.append((name, shape, bx, f, want))

    for fam, shape in wc.GATED + wc.UNGATED:
        f = pc.family(fam, *shape)
        for kind in pc.KINDS:
            add(fam, shape, None, dict(f, kind=kind, max_iter=wc.MAX_ITER, lower=None, upper=None),
                wc.restated(fam, kind, shape))
    for fam, bx, shape in wc.GATED_BOUNDED + tuple((fam, "pinned", shape) for fam, shape in wc.GATED[-4:-1]):
        f = pc.family(fam, *shape)
        lower, upper = wc.bounds(bx, shape[1], shape[3])
        for kind in pc.KINDS:
            add(fam, shape, bx, dict(f, kind=kind, max_iter=wc.MAX_ITER, lower=lower, upper=upper),
                wc.restated(fam, kind, shape, bx))
    # the narrow form's own cases, J <= 8 (the two large shapes left to the device): the restatement, hence the
    # narrow header
    for fam, shape in pc.gated_cases():
        if shape in (pc.STRIP_SHAPE, pc.TILE_SHAPE) or shape[0] * shape[1] > 600:
            continue
        f = pc.family(fam, *shape)
        for kind in pc.KINDS[::3]:
            add(fam, shape, None, dict(f, kind=kind, max_iter=pc.MAX_ITER, lower=None, upper=None), None)
    for name in pc.STATUS_FAMILIES:
        add(name, None, None, dict(pc.status_family(name), lower=None, upper=None), None)
    for name in pbc.STATUS_FAMILIES:
        add(name, None, "own", pbc.status_family(name), None)
    return cases


def test_the_wide_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/profile_wide_device.hpp compiled with g++ under ASan + UBSan and run as a program of its own, a loop over
    the lanes in the kernel's place: status, n_iter and eta `==` the restatement's (so the coordinates on a bound are
    the restatement's), every value of a gated case inside the gate of the exact reference, every other value inside
    it around the exact value at the returned eta; the order of the lanes within a phase changes no bit"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "profile_wide_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = _cases()
    with open(tmp_path / "cases.bin", "wb") as fh:
        for _, _, _, f, _ in cases:
            T, B = f["D"].shape
            K = f["E"].shape[0]
            J = f["R"].shape[-2]
            bounded = f["lower"] is not None or f["upper"] is not None
            lo, hi = pbc.full_bounds(f["lower"], f["upper"], K, J)
            fh.write(np.array([pc.KINDS.index(f["kind"]), T, K, B, J, int(f["R"].ndim == 2), f["max_iter"],
                               int(bounded)], dtype=np.int64).tobytes())
            for a in (f["D"], f["E"], f["S2"], f["R"], np.zeros(J) if f["ips"] is None else f["ips"],
                      np.zeros((K, J)) if f["c"] is None else f["c"], lo, hi):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.split() == [str(len(cases)), "0"], res.stdout
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    worst = {False: {k: 0.0 for k in pc.KINDS}, True: {k: 0.0 for k in pc.KINDS}}
    for name, shape, bx, f, want in cases:
        T, K, J = f["D"].shape[0], f["E"].shape[0], f["R"].shape[-2]
        n = T * K
        value = got_all[at:at + n].reshape(T, K)
        eta = got_all[at + n:at + n + n * J].reshape(T, K, J)
        n_iter = got_all[at + n + n * J:at + 2 * n + n * J].reshape(T, K)
        status = got_all[at + 2 * n + n * J:at + 3 * n + n * J].reshape(T, K)
        at += 3 * n + n * J
        kind = f["kind"]
        bounded = f["lower"] is not None or f["upper"] is not None
        if want is None:
            want = (pbc.solve_bounded(kind, f["D"], f["E"], f["R"], f["lower"], f["upper"], f["S2"], f["ips"], f["c"],
                                      f["max_iter"]) if bounded else
                    pc.solve(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"]))
        what = "%s %s %s %s" % (name, shape, bx, kind)
        assert np.array_equal(status, want["status"]), what
        assert np.array_equal(n_iter, want["n_iter"]), what
        assert np.array_equal(eta, want["eta"]), what
        if bounded:
            assert np.array_equal(pbc.on_bound(eta, f["lower"], f["upper"]),
                                  pbc.on_bound(want["eta"], f["lower"], f["upper"])), what
        wide_case = shape is not None and J > pc.MAX_PARAMS or (name, shape) in wc.GATED
        g = wc.g_of(kind, bounded) if wide_case else (pbc.g_of(kind) if bounded else pc.g_of(kind))
        gated = ((name, shape) in wc.GATED and bx is None) or (name, bx, shape) in wc.GATED_BOUNDED or (
            shape is not None and not wide_case)
        if gated:
            ex = pbc.exact_bounded(name, bx, kind, *shape) if bounded else pc.exact(name, kind, *shape)
            r = ec.check(value, ex["value"], ex["scale"], g, what)
            if wide_case:
                worst[bounded][kind] = max(worst[bounded][kind], r)
        else:
            val, scale = pc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], eta.astype(np.longdouble), f["ips"],
                                        f["c"])
            ec.check(value, val, scale, g, what)
    assert at == got_all.size
    print("the wide header on the host: worst ratios %s" % worst)


# --------------------------------------------------------------------------- the ensemble's plumbing
class _WideSolver(pbc.NumpyBoundedProfileSolver):
    """the numpy solver with the keyword of the wide form: the restatements are generic in J"""

    def profiled_matrix(self, *args, wide=False, **kw):
        self.calls.append(("wide", bool(wide)))
        return super().profiled_matrix(*args, **kw)

    def profiled_best(self, *args, wide=False, **kw):
        self.calls.append(("wide", bool(wide)))
        return super().profiled_best(*args, **kw)

    def hesse(self, *args, **kw):
        raise AssertionError("a refused call reached the solver")

    posterior = draw_linear = draw_linear_mvn = draw_linear_at = hesse

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        from tests import fluctuate_cases as fc

        return fc.block(mu, n_trials, seed, stream, first_trial)[0]


def toy(metric, n_j, wide=True, bounded=False):
    """the toy grid of tests/ensemble_cases.py with n_j nuisance parameters that are not dimensions of the grid: a
    normalisation with a 10 % Gaussian prior that sits 0.05 above its mean at every point, then cosine modes of
    falling size with a Gaussian prior of width 0.2 on every second one"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    K, B = hist.shape
    x = (np.arange(B) + 0.5) / B
    modes = [np.ones(B)] + [np.cos(j * np.pi * x) / (1.0 + j) for j in range(1, n_j)]
    R = np.stack([hist * m[None, :] for m in modes], axis=1)
    ips = np.array([10.0] + [5.0 if j % 2 else 0.0 for j in range(1, n_j)])
    center = np.zeros((K, n_j))
    center[:, 0] = 0.05
    share = (ips[0] * 0.05) ** 2 * (1.0 if metric in ("chi2", "mod_chi2") else -0.5)
    prior_at_point = np.full(K, share)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty + prior_at_point, metric)
    kw = dict(lower=np.full(n_j, -0.2), upper=np.full(n_j, 0.3)) if bounded else {}
    resp = en.NuisanceResponse(tuple("p%d" % j for j in range(n_j)), R, ips, center, prior_at_point,
                               np.zeros((K, n_j)), wide=wide, **kw)
    return grid, resp, penalty


def test_wide_responses_take_up_to_32_names_and_the_default_stays_at_8():
    from pisa_amd.analysis import ensemble as en

    for n in (9, 32):
        r = en.NuisanceResponse(tuple("n%d" % j for j in range(n)), np.zeros((9, n, 24)), wide=True)
        assert r.wide and r.fit_keywords() == {"wide": True}
    for n in (0, 33):
        with pytest.raises(ValueError, match="1 to 32"):
            en.NuisanceResponse(tuple("n%d" % j for j in range(n)), np.zeros((9, n, 24)), wide=True)
    with pytest.raises(ValueError, match="1 to 8"):
        en.NuisanceResponse(tuple("abcdefghi"), np.zeros((9, 9, 24)))
    narrow = en.NuisanceResponse(("a", "b"), np.zeros((9, 2, 24)))
    assert not narrow.wide and narrow.fit_keywords() == {}
    boxed = en.NuisanceResponse(("a",), np.zeros((9, 1, 24)), lower=[-1.0], upper=[1.0], wide=True)
    assert set(boxed.fit_keywords()) == {"lower", "upper", "wide"} and set(boxed.bounds()) == {"lower", "upper"}


def test_wide_reaches_the_solver_only_for_wide_responses():
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    for n_j, wide in ((12, True), (3, True), (3, False)):
        grid, resp, _ = toy(metric, n_j, wide)
        solver = _WideSolver()
        data = en.pseudo_data(grid, 4, 6, 3)
        en.metric_matrix(data, grid, metric, True, solver, resp)
        en.delta_metric(data, grid, metric, 4, solver, resp)
        en.accepted(data[:1], grid, metric, np.zeros(len(grid)), solver, resp)
        en.fit_observed(data[:1], grid, metric, resp, solver)
        en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[2], solver=solver, response=resp)
        flags = [c[1] for c in solver.calls if c[0] == "wide"]
        assert len(flags) == 5 and all(f == wide for f in flags), (n_j, wide, solver.calls)
    # a solver that knows nothing of the keyword: refused by name for a wide response, serving a narrow one
    old = pbc.NumpyBoundedProfileSolver()
    grid, resp, _ = toy(metric, 3, True)
    data = en.pseudo_data(grid, 4, 6, 3)
    for call in (lambda: en.metric_matrix(data, grid, metric, True, old, resp),
                 lambda: en.delta_metric(data, grid, metric, 4, old, resp),
                 lambda: en.fit_observed(data[:1], grid, metric, resp, old),
                 lambda: en.accepted(data[:1], grid, metric, np.zeros(len(grid)), old, resp),
                 lambda: en.feldman_cousins(grid, metric, 4, random_state=1, solver=old, response=resp)):
        with pytest.raises(ValueError, match="wide="):
            call()
    assert not old.calls
    grid, resp, _ = toy(metric, 3, False)
    assert en.metric_matrix(data, grid, metric, True, old, resp).shape == (6, len(grid))
    # ... and both forms give the same numbers through the restatement
    grid, wide3, _ = toy(metric, 3, True)
    assert np.array_equal(en.metric_matrix(data, grid, metric, True, _WideSolver(), wide3),
                          en.metric_matrix(data, grid, metric, True, old, resp))


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


def test_what_stays_limited_to_8_parameters_is_refused_above_8_and_not_below():
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    grid, resp, _ = toy(metric, 12)
    solver = _WideSolver()      # (its hesse, posterior and draw_linear* raise AssertionError: no call gets that far)
    for name, call in _refused_calls(en, grid, resp, solver, metric).items():
        with pytest.raises(ValueError, match="limited to 8 nuisance parameters"):
            call()
    assert not solver.calls, solver.calls
    # the device generator with the nuisances left fixed needs no kernel beyond the fit
    crit, _ = en.feldman_cousins(grid, metric, 4, random_state=1, true_points=[4], solver=solver, generator="device",
                                 response=resp)
    assert crit.shape == (1, 2)
    # a wide response of 3 parameters gets as far as the solver's method in every one of them
    grid, resp, _ = toy(metric, 3)
    for name, call in _refused_calls(en, grid, resp, _WideSolver(), metric).items():
        with pytest.raises(AssertionError, match="reached the solver"):
            call()


@pytest.mark.parametrize("nuisance", ("fixed", "prior", "profiled"))
def test_feldman_cousins_on_the_host_generator_with_12_parameters_does_not_depend_on_chunks(nuisance):
    from pisa_amd.analysis import ensemble as en

    crit, info = host_fc(nuisance)
    assert crit.shape == (2, 2) and np.all(crit >= 0) and not info["flagged"].any()
    metric = "llh"
    grid, resp, _ = toy(metric, 12)
    got, _ = en.feldman_cousins(grid, metric, FC_TRIALS, random_state=FC_SEED, true_points=FC_POINTS,
                                solver=_WideSolver(), response=resp, nuisance=nuisance,
                                observed=observed_map(grid) if nuisance == "profiled" else None,
                                chunk_bytes=5 * 8 * grid.n_bins)
    assert np.array_equal(got, crit)
    one, _ = en.feldman_cousins(grid, metric, FC_TRIALS, random_state=FC_SEED, true_points=FC_POINTS[1:],
                                solver=_WideSolver(), response=resp, nuisance=nuisance,
                                observed=observed_map(grid) if nuisance == "profiled" else None)
    assert np.array_equal(one, crit[1:])


FC_TRIALS, FC_SEED, FC_POINTS = 12, 1, [2, 6]
_FC = {}


def observed_map(grid):
    from pisa_amd.analysis import ensemble as en

    return en.pseudo_data(grid, 4, 1, 9)


def host_fc(nuisance, metric="llh"):
    """`feldman_cousins` with the 12-parameter wide toy response, the host generator and the numpy solver: what the
    device run of tests/test_gpu_profiled_wide.py is compared with"""
    from pisa_amd.analysis import ensemble as en

    if (nuisance, metric) not in _FC:
        grid, resp, _ = toy(metric, 12)
        _FC[(nuisance, metric)] = en.feldman_cousins(
            grid, metric, FC_TRIALS, random_state=FC_SEED, true_points=FC_POINTS, solver=_WideSolver(), response=resp,
            nuisance=nuisance, observed=observed_map(grid) if nuisance == "profiled" else None)
    return _FC[(nuisance, metric)]


@pytest.mark.parametrize("metric", ("llh", "chi2", "mod_chi2"))
def test_no_prior_is_counted_twice_with_12_parameters(metric):
    """the check of tests/test_host_profiled.py at J = 12"""
    from pisa_amd.analysis import ensemble as en

    grid, resp, other = toy(metric, 12)
    solver = _WideSolver()
    data = en.pseudo_data(grid, 4, 10, 3)
    full = pc.restated(metric, data, grid.hist, resp.response, grid.sigma2_for(metric), resp.inv_prior_sigma, resp.center)
    assert not full["status"].any()
    m = en.metric_matrix(data, grid, metric, True, solver, resp)
    assert np.array_equal(m, full["value"] + other[None, :])
    assert np.array_equal(en.metric_matrix(data, grid, metric, False, solver, resp), full["value"])
    plain = en.metric_matrix(data, grid, metric, True, solver)
    at_zero = pc.value(metric, data, grid.hist, resp.response, grid.sigma2_for(metric), np.zeros(full["eta"].shape),
                       resp.inv_prior_sigma, resp.center) + other[None, :]
    scale = ec.scale_fp64(metric, data, grid.hist, grid.sigma2_for(metric))
    assert np.all(np.abs(at_zero - plain) <= 4 * pc.EPS * (scale + np.abs(plain)))
    sign = 1.0 if metric in ec.LLH_KINDS else -1.0
    tol = wc.g_of(metric) * pc.EPS * (scale + np.abs(plain))
    assert np.all(sign * (m - plain) >= -tol)
    assert np.any(sign * (m - plain) > 1e-3)
    for k0 in (0, 4):
        delta, info = en.delta_metric(data, grid, metric, k0, solver, resp, return_info=True)
        red = pc.reduce_profiled(metric, full, other, k0)
        assert np.array_equal(delta, sign * (red["best"] - red["at"])) and np.all(delta >= 0)
        assert info["flagged"] == 0 and np.array_equal(info["arg"], red["arg"])
        assert np.array_equal(info["eta_best"], red["eta_best"]) and np.array_equal(info["eta_at"], red["eta_at"])
        assert info["eta_at"].shape == (10, 12)
