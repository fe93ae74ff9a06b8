"""The bounded profiled trial ensembles without a GPU (tests/profile_bounded_cases.py): the numpy restatement of the
projected Newton iteration against the exact reference on every box, gated family and shape (G_REF_B measured again
and held against the recorded figures; every pair with status 0 in both, the same coordinates on a bound in both, no
pair beyond max_iter), the KKT conditions in longdouble at the restatement's eta, an independent oracle that tries
every assignment of the coordinates to (free, at lo, at hi), the closed forms, the status families, the solver's own
source (csrc/profile_device.hpp) compiled for the host under the sanitizers against the restatement, and the bounded
`response=` paths of pisa_amd/analysis/ensemble.py with a numpy solver.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import fluctuate_cases as fc
from tests import profile_bounded_cases as bc
from tests import profile_cases as pc

_RESTATED = {}
_WORST = {}


def _restated(name, bx, shape, kind):
    key = (name, bx, shape, kind)
    if key not in _RESTATED:
        f = pc.family(name, *shape)
        lower, upper = bc.box(bx, shape[1], shape[3])
        _RESTATED[key] = bc.restated_bounded(kind, f["D"], f["E"], f["R"], lower, upper, f["S2"], f["ips"], f["c"])
    return _RESTATED[key]


def _worst(kind):
    """(worst ratio of the restatement, where, most Newton steps, share of pairs with a coordinate on a bound) over
    every gated case.  Conditions, not measurements: every pair has status 0 in the exact reference and in the
    restatement, no coordinate is on a bound in one and off it in the other, no pair needs more than max_iter steps"""
    if kind not in _WORST:
        worst, where, steps, bound, pairs = 0.0, None, 0, 0, 0
        for name, bx, shape in bc.gated_cases():
            ex = bc.exact_bounded(name, bx, kind, *shape)
            what = "%s %s %s %s" % (name, bx, shape, kind)
            assert not ex["status"].any(), (what, np.unique(ex["status"]))
            got = _restated(name, bx, shape, kind)
            assert not got["status"].any(), (what, np.unique(got["status"]))
            assert int(got["n_iter"].max()) <= pc.MAX_ITER, what
            lower, upper = bc.box(bx, shape[1], shape[3])
            on_got, on_ex = bc.on_bound(got["eta"], lower, upper), bc.on_bound(ex["eta"], lower, upper)
            assert np.array_equal(on_got, on_ex), (what, int(np.count_nonzero(on_got != on_ex)))
            r = float(ec.gate_ratio(got["value"], ex["value"], ex["scale"]).max())
            steps = max(steps, int(got["n_iter"].max()))
            bound += int(np.count_nonzero(on_got.any(axis=2)))
            pairs += on_got.shape[0] * on_got.shape[1]
            if r > worst:
                worst, where = r, (name, bx, shape)
        _WORST[kind] = (worst, where, steps, bound / pairs)
    return _WORST[kind]


@pytest.mark.parametrize("kind", pc.KINDS)
def test_g_ref_b_is_the_measured_worst_ratio_of_the_restatement(kind):
    worst, where, steps, share = _worst(kind)
    print("%s: measured %.4f at %s, recorded %.2f, at most %d Newton steps, %.0f %% of the pairs on a bound" % (
        kind, worst, where, bc.G_REF_B[kind], steps, 100 * share))
    assert worst <= bc.G_REF_B[kind] <= worst + 0.02
    assert bc.g_of(kind) == pc.mc.KERNEL_FACTOR * max(1.0, bc.G_REF_B[kind])
    assert steps <= bc.MOST_STEPS <= pc.MAX_ITER
    assert share > 0.5                       # (the boxes bind: the families test the projected step, not the free one)
    assert set(bc.G_REF_B) == set(pc.KINDS)


def test_the_boxes_are_the_issues():
    lo, hi = bc.box("wide", 3, 4)
    assert lo.shape == hi.shape == (4,) and np.allclose(lo, -0.25 * (1 + 0.1 * np.arange(4)))
    assert np.allclose(hi, 0.25 * (1 + 0.2 * np.arange(4)))
    lo, hi = bc.box("narrow", 3, 4)
    assert lo.shape == hi.shape == (3, 4) and np.allclose(lo[2], -0.05 * (1 + 0.1 * np.arange(4)))
    assert np.allclose(hi[0], 0.05 * (1 + 0.2 * np.arange(4)))
    lo, hi = bc.box("lower", 3, 4)
    assert hi is None and np.array_equal(lo, bc.box("wide", 3, 4)[0])
    assert len(bc.gated_cases()) == 3 * len(pc.gated_cases())


KKT_CASES = [("poisson", "wide", (65, 3, 65, 8)), ("poisson", "narrow", (64, 17, 64, 5)), ("prior", "wide", (63, 3, 3, 2)),
             ("shared", "narrow", (257, 3, 64, 2)), ("asimov", "lower", (63, 17, 65, 1)), ("low", "wide", (65, 1, 3, 1)),
             ("far", "narrow", (63, 17, 65, 1)), ("poisson", "lower", (64, 3, 3, 8))]


@pytest.mark.parametrize("kind", ("llh", "chi2", "mod_chi2"))
def test_kkt_conditions_hold_in_longdouble_at_the_restatements_eta(kind):
    """off the bounds the squared scaled gradient g_j^2 / H_jj (a lower bound of the free block's squared Newton
    decrement) lies below Phi's fp64 rounding floor; on a bound the gradient points out of the box, or lies below it"""
    n_free = 0
    for name, bx, shape in KKT_CASES:
        f = pc.family(name, *shape)
        got = _restated(name, bx, shape, kind)
        lower, upper = bc.box(bx, shape[1], shape[3])
        on = bc.on_bound(got["eta"], lower, upper)
        g, diag, floor_ = bc.gradient(kind, f, got["eta"])
        small = (g * g / diag).astype(np.float64) <= floor_[:, :, None]
        what = "%s %s %s %s" % (name, bx, shape, kind)
        assert np.all(small[on == 0]), (what, float((g * g / diag / floor_[:, :, None])[on == 0].max()))
        assert np.all((g[on == -1] >= 0) | small[on == -1]), what
        assert np.all((g[on == 1] <= 0) | small[on == 1]), what
        assert np.any(on != 0), what
        n_free += int(np.count_nonzero(on == 0))
    assert n_free > 0


# ------------------------------------------------------------------------- an oracle that shares no bound-set rule
def _phi_g_h(kind, one, eta):
    """(Phi, g [J], H [J, J], inside) of one pair at eta [J] in longdouble, priors included"""
    ld = np.longdouble
    J = eta.size
    inside, s, c, _, g, H = pc._sweep(kind, one["D"], one["E"], one["S2"], one["R"], eta.reshape(1, 1, J).astype(ld))
    w = ld(pc.w_of(kind))
    phi, g = (s + c)[0, 0], g[0, 0].copy()
    Hm = np.zeros((J, J), dtype=ld)
    for i in range(J):
        for j in range(i + 1):
            Hm[i, j] = Hm[j, i] = H[(i, j)][0, 0]
    for j in range(J):
        p = ld(one["ips"][j]) * (eta[j] + ld(one["c"][0, j]))
        phi = phi + w * p * p
        g[j] += 2 * w * ld(one["ips"][j]) * p
        Hm[j, j] += 2 * w * ld(one["ips"][j]) ** 2
    return phi, g, Hm, bool(inside[0, 0])


def _gauss(A, b):
    """A x = b by Gaussian elimination with partial pivoting, in the arrays' own precision"""
    A, b = A.copy(), b.copy()
    n = b.size
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            m = A[i, k] / A[k, k]
            A[i, k:] -= m * A[k, k:]
            b[i] -= m * b[k]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def _equality_constrained(kind, one, fixed):
    """argmin Phi with the coordinates of `fixed` {j: value} held, by longdouble Newton with backtracking from the
    held point -> (eta [J], g [J]) or None where the iteration leaves the domain for good"""
    ld = np.longdouble
    J = one["R"].shape[1]
    eta = np.zeros(J, dtype=ld)
    for j, v in fixed.items():
        eta[j] = ld(v)
    free = [j for j in range(J) if j not in fixed]
    phi, g, H, inside = _phi_g_h(kind, one, eta)
    if not inside:
        return None
    for _ in range(200):
        if not free:
            break
        step = np.zeros(J, dtype=ld)
        step[free] = -_gauss(H[np.ix_(free, free)], g[free])
        lam2 = -(g[free] @ step[free])
        if lam2 <= ld(1e-33) * (abs(phi) + 1):
            break
        alpha = ld(1)
        for _ in range(80):
            phi_t, g_t, H_t, inside = _phi_g_h(kind, one, eta + alpha * step)
            # (a step whose decrement is below what Phi resolves in longdouble is a pure Newton step)
            if inside and (phi_t <= phi or lam2 <= ld(1e-16) * (abs(phi) + 1)):
                break
            alpha /= 2
        else:
            break
        eta, phi, g, H = eta + alpha * step, phi_t, g_t, H_t
    return eta, g


ORACLE_CASES = [("poisson", "wide", (63, 3, 3, 2), [(0, 0), (1, 1), (2, 2), (5, 0), (7, 1)]),
                ("poisson", "narrow", (64, 300, 12, 3), [(0, 0), (1, 1), (3, 2), (4, 7)]),
                ("prior", "lower", (64, 300, 12, 3), [(0, 0), (2, 1), (5, 3)]),
                ("low", "wide", (65, 1, 3, 1), [(0, 0), (9, 0)]), ("far", "lower", (65, 1, 3, 1), [(3, 0)])]


@pytest.mark.parametrize("kind", ("llh", "chi2"))
def test_an_oracle_over_all_assignments_finds_the_exact_references_eta(kind):
    """each of the 3^J assignments (free / at lo / at hi): the equality-constrained minimum by a Newton iteration of
    its own; exactly one assignment is feasible with the multipliers' signs right, and it is the exact reference's"""
    ld = np.longdouble
    seen = set()
    for name, bx, shape, pairs in ORACLE_CASES:
        f = pc.family(name, *shape)
        K, J = shape[1], shape[3]
        ex = bc.exact_bounded(name, bx, kind, *shape)
        lo, hi = bc.full_bounds(*bc.box(bx, K, J), K, J)
        R = f["R"] if f["R"].ndim == 3 else np.broadcast_to(f["R"][None], (K,) + f["R"].shape)
        for t, k in pairs:
            one = dict(D=f["D"][t:t + 1], E=f["E"][k:k + 1], S2=f["S2"][k:k + 1], R=R[k:k + 1],
                       ips=np.zeros(J) if f["ips"] is None else f["ips"],
                       c=np.zeros((1, J)) if f["c"] is None else f["c"][k:k + 1])
            found = []
            for assign in itertools.product((0, -1, 1), repeat=J):
                if any((a == -1 and np.isinf(lo[k, j])) or (a == 1 and np.isinf(hi[k, j])) for j, a in enumerate(assign)):
                    continue
                fixed = {j: (lo[k, j] if a == -1 else hi[k, j]) for j, a in enumerate(assign) if a}
                sol = _equality_constrained(kind, one, fixed)
                if sol is None:
                    continue
                eta, g = sol
                tiny = ld(1e-12) * (1 + np.abs(g).max())
                feasible = all(lo[k, j] < eta[j] < hi[k, j] for j, a in enumerate(assign) if a == 0)
                signs = all((g[j] >= -tiny) if a == -1 else (g[j] <= tiny) for j, a in enumerate(assign) if a)
                stationary = all(abs(g[j]) <= tiny for j, a in enumerate(assign) if a == 0)
                if feasible and signs and stationary:
                    found.append((assign, eta))
            what = "%s %s %s %s pair %s" % (name, bx, shape, kind, (t, k))
            assert len(found) == 1, (what, [a for a, _ in found])
            assign, eta = found[0]
            want = ex["eta"][t, k]
            assert np.all(np.abs(eta - want) <= 1e-9 * (1 + np.abs(want))), (what, assign, eta, want)
            assert np.array_equal(np.array(assign), np.where(want == lo[k], -1, np.where(want == hi[k], 1, 0))), what
            seen.update(assign)
    assert seen == {0, -1, 1}


# ----------------------------------------------------------------------------------------------- closed forms
def test_closed_forms():
    # norm: one scale, R = E, no prior: the unconstrained minimum of a convex function of one variable, clipped
    for bx in bc.BOXES:
        for shape in pc.shapes_of("norm"):
            f = pc.family("norm", *shape)
            lower, upper = bc.box(bx, shape[1], 1)
            lo, hi = bc.full_bounds(lower, upper, shape[1], 1)
            got = bc.solve_bounded("llh", f["D"], f["E"], f["R"], lower, upper, f["S2"])
            free = f["D"].sum(axis=1)[:, None] / f["E"].sum(axis=1)[None, :] - 1.0
            want = np.clip(free, lo[None, :, 0], hi[None, :, 0])
            assert not got["status"].any()
            assert np.all(np.abs(got["eta"][:, :, 0] - want) <= 64 * pc.EPS * (1.0 + np.abs(want))), (bx, shape)
            clipped = want != free
            assert np.array_equal(got["eta"][:, :, 0][clipped], want[clipped])       # the bound's own double
    for fam, shape in (("poisson", (65, 3, 65, 8)), ("prior", (64, 17, 64, 5)), ("shared", (63, 3, 3, 2))):
        f = pc.family(fam, *shape)
        T, K, _, J = shape
        for kind in pc.KINDS:
            # every parameter pinned at 0: the metric at eta = 0, no step
            got = bc.restated_bounded(kind, f["D"], f["E"], f["R"], np.zeros(J), np.zeros((K, J)), f["S2"], f["ips"],
                                      f["c"])
            assert not got["status"].any() and not got["n_iter"].any() and not got["eta"].any(), (fam, kind)
            assert not np.signbit(got["eta"]).any()
            assert np.array_equal(got["value"], pc.value(kind, f["D"], f["E"], f["R"], f["S2"], np.zeros((T, K, J)),
                                                         f["ips"], f["c"])), (fam, kind)
            # all bounds infinite (given, or left out on one side): the unbounded restatement, array for array
            want = pc.restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"])
            for lower, upper in ((np.full(J, -np.inf), np.full((K, J), np.inf)), (None, np.full(J, np.inf)), (None, None)):
                got = bc.restated_bounded(kind, f["D"], f["E"], f["R"], lower, upper, f["S2"], f["ips"], f["c"])
                for key in ("eta", "n_iter", "status", "value"):
                    assert np.array_equal(got[key], want[key]), (fam, kind, key)
    # the unbounded status families keep their flags under infinite bounds
    for name in pc.STATUS_FAMILIES:
        f = pc.status_family(name)
        want = pc.restated(f["kind"], f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
        got = bc.restated_bounded(f["kind"], f["D"], f["E"], f["R"], None, None, f["S2"], f["ips"], f["c"], f["max_iter"])
        for key in ("eta", "n_iter", "status", "value"):
            assert np.array_equal(got[key], want[key]), (name, key)


def check_status_family(name, f, got):
    """what a status family has to show, on the host and on the device"""
    st = got["status"]
    T, K = st.shape
    J = got["eta"].shape[2]
    lo, hi = bc.full_bounds(f["lower"], f["upper"], K, J)
    assert np.all(np.isfinite(got["value"])), name
    if name in ("bad", "bad_nan"):
        assert np.all(st[:, 1] == bc.BAD_BOUNDS) and not st[:, [0, 2]].any(), st
        assert not got["eta"][:, 1].any() and not got["n_iter"][:, 1].any()
        assert np.array_equal(got["value"][:, 1], pc.value(f["kind"], f["D"], f["E"], f["R"], f["S2"],
                                                           np.zeros((T, K, J)), f["ips"], f["c"])[:, 1])
        assert got["n_iter"][:, [0, 2]].all()
    elif name == "start_clamped":
        assert not st.any()
        assert np.all(got["eta"] >= lo[None]) and np.all(got["eta"] <= hi[None])
        # 0 is outside the box: every pair ends at a point the box allows, most of them on the edge nearest to 0
        assert np.all(got["eta"][:, :, 0] >= 0.05) and np.all(got["eta"][:, :, 1] <= -0.02)
        assert np.any(got["eta"][:, :, 0] == 0.05) and np.any(got["eta"][:, :, 0] > 0.05)
    elif name == "posdef_pinned":
        assert not st.any() and np.all(got["eta"][:, :, 2:] == 0.0) and np.all(got["eta"][:, :, :2] != 0.0)
    elif name == "posdef":
        assert np.all(st == pc.NOT_POSDEF)
    elif name == "maxiter":
        assert np.all(st == pc.NOT_CONVERGED) and np.all(got["n_iter"] == 1)
    elif name == "start":
        assert np.all(st[:, 1] == pc.START_OUTSIDE) and not st[:, [0, 2]].any(), st
        assert not got["eta"][:, 1].any() and not got["n_iter"][:, 1].any()
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name", bc.STATUS_FAMILIES)
def test_status_families(name):
    f = bc.status_family(name)
    got = bc.restated_bounded(f["kind"], f["D"], f["E"], f["R"], f["lower"], f["upper"], f["S2"], f["ips"], f["c"],
                              f["max_iter"])
    check_status_family(name, f, got)
    if name == "posdef":
        want = pc.restated(f["kind"], f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
        assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["value"], want["value"])


# ------------------------------------------------------------- the kernel's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through the bounded solver of profile_device.hpp as a lane of the kernel drives it:
// seven int64 (kind, T, K, B, J, shared response, max_iter), then D [T][B], E and S2 [K][B], R [K or 1][J][B],
// ips [J], c [K][J], lo [K][J], hi [K][J]; per case value [T][K], eta [T][K][J], then n_iter and status as doubles
#include "profile_device.hpp"
#include <stdio.h>
#include <vector>
using namespace pisa;
struct Case {
    int64_t kind, T, K, B, J, shared, max_iter;
    std::vector<double> D, E, S2, R, ips, c, lo, hi;
};
template <int KIND, int J>
static void run(const Case &q, FILE *out) {
    std::vector<double> value(q.T * q.K), eta(q.T * q.K * J), iters(q.T * q.K), status(q.T * q.K);
    for (int64_t t = 0; t < q.T; t++)
        for (int64_t k = 0; k < q.K; k++) {
            const double *d = &q.D[t * q.B], *e = &q.E[k * q.B], *s2 = &q.S2[k * q.B];
            const double *R = &q.R[q.shared ? 0 : k * J * q.B], *c = &q.c[k * J];
            const double *lo = &q.lo[k * J], *hi = &q.hi[k * J];
            PfState<J> st;
            pf_init_bounded<J>(st, lo, hi);
            double r[J];
            while (!st.done) {
                pf_sweep_begin<J>(st);
                for (int64_t b = 0; b < q.B; b++) {
                    for (int j = 0; j < J; j++) r[j] = R[j * q.B + b];
                    pf_bin<KIND, J>(st, d[b], e[b], s2[b], r);
                }
                pf_decide_bounded<KIND, J>(st, q.ips.data(), c, lo, hi, (int32_t)q.max_iter);
            }
            PfValue pv;
            pf_value_begin(pv);
            for (int64_t b = 0; b < q.B; b++) {
                for (int j = 0; j < J; j++) r[j] = R[j * q.B + b];
                pf_value_bin<KIND, J>(pv, st.eta, d[b], e[b], s2[b], r);
            }
            const int64_t o = t * q.K + k;
            value[o] = pf_value_end<KIND, J>(pv, st.eta, q.ips.data(), c);
            for (int j = 0; j < J; j++) eta[o * J + j] = st.eta[j];
            iters[o] = st.n_iter;
            status[o] = pf_status<J>(st);
        }
    fwrite(value.data(), 8, value.size(), out);
    fwrite(eta.data(), 8, eta.size(), out);
    fwrite(iters.data(), 8, iters.size(), out);
    fwrite(status.data(), 8, status.size(), out);
}
template <int KIND>
static void run_j(const Case &q, FILE *out) {
    switch (q.J) {
    case 1: return run<KIND, 1>(q, out);
    case 2: return run<KIND, 2>(q, out);
    case 3: return run<KIND, 3>(q, out);
    case 4: return run<KIND, 4>(q, out);
    case 5: return run<KIND, 5>(q, out);
    case 6: return run<KIND, 6>(q, out);
    case 7: return run<KIND, 7>(q, out);
    default: return run<KIND, 8>(q, out);
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
    int64_t head[7];
    int n_cases = 0;
    while (fread(head, 8, 7, in) == 7) {
        Case q;
        q.kind = head[0], q.T = head[1], q.K = head[2], q.B = head[3], q.J = head[4], q.shared = head[5];
        q.max_iter = head[6];
        if (q.J < 1 || q.J > PF_MAX_PARAMS) return 3;
        if (!take(in, q.D, q.T * q.B) || !take(in, q.E, q.K * q.B) || !take(in, q.S2, q.K * q.B) ||
            !take(in, q.R, (q.shared ? 1 : q.K) * q.J * q.B) || !take(in, q.ips, q.J) || !take(in, q.c, q.K * q.J) ||
            !take(in, q.lo, q.K * q.J) || !take(in, q.hi, q.K * q.J))
            return 3;
        switch (q.kind) {
        case PF_LLH: run_j<PF_LLH>(q, out); break;
        case PF_POISSON_LLH: run_j<PF_POISSON_LLH>(q, out); break;
        case PF_CHI2: run_j<PF_CHI2>(q, out); break;
        default: run_j<PF_MOD_CHI2>(q, out);
        }
        n_cases++;
    }
    fclose(out);
    printf("%d\n", n_cases);
    return 0;
}
"""


def test_the_kernel_source_on_the_host_equals_the_restatement(tmp_path):
    """csrc/profile_device.hpp with `pf_init_bounded` / `pf_decide_bounded` (what every lane of the bounded kernel
    runs) compiled with g++ under ASan + UBSan and run as a program of its own on the cases of the GPU test: eta,
    n_iter and status `==` the restatement's, every value of a gated case inside the device's gate of the exact
    reference, every value of a status family inside it around the exact value at the returned eta"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "profile_bounded_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = []
    for name, bx, shape in bc.gated_cases():
        f = pc.family(name, *shape)
        lower, upper = bc.box(bx, shape[1], shape[3])
        for kind in pc.KINDS:
            cases.append((name, bx, shape, dict(f, kind=kind, max_iter=pc.MAX_ITER, lower=lower, upper=upper)))
    for name in bc.STATUS_FAMILIES:
        cases.append((name, None, None, bc.status_family(name)))
    with open(tmp_path / "cases.bin", "wb") as fh:
        for _, _, _, f in cases:
            T, B = f["D"].shape
            K = f["E"].shape[0]
            J = f["R"].shape[-2]
            fh.write(np.array([pc.KINDS.index(f["kind"]), T, K, B, J, int(f["R"].ndim == 2), f["max_iter"]],
                              dtype=np.int64).tobytes())
            lo, hi = bc.full_bounds(f["lower"], f["upper"], K, J)
            for a in (f["D"], f["E"], f["S2"], f["R"], np.zeros(J) if f["ips"] is None else f["ips"],
                      np.zeros((K, J)) if f["c"] is None else f["c"], lo, hi):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert int(res.stdout) == len(cases)
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    worst = {k: 0.0 for k in pc.KINDS}
    for name, bx, shape, f in cases:
        T, K, J = f["D"].shape[0], f["E"].shape[0], f["R"].shape[-2]
        n = T * K
        value = got_all[at:at + n].reshape(T, K)
        eta = got_all[at + n:at + n + n * J].reshape(T, K, J)
        n_iter = got_all[at + n + n * J:at + 2 * n + n * J].reshape(T, K)
        status = got_all[at + 2 * n + n * J:at + 3 * n + n * J].reshape(T, K)
        at += 3 * n + n * J
        kind = f["kind"]
        what = "%s %s %s %s" % (name, bx, shape, kind)
        if shape is not None:
            want = _restated(name, bx, shape, kind)
        else:
            want = bc.solve_bounded(kind, f["D"], f["E"], f["R"], f["lower"], f["upper"], f["S2"], f["ips"], f["c"],
                                    f["max_iter"])
        assert np.array_equal(status, want["status"]), what
        assert np.array_equal(n_iter, want["n_iter"]), what
        assert np.array_equal(eta, want["eta"]), what
        if shape is not None:
            ex = bc.exact_bounded(name, bx, kind, *shape)
            worst[kind] = max(worst[kind], ec.check(value, ex["value"], ex["scale"], bc.g_of(kind), what))
        else:
            val, scale = pc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], eta.astype(np.longdouble), f["ips"],
                                        f["c"])
            ec.check(value, val, scale, bc.g_of(kind), what)
    assert at == got_all.size
    print("the header on the host: worst ratios %s" % worst)


# --------------------------------------------------------------------------- the ensemble's plumbing
class _Solver(bc.NumpyBoundedProfileSolver):
    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        self.calls.append(("draw", int(n_trials), int(stream), int(first_trial)))
        return fc.block(mu, n_trials, seed, stream, first_trial)[0]


class _OldSolver(pc.NumpyProfileSolver):
    """a solver from before the bounds existed: its profiled methods take no lower / upper"""

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        return fc.block(mu, n_trials, seed, stream, first_trial)[0]


def _toy(metric, lower=None, upper=None):
    """the toy grid of tests/test_host_profiled.py (a normalisation with a 10 % Gaussian prior 0.05 above its mean,
    and a free tilt) with a box on the displacements"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    K, B = hist.shape
    x = np.linspace(-1.0, 1.0, B)
    R = np.stack([hist, hist * x[None, :]], axis=1)
    ips = np.array([10.0, 0.0])
    center = np.tile(np.array([[0.05, 0.0]]), (K, 1))
    share = (ips[0] * 0.05) ** 2 * (1.0 if metric in ("chi2", "mod_chi2") else -0.5)
    prior_at_point = np.full(K, share)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty + prior_at_point, metric)
    resp = en.NuisanceResponse(("norm", "tilt"), R, ips, center, prior_at_point, np.full((K, 2), [1.0, 0.0]),
                               lower=lower, upper=upper)
    return grid, resp, penalty


@pytest.mark.parametrize("metric", ("llh", "chi2", "mod_chi2"))
def test_bounded_distances_lie_between_the_unprofiled_and_the_profiled_ones(metric):
    from pisa_amd.analysis import ensemble as en

    K = 9
    # the tilt's range is so narrow that it binds for part of the trials; the normalisation's does not bind at all
    lower = np.tile(np.array([[-0.5, -0.004]]), (K, 1))
    upper = np.array([0.5, 0.006])
    grid, resp, other = _toy(metric, lower, upper)
    _, free, _ = _toy(metric)
    _, pinned, _ = _toy(metric, np.zeros(2), np.zeros(2))
    assert resp.bounded and not free.bounded and resp.lower.shape == resp.upper.shape == (K, 2)
    solver = _Solver()
    data = en.pseudo_data(grid, 4, 40, 3)
    m = en.metric_matrix(data, grid, metric, True, solver, resp)
    full = bc.restated_bounded(metric, data, grid.hist, resp.response, resp.lower, resp.upper, grid.sigma2_for(metric),
                               resp.inv_prior_sigma, resp.center)
    assert not full["status"].any() and np.array_equal(m, full["value"] + other[None, :])
    # values + eta inside the range for every trial, some exactly on the edge, some inside
    tilt = resp.values[None, :, 1] + full["eta"][:, :, 1]
    assert np.all(tilt >= -0.004) and np.all(tilt <= 0.006)
    assert np.any(tilt == -0.004) and np.any(tilt == 0.006) and np.any((tilt > -0.004) & (tilt < 0.006))
    assert np.all(np.abs(full["eta"][:, :, 0]) < 0.5)
    # a smaller feasible set cannot fit better: unbounded >= bounded >= pinned for the llh kinds, <= for the chi2 kinds
    m_free = en.metric_matrix(data, grid, metric, True, solver, free)
    m_pin = en.metric_matrix(data, grid, metric, True, solver, pinned)
    plain = en.metric_matrix(data, grid, metric, True, solver)
    scale = ec.scale_fp64(metric, data, grid.hist, grid.sigma2_for(metric))
    tol = bc.g_of(metric) * pc.EPS * (scale + np.abs(plain))
    sign = 1.0 if metric in ec.LLH_KINDS else -1.0
    assert np.all(sign * (m_free - m) >= -tol) and np.any(sign * (m_free - m) > 1e-3)
    assert np.all(sign * (m - m_pin) >= -tol) and np.any(sign * (m - m_pin) > 1e-3)
    # pinned at 0 IS the unprofiled entry
    assert np.all(np.abs(m_pin - plain) <= 4 * pc.EPS * (scale + np.abs(plain)))
    # so the bounded profiled distance is not smaller than the unbounded one where the best point is shared ...
    for k0 in (0, 4):
        d_b, info = en.delta_metric(data, grid, metric, k0, solver, resp, return_info=True)
        red = pc.reduce_profiled(metric, full, other, k0)
        assert np.array_equal(d_b, sign * (red["best"] - red["at"])) and np.all(d_b >= 0) and info["flagged"] == 0
        assert np.array_equal(info["eta_at"], red["eta_at"]) and np.array_equal(info["arg"], red["arg"])
    calls = [c for c in solver.calls if c[0].startswith("profiled")]
    assert calls and all(c[-1] for c in calls[:1])


def test_feldman_cousins_with_a_bounded_response_does_not_depend_on_chunks():
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    grid, resp, _ = _toy(metric, np.array([-0.5, -0.004]), np.array([0.5, 0.006]))
    _, free, _ = _toy(metric)
    T, cl, seed = 48, (0.6827, 0.90), 1
    solver = _Solver()
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device", response=resp)
    assert crit.shape == (9, 2) and np.all(crit >= 0) and not info["flagged"].any()
    assert [c[0] for c in solver.calls[:2]] == ["draw", "profiled_best"] and solver.calls[1][-1] is True
    got, _ = en.feldman_cousins(grid, metric, T, cl, seed, solver=_Solver(), generator="device",
                                chunk_bytes=7 * 8 * grid.n_bins, response=resp)
    assert np.array_equal(got, crit)
    for k0 in (0, 5):
        data = en.pseudo_data(grid, k0, T, seed, generator="device", solver=solver)
        assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver, resp), cl), crit[k0])
    unbounded, _ = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device", response=free)
    assert not np.array_equal(unbounded, crit)
    observed = en.pseudo_data(grid, 4, 1, 9)
    m = en.metric_matrix(observed, grid, metric, True, solver, resp)[0]
    assert np.array_equal(en.accepted(observed, grid, metric, crit[:, 1], solver, resp), m.max() - m <= crit[:, 1])


def test_bad_bounds_are_refused_and_an_unbounded_response_passes_no_new_keyword():
    from pisa_amd.analysis import ensemble as en

    metric = "mod_chi2"
    grid, free, _ = _toy(metric)
    R = free.response
    for kw, match in ((dict(lower=[0.1, 0.0], upper=[0.0, 1.0]), "lower > upper"),
                      (dict(lower=[np.nan, 0.0]), "NaN"), (dict(upper=[[0.0, np.nan]] * 9), "NaN"),
                      (dict(lower=np.zeros(3)), r"lower is \[2\]"), (dict(upper=np.zeros((9, 3))), r"upper is \[2\]"),
                      (dict(lower=np.zeros((4, 2))), r"lower is \[2\]")):
        with pytest.raises(ValueError, match=match):
            en.NuisanceResponse(("norm", "tilt"), R, **kw)
    # one side alone, -inf / +inf, and a pinned parameter are all fine
    assert en.NuisanceResponse(("norm", "tilt"), R, lower=[-np.inf, 0.0]).bounded
    assert en.NuisanceResponse(("norm", "tilt"), R, lower=[0.0, 0.0], upper=[0.0, np.inf]).bounded
    data = en.pseudo_data(grid, 2, 16, 5)
    # an unbounded response: the old protocol, on a solver that has never heard of bounds and on the new one
    old, new = _OldSolver(), _Solver()
    want = en.metric_matrix(data, grid, metric, True, old, free)
    assert np.array_equal(en.metric_matrix(data, grid, metric, True, new, free), want)
    assert np.array_equal(en.delta_metric(data, grid, metric, 2, old, free), en.delta_metric(data, grid, metric, 2, new, free))
    crit, _ = en.feldman_cousins(grid, metric, 8, random_state=1, true_points=[2], solver=old, generator="device",
                                 response=free)
    assert crit.shape == (1, 2)
    assert en.accepted(data[:1], grid, metric, np.zeros(9), old, free).shape == (9,)
    assert all(c[-1] is False for c in new.calls if c[0].startswith("profiled"))
    assert free.bounds() == {}
    # a bounded response on that solver is refused by every driver
    _, resp, _ = _toy(metric, [-0.5, -0.004], [0.5, 0.006])
    for call in (lambda: en.metric_matrix(data, grid, metric, True, old, resp),
                 lambda: en.delta_metric(data, grid, metric, 2, old, resp),
                 lambda: en.feldman_cousins(grid, metric, 8, random_state=1, solver=old, response=resp),
                 lambda: en.accepted(data[:1], grid, metric, np.zeros(9), old, resp)):
        with pytest.raises(ValueError, match="lower= and upper="):
            call()
    # bounds of another grid
    other = en.NuisanceResponse(("norm", "tilt"), R[0], lower=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="do not belong"):
        en.metric_matrix(data, grid, metric, True, new, other)
