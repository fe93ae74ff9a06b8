"""The profiled trial ensembles without a GPU: the numpy restatement of the solver (tests/profile_cases.py) against the
exact reference on every gated family and shape (held to G_HOST = 2, G_REF measured again and held against the recorded
figures, every pair with status 0 in both), the closed forms of `norm` and `prior`, the flags of the status families,
the solver's own source (csrc/profile_device.hpp) compiled for the host under the sanitizers against the restatement,
and the `response=` paths of pisa_amd/analysis/ensemble.py with a numpy solver.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import fluctuate_cases as fc
from tests import profile_cases as pc

_WORST = {}


def _worst(kind):
    """(worst ratio of the restatement, where, most Newton steps) over every gated case; every pair of every case has
    status 0 in the exact reference and in the restatement"""
    if kind not in _WORST:
        worst, where, steps = 0.0, None, 0
        for name, shape in pc.gated_cases():
            f = pc.family(name, *shape)
            ex = pc.exact(name, kind, *shape)
            assert not ex["status"].any(), (name, shape, kind, np.unique(ex["status"]))
            got = pc.restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"])
            assert not got["status"].any(), (name, shape, kind, np.unique(got["status"]))
            r = ec.check(got["value"], ex["value"], ex["scale"], pc.G_HOST, "%s %s %s" % (name, shape, kind))
            steps = max(steps, int(got["n_iter"].max()))
            if r > worst:
                worst, where = r, (name, shape)
        _WORST[kind] = (worst, where, steps)
    return _WORST[kind]


@pytest.mark.parametrize("kind", pc.KINDS)
def test_restatement_within_the_host_gate_and_g_ref_is_the_measured_worst_ratio(kind):
    worst, where, steps = _worst(kind)
    print("%s: measured %.4f at %s, recorded %.2f, at most %d Newton steps" % (kind, worst, where, pc.G_REF[kind], steps))
    assert worst <= pc.G_HOST
    assert worst <= pc.G_REF[kind] <= worst + 0.02
    assert pc.g_of(kind) == pc.mc.KERNEL_FACTOR * max(1.0, pc.G_REF[kind])
    assert steps <= pc.MAX_ITER // 2
    assert set(pc.G_REF) == set(pc.KINDS)


def test_every_size_of_the_issue_is_among_the_shapes():
    shapes = pc.SHAPES
    assert {s[0] for s in shapes} == {1, 63, 64, 65, 257} and {s[1] for s in shapes} == {1, 3, 17}
    assert {s[2] for s in shapes} == {1, 3, 64, 65, 130} and {s[3] for s in shapes} == {1, 2, 5, 8}
    assert pc.STRIP_SHAPE == (1000, 5, 8, 2) and pc.TILE_SHAPE == (64, 300, 12, 3)
    for name in pc.GATED:
        assert len(pc.shapes_of(name)) >= 3, name


def test_closed_forms_of_norm_and_prior():
    for shape in pc.shapes_of("norm"):
        f = pc.family("norm", *shape)
        got = pc.solve("llh", f["D"], f["E"], f["R"], f["S2"])
        want = f["D"].sum(axis=1)[:, None] / f["E"].sum(axis=1)[None, :] - 1.0
        assert np.all(np.abs(got["eta"][:, :, 0] - want) <= 64 * pc.EPS * (1.0 + np.abs(want))), shape
    for shape in pc.shapes_of("prior"):
        f = pc.family("prior", *shape)
        for kind in ("llh", "chi2"):
            got = pc.solve(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"])
            # the parameter without response sits at its prior mean: eta = -c
            assert np.all(np.abs(got["eta"][:, :, -1] + f["c"][None, :, -1]) <= 4 * pc.EPS), (shape, kind)
    # asimov: the pair's own template is fitted back to eta_0 and the value is near 0
    for shape in [s for s in pc.shapes_of("asimov") if s[2] >= 3][:4]:
        f = pc.family("asimov", *shape)
        T, K = shape[:2]
        got = pc.restated("chi2", f["D"], f["E"], f["R"], f["S2"])
        own = np.arange(T) % K
        assert np.all(np.abs(got["eta"][np.arange(T), own] - f["eta0"]) <= 1e-9 * (1 + np.abs(f["eta0"]))), shape
        assert np.all(np.abs(got["value"][np.arange(T), own]) <= 1e-18 * f["E"].sum()), shape


def test_low_needs_the_damping_and_far_does_not_stop_early():
    f = pc.family("low", 65, 1, 3, 1)
    got = pc.solve("llh", f["D"], f["E"], f["R"], f["S2"])
    # D = E / 4: the full first step is -3 (mu = -2 E), accepted at a quarter of it
    assert not got["status"].any() and np.allclose(got["eta"], -0.75, rtol=1e-12)
    f = pc.family("far", 65, 1, 3, 1)
    got = pc.solve("llh", f["D"], f["E"], f["R"], f["S2"])
    assert not got["status"].any() and np.allclose(got["eta"], 2.0, rtol=1e-12) and got["n_iter"].min() >= 4


WANT_FLAGS = {"posdef": pc.NOT_POSDEF, "start": pc.START_OUTSIDE, "maxiter": pc.NOT_CONVERGED}


def test_status_families():
    for name in pc.STATUS_FAMILIES:
        f = pc.status_family(name)
        got = pc.restated(f["kind"], f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
        st = got["status"]
        assert np.all(np.isfinite(got["value"])), name
        if name == "boundary":
            # the rows without data end cut by the domain, the others are clean
            assert np.all(st[::2] & pc.BOUNDARY) and not st[1::2].any(), st
            assert np.all(got["eta"][::2] > -1.0) and np.all(got["eta"][::2] < -0.5)
        elif name == "start":
            assert np.all(st[:, 1] == pc.START_OUTSIDE) and not st[:, [0, 2]].any(), st
            assert not got["eta"][:, 1].any() and not got["n_iter"][:, 1].any()
        else:
            assert np.all(st == WANT_FLAGS[name]), (name, st)
        if name == "maxiter":
            assert np.all(got["n_iter"] == 1)


# ------------------------------------------------------------- the kernel's own source, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through the solver of profile_device.hpp as a lane of the kernel drives it: nine
// int64 (kind, T, K, B, J, shared response, max_iter, priors given, centres given), then D [T][B], E and S2 [K][B],
// R [K or 1][J][B], ips [J], c [K][J]; per case value [T][K], eta [T][K][J], then n_iter and status as doubles
#include "profile_device.hpp"
#include <stdio.h>
#include <vector>
using namespace pisa;
struct Case {
    int64_t kind, T, K, B, J, shared, max_iter;
    std::vector<double> D, E, S2, R, ips, c;
};
template <int KIND, int J>
static void run(const Case &q, FILE *out) {
    std::vector<double> value(q.T * q.K), eta(q.T * q.K * J), iters(q.T * q.K), status(q.T * q.K);
    for (int64_t t = 0; t < q.T; t++)
        for (int64_t k = 0; k < q.K; k++) {
            const double *d = &q.D[t * q.B], *e = &q.E[k * q.B], *s2 = &q.S2[k * q.B];
            const double *R = &q.R[q.shared ? 0 : k * J * q.B], *c = &q.c[k * J];
            PfState<J> st;
            pf_init<J>(st);
            double r[J];
            while (!st.done) {
                pf_sweep_begin<J>(st);
                for (int64_t b = 0; b < q.B; b++) {
                    for (int j = 0; j < J; j++) r[j] = R[j * q.B + b];
                    pf_bin<KIND, J>(st, d[b], e[b], s2[b], r);
                }
                pf_decide<KIND, J>(st, q.ips.data(), c, (int32_t)q.max_iter);
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
            !take(in, q.R, (q.shared ? 1 : q.K) * q.J * q.B) || !take(in, q.ips, q.J) || !take(in, q.c, q.K * q.J))
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
    """csrc/profile_device.hpp (the sweep over the bins, the Cholesky factor, the line search and the final value:
    what every lane of the kernel runs) compiled with g++ under ASan + UBSan and run as a program of its own on the
    cases of the GPU test: eta, n_iter and status `==` the restatement's, every value of a gated case inside the
    device's gate of the exact reference, every value of a status family inside it around the exact value at the
    returned eta"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "main.cpp", tmp_path / "profile_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(root, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    cases = []
    for name, shape in pc.gated_cases():
        f = pc.family(name, *shape)
        for kind in pc.KINDS:
            cases.append((name, shape, dict(f, kind=kind, max_iter=pc.MAX_ITER)))
    for name in pc.STATUS_FAMILIES:
        cases.append((name, None, pc.status_family(name)))
    with open(tmp_path / "cases.bin", "wb") as fh:
        for _, _, f in cases:
            T, B = f["D"].shape
            K = f["E"].shape[0]
            J = f["R"].shape[-2]
            fh.write(np.array([pc.KINDS.index(f["kind"]), T, K, B, J, int(f["R"].ndim == 2), f["max_iter"]],
                              dtype=np.int64).tobytes())
            for a in (f["D"], f["E"], f["S2"], f["R"], np.zeros(J) if f["ips"] is None else f["ips"],
                      np.zeros((K, J)) if f["c"] is None else f["c"]):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert int(res.stdout) == len(cases)
    got_all = np.fromfile(tmp_path / "out.bin")
    at = 0
    worst = {k: 0.0 for k in pc.KINDS}
    for name, shape, f in cases:
        T, K, J = f["D"].shape[0], f["E"].shape[0], f["R"].shape[-2]
        n = T * K
        value = got_all[at:at + n].reshape(T, K)
        eta = got_all[at + n:at + n + n * J].reshape(T, K, J)
        n_iter = got_all[at + n + n * J:at + 2 * n + n * J].reshape(T, K)
        status = got_all[at + 2 * n + n * J:at + 3 * n + n * J].reshape(T, K)
        at += 3 * n + n * J
        kind = f["kind"]
        want = pc.solve(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], f["max_iter"])
        what = "%s %s %s" % (name, shape, kind)
        assert np.array_equal(status, want["status"]), what
        assert np.array_equal(n_iter, want["n_iter"]), what
        assert np.array_equal(eta, want["eta"]), what
        if shape is not None:
            ex = pc.exact(name, kind, *shape)
            worst[kind] = max(worst[kind], ec.check(value, ex["value"], ex["scale"], pc.g_of(kind), what))
        else:
            val, scale = pc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], eta.astype(np.longdouble), f["ips"],
                                        f["c"])
            ec.check(value, val, scale, pc.g_of(kind), what)
    assert at == got_all.size
    print("the header on the host: worst ratios %s" % worst)


# --------------------------------------------------------------------------- the ensemble's plumbing
class _Solver(pc.NumpyProfileSolver):
    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        self.calls.append(("draw", int(n_trials), int(stream), int(first_trial)))
        return fc.block(mu, n_trials, seed, stream, first_trial)[0]


def _toy(metric):
    """the toy grid of tests/ensemble_cases.py with two nuisance parameters that are not dimensions of the grid: a
    normalisation with a 10 % Gaussian prior that sits 0.05 above its mean at every point, and a free tilt"""
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
    resp = en.NuisanceResponse(("norm", "tilt"), R, ips, center, prior_at_point, np.zeros((K, 2)))
    return grid, resp, penalty


@pytest.mark.parametrize("metric", ("llh", "chi2", "mod_chi2"))
def test_no_prior_is_counted_twice_and_profiling_is_no_worse(metric):
    from pisa_amd.analysis import ensemble as en

    grid, resp, other = _toy(metric)
    solver = _Solver()
    data = en.pseudo_data(grid, 4, 40, 3)
    full = pc.restated(metric, data, grid.hist, resp.response, grid.sigma2_for(metric), resp.inv_prior_sigma, resp.center)
    assert not full["status"].any()
    # the matrix: the fit's value (which holds the prior at the FITTED value) + the penalty of the other parameters
    m = en.metric_matrix(data, grid, metric, True, solver, resp)
    assert np.array_equal(m, full["value"] + other[None, :])
    assert np.array_equal(en.metric_matrix(data, grid, metric, False, solver, resp), full["value"])
    # at eta = 0 the profiled entry IS the unprofiled one: the named prior's share stands once on either side
    plain = en.metric_matrix(data, grid, metric, True, solver)
    at_zero = pc.value(metric, data, grid.hist, resp.response, grid.sigma2_for(metric), np.zeros(full["eta"].shape),
                       resp.inv_prior_sigma, resp.center) + other[None, :]
    scale = ec.scale_fp64(metric, data, grid.hist, grid.sigma2_for(metric))
    assert np.all(np.abs(at_zero - plain) <= 4 * pc.EPS * (scale + np.abs(plain)))
    # so the fit can only improve every entry, and with it `best` and `at` of every trial
    sign = 1.0 if metric in ec.LLH_KINDS else -1.0
    tol = pc.g_of(metric) * pc.EPS * (scale + np.abs(plain))
    assert np.all(sign * (m - plain) >= -tol)
    assert np.any(sign * (m - plain) > 1e-3)
    for k0 in (0, 4):
        b0, _, a0 = solver.best(metric, data, grid.hist, grid.sigma2_for(metric), grid.penalty, k0)
        delta, info = en.delta_metric(data, grid, metric, k0, solver, resp, return_info=True)
        red = pc.reduce_profiled(metric, full, other, k0)
        assert np.all(sign * (red["best"] - b0) >= -tol.max()) and np.all(sign * (red["at"] - a0) >= -tol.max())
        assert np.array_equal(delta, sign * (red["best"] - red["at"])) and np.all(delta >= 0)
        assert np.array_equal(delta, en.delta_metric(data, grid, metric, k0, solver, resp))
        assert info["flagged"] == 0 and np.array_equal(info["arg"], red["arg"])
        assert np.array_equal(info["eta_best"], red["eta_best"]) and np.array_equal(info["eta_at"], red["eta_at"])
        assert info["eta_at"].shape == (40, 2)


def test_feldman_cousins_with_a_response_does_not_depend_on_chunks_or_on_the_subset():
    from pisa_amd.analysis import ensemble as en

    metric = "llh"
    grid, resp, _ = _toy(metric)
    T, cl, seed = 48, (0.6827, 0.90), 1
    solver = _Solver()
    crit, info = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device", response=resp)
    assert crit.shape == (9, 2) and np.all(crit >= 0) and info["flagged"].shape == (9,) and not info["flagged"].any()
    assert [c[0] for c in solver.calls[:2]] == ["draw", "profiled_best"]
    for k0 in (0, 5):
        data = en.pseudo_data(grid, k0, T, seed, generator="device", solver=solver)
        assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver, resp), cl), crit[k0])
    got, _ = en.feldman_cousins(grid, metric, T, cl, seed, solver=_Solver(), generator="device",
                                chunk_bytes=7 * 8 * grid.n_bins, response=resp)
    assert np.array_equal(got, crit)
    sub, sub_info = en.feldman_cousins(grid, metric, T, cl, seed, true_points=[7, 2], solver=solver,
                                       generator="device", response=resp)
    assert np.array_equal(sub, crit[[7, 2]]) and sub_info["flagged"].shape == (2,)
    host, _ = en.feldman_cousins(grid, metric, T, cl, seed, true_points=[3], solver=solver, response=resp)
    data = en.pseudo_data(grid, 3, T, np.random.RandomState([seed, 3]))
    assert np.array_equal(host[0], en.critical_values(en.delta_metric(data, grid, metric, 3, solver, resp), cl))
    # profiling two more directions brings every point closer to the data: smaller critical values on the whole
    plain = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver, generator="device")
    assert isinstance(plain, np.ndarray) and crit.mean() < plain.mean()
    # `accepted` with the response: the row of the profiled matrix against its best
    observed = en.pseudo_data(grid, 4, 1, 9)
    m = en.metric_matrix(observed, grid, metric, True, solver, resp)[0]
    assert np.array_equal(en.accepted(observed, grid, metric, crit[:, 1], solver, resp), m.max() - m <= crit[:, 1])


def test_calls_without_a_response_are_unchanged_and_bad_responses_are_refused():
    from pisa_amd.analysis import ensemble as en

    metric = "mod_chi2"
    grid, resp, _ = _toy(metric)
    data = en.pseudo_data(grid, 2, 16, 5)
    plain, prof = ec.NumpySolver(), _Solver()
    want = ec.direct_form(metric, data, grid.hist, grid.sumw2) + grid.penalty[None, :]
    for solver in (plain, prof):
        assert np.array_equal(en.metric_matrix(data, grid, metric, True, solver), want)
        assert np.array_equal(en.delta_metric(data, grid, metric, 2, solver), want[:, 2] - want.min(axis=1))
        crit = en.feldman_cousins(grid, metric, 8, random_state=1, true_points=[2], solver=solver)
        assert isinstance(crit, np.ndarray) and crit.shape == (1, 2)
    assert not any(c[0].startswith("profiled") for c in prof.calls)
    # a solver without the profiled methods
    for call in (lambda: en.metric_matrix(data, grid, metric, True, plain, resp),
                 lambda: en.delta_metric(data, grid, metric, 2, plain, resp),
                 lambda: en.feldman_cousins(grid, metric, 8, random_state=1, solver=plain, response=resp),
                 lambda: en.accepted(data[:1], grid, metric, np.zeros(9), plain, resp)):
        with pytest.raises(ValueError, match="profiled_matrix"):
            call()
    with pytest.raises(ValueError, match="return_info"):
        en.delta_metric(data, grid, metric, 2, prof, return_info=True)
    # responses that do not fit
    with pytest.raises(ValueError, match="1 to 8"):
        en.NuisanceResponse(tuple("abcdefghi"), np.zeros((9, 9, 24)))
    with pytest.raises(ValueError, match="response is"):
        en.NuisanceResponse(("a", "b"), np.zeros((9, 3, 24)))
    with pytest.raises(ValueError, match="inv_prior_sigma"):
        en.NuisanceResponse(("a",), np.zeros((9, 1, 24)), [-1.0])
    other = en.NuisanceResponse(("a",), np.zeros((4, 1, 24)))
    with pytest.raises(ValueError, match="does not belong"):
        en.metric_matrix(data, grid, metric, True, prof, other)
    # the shared [J, B] form is taken as it is
    shared = en.NuisanceResponse(("a",), np.asarray(grid.hist[4:5]))
    assert en.metric_matrix(data, grid, metric, True, prof, shared).shape == (16, 9)
