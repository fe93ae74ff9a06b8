"""The nuisance-posterior sampler without a GPU (csrc/posterior_device.hpp, tests/posterior_cases.py; DESIGN.md §4,
"Trial ensembles: the nuisance posterior"): the header compiled for the host against the numpy restatement, the seeds of
the GPU shapes, the statistical validity of the definition on exactly known targets, and the argument checks of the entry
points, which come before any device access."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import posterior_cases as po
from tests import profile_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the restatement itself
def test_phi_of_the_restatement_is_the_solvers():
    """`posterior_cases.logp` forms Phi as `profile_cases._sweep` does at a trial point: the same bits, so lp is -Phi
    (or -Phi / 2) of the profile solver's objective"""
    for kind in po.KINDS:
        f = po.case(kind, 3, 65, 3, 8, "none")
        rs = np.random.RandomState(5)
        eta = 0.3 * rs.randn(3, 4, 3)
        lp, _, _ = po.logp(f["pr"], eta)
        for p in range(3):
            t, k = f["t_of"][p], f["k_of"][p]
            inside, s, c, _, _, _ = pc._sweep(kind, f["D"][t:t + 1], f["E"][k:k + 1], f["S2"][k:k + 1],
                                              f["R"][k:k + 1], eta[p, 0][None, None, :])
            Phi = (s + c)[0, 0]
            for j in range(3):
                pj = f["ips"][j] * (eta[p, 0, j] + f["c"][k, j])
                Phi = Phi + pc.w_of(kind) * (pj * pj)
            assert inside.all()
            assert lp[p, 0] == (-Phi if kind in po.LLH_KINDS else -0.5 * Phi), (kind, p)


def test_log_density_is_minus_infinity_outside_box_and_domain():
    f = po.case("llh", 1, 5, 2, 4, "box")
    eta = np.zeros((1, 3, 2))
    eta[0, 1, 0] = 1.6                    # outside the box (the upper bound is 1.5)
    eta[0, 2, 0] = -1e3                   # inside no box and outside the domain
    lp, _, _ = po.logp(f["pr"], eta)
    assert np.isfinite(lp[0, 0]) and lp[0, 1] == -np.inf and lp[0, 2] == -np.inf


def test_kept_steps_and_their_count():
    from pisa_amd import kernels

    for first, n, keep_from, thin in ((0, 10, 0, 1), (3, 10, 0, 4), (3, 10, 5, 3), (20, 7, 5, 4), (0, 5, 9, 2),
                                      (2 ** 32 - 64, 64, 2 ** 32 - 10, 3)):
        assert kernels.posterior_n_keep(first, n, keep_from, thin) == po.n_keep_of(first, n, keep_from, thin)


# ------------------------------------------------------------- the header, compiled for the host
_HOST_MAIN = r"""
// every case of the input file through posterior_device.hpp as a lane of the kernel drives it.  Per case twelve int64
// (kind, P, B, J, W, n_steps, first_step, keep_from, thin, stream, key word 0, key word 1), then d, e, s2 [P][B],
// R [P][J][B], ips [J], c, lo, hi [P][J], x0 [P][W][J], chain ids [P] (as doubles); written: chain, logp, accepted,
// end, status (as doubles)
#include "posterior_device.hpp"
#include <stdio.h>
#include <vector>
using namespace pisa;
struct Case {
    int64_t kind, P, B, J, W, n_steps, first, keep_from, thin, stream, k0, k1;
    std::vector<double> d, e, s2, R, ips, c, lo, hi, x0, ids;
};
template <int KIND, int J>
static double lp_of(const Case &q, int64_t p, const double *eta) {
    PsSweep sw;
    ps_begin(sw);
    double r[J];
    for (int64_t b = 0; b < q.B; b++) {
        for (int j = 0; j < J; j++) r[j] = q.R[(p * J + j) * q.B + b];
        ps_bin<KIND, J>(sw, eta, q.d[p * q.B + b], q.e[p * q.B + b], q.s2[p * q.B + b], r);
    }
    return ps_end<KIND, J>(sw, eta, q.ips.data(), &q.c[p * J], &q.lo[p * J], &q.hi[p * J]);
}
template <int KIND, int J>
static void run(const Case &q, FILE *out) {
    const int64_t W = q.W, H = W / 2, n_keep = ps_n_keep(q.first, q.n_steps, q.keep_from, q.thin);
    std::vector<double> chain(q.P * n_keep * W * J), logp(q.P * n_keep * W), acc(q.P * W), end(q.P * W * J), status(q.P);
    for (int64_t p = 0; p < q.P; p++) {
        std::vector<double> x(q.x0.begin() + p * W * J, q.x0.begin() + (p + 1) * W * J), lp(W);
        int n_free;
        int st = ps_box<J>(&q.lo[p * J], &q.hi[p * J], n_free) ? 0 : PF_BAD_BOUNDS;
        if (!st)
            for (int64_t w = 0; w < W; w++) {
                lp[w] = lp_of<KIND, J>(q, p, &x[w * J]);
                if (lp[w] != lp[w] || lp[w] == -INFINITY) st = PF_START_OUTSIDE;
            }
        std::vector<double> n_acc(W, 0.0);
        int64_t i_keep = 0;
        for (int64_t i = 0; i < q.n_steps; i++) {
            const int64_t s = q.first + i;
            for (int half = 0; half < 2 && !st; half++)
                for (int64_t h = 0; h < H; h++) {
                    const int64_t w = half * H + h;
                    double u_z, u_p, u_a, y[J];
                    ps_uniforms((uint32_t)w, (uint32_t)s, (uint32_t)q.stream, (uint32_t)q.ids[p], (uint32_t)q.k0,
                                (uint32_t)q.k1, u_z, u_p, u_a);
                    const double z = ps_stretch(u_z);
                    const int64_t partner = (1 - half) * H + ps_partner(u_p, (int)H);
                    ps_propose<J>(&x[w * J], &x[partner * J], z, y);
                    const double lp_y = lp_of<KIND, J>(q, p, y);
                    if (ps_accept(u_a, z, n_free, lp_y, lp[w])) {
                        for (int j = 0; j < J; j++) x[w * J + j] = y[j];
                        lp[w] = lp_y;
                        n_acc[w] += 1.0;
                    }
                }
            if (ps_kept(s, q.keep_from, q.thin)) {
                for (int64_t w = 0; w < W; w++) {
                    const int64_t o = (p * n_keep + i_keep) * W + w;
                    for (int j = 0; j < J; j++) chain[o * J + j] = st ? NAN : x[w * J + j];
                    logp[o] = st ? NAN : lp[w];
                }
                i_keep++;
            }
        }
        for (int64_t w = 0; w < W; w++) {
            acc[p * W + w] = n_acc[w];
            for (int j = 0; j < J; j++) end[(p * W + w) * J + j] = st ? NAN : x[w * J + j];
        }
        status[p] = st;
    }
    fwrite(chain.data(), 8, chain.size(), out);
    fwrite(logp.data(), 8, logp.size(), out);
    fwrite(acc.data(), 8, acc.size(), out);
    fwrite(end.data(), 8, end.size(), out);
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
    int64_t h[12];
    int n_cases = 0;
    while (fread(h, 8, 12, in) == 12) {
        Case q;
        q.kind = h[0], q.P = h[1], q.B = h[2], q.J = h[3], q.W = h[4], q.n_steps = h[5], q.first = h[6];
        q.keep_from = h[7], q.thin = h[8], q.stream = h[9], q.k0 = h[10], q.k1 = h[11];
        if (q.J < 1 || q.J > PF_MAX_PARAMS || q.W < 2 || q.W > PS_MAX_WALKERS || (q.W & 1)) return 3;
        if (!take(in, q.d, q.P * q.B) || !take(in, q.e, q.P * q.B) || !take(in, q.s2, q.P * q.B) ||
            !take(in, q.R, q.P * q.J * q.B) || !take(in, q.ips, q.J) || !take(in, q.c, q.P * q.J) ||
            !take(in, q.lo, q.P * q.J) || !take(in, q.hi, q.P * q.J) || !take(in, q.x0, q.P * q.W * q.J) ||
            !take(in, q.ids, q.P))
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


def _host_table():
    """(case, call arguments): the GPU shapes at a few steps, thinned and late-kept calls, and the status problems"""
    table = []
    for q in po.GPU_CASES:
        kind, P, B, J, W, bounds, n_steps, first = q
        if B * W > 20000:
            continue                                      # (the large rows: the GPU test's; the code is the same)
        f = po.case(kind, P, B, J, W, bounds)
        table.append((f["pr"], f["x0"], dict(n_steps=min(n_steps, 12), first_step=first, chain_id=np.arange(P) + 11,
                                             stream=3)))
    f = po.case("llh", 3, 9, 2, 8, "box")
    table.append((f["pr"], f["x0"], dict(n_steps=20, first_step=3, keep_from=6, thin=4, chain_id=np.arange(3),
                                         stream=1)))
    table.append(_status_case())
    return table


def _status_case():
    """problem 0 clean, 1 with a walker outside its box, 2 with lo > hi, 3 with a walker outside the domain, 4 clean"""
    f = po.case("poisson_llh", 5, 9, 2, 8, "box")
    pr = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in f["pr"].items()}
    x0 = np.array(f["x0"])
    x0[1, 3, 0] = 9.0
    pr["lo"][2, 1], pr["hi"][2, 1] = 1.0, -1.0
    pr["lo"][3], pr["hi"][3] = -np.inf, np.inf
    x0[3, 5, 0] = -1e4
    return pr, x0, dict(n_steps=6, first_step=0, chain_id=np.arange(5), stream=0)


def test_the_header_on_the_host_equals_the_restatement(tmp_path):
    """csrc/posterior_device.hpp (log-density, counters, move, acceptance, kept steps: what a lane of the kernel runs)
    compiled with g++ under ASan + UBSan into a program of its own and run on the case table: positions, accept
    counts, end states and status `==` the restatement's wherever it marks nothing (nothing is marked), every lp inside
    the window of a log within LOG_ULPS ulps (`==` for the chi2 kinds)"""
    src, exe = tmp_path / "main.cpp", tmp_path / "posterior_host"
    src.write_text(_HOST_MAIN)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pisa_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    table = _host_table()
    k0, k1 = po.key_of(po.SEED)
    with open(tmp_path / "cases.bin", "wb") as fh:
        for pr, x0, kw in table:
            P, W, J = x0.shape
            fh.write(np.array([po.KINDS.index(pr["kind"]), P, pr["d"].shape[1], J, W, kw["n_steps"], kw["first_step"],
                               kw.get("keep_from", 0), kw.get("thin", 1), kw["stream"], k0, k1],
                              dtype=np.int64).tobytes())
            for a in (pr["d"], pr["e"], pr["s2"], pr["R"], pr["ips"], pr["c"], pr["lo"], pr["hi"], x0,
                      kw["chain_id"]):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    res = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert int(res.stdout) == len(table)
    got = np.fromfile(tmp_path / "out.bin")
    at = 0
    for n, (pr, x0, kw) in enumerate(table):
        P, W, J = x0.shape
        want = po.sample(pr, x0, seed=po.SEED, **kw)
        assert want["n_marginal"] == 0 and want["n_edge"] == 0, n
        n_keep = want["chain"].shape[1]
        sizes = (P * n_keep * W * J, P * n_keep * W, P * W, P * W * J, P)
        chain, logp, acc, end, status = (got[at + sum(sizes[:i]):at + sum(sizes[:i + 1])] for i in range(5))
        at += sum(sizes)
        assert np.array_equal(status, want["status"].ravel()), n
        assert np.array_equal(chain.reshape(want["chain"].shape), want["chain"], equal_nan=True), n
        assert np.array_equal(end.reshape(want["end"].shape), want["end"], equal_nan=True), n
        assert np.array_equal(acc.reshape(P, W), want["accepted"]), n
        window = po.logp_window(pr["kind"], want["S"])
        live = ~np.isnan(want["logp"])
        assert np.array_equal(np.isnan(logp.reshape(want["logp"].shape)), ~live), n
        assert np.all(np.abs(logp.reshape(want["logp"].shape) - want["logp"])[live] <= window[live]), n
    assert at == got.size
    pr, x0, kw = table[-1]
    want = po.sample(pr, x0, seed=po.SEED, **kw)
    assert list(want["status"]) == [0, po.START_OUTSIDE, po.BAD_BOUNDS, po.START_OUTSIDE, 0]
    assert not want["accepted"][[1, 2, 3]].any() and want["accepted"][[0, 4]].any()


def test_the_seeds_of_the_gpu_shapes_mark_nothing():
    """no accept decision of a GPU case lies within the margin of its threshold and no proposal within it of an edge:
    the device must reproduce every position (another seed rather than a wider window)"""
    total = 0
    for q in po.GPU_CASES:
        _, want = po.gpu_want(q)
        assert want["n_marginal"] == 0 and want["n_edge"] == 0, po.gpu_case_id(q)
        assert (want["first_mark"] == q[6]).all()
        assert (want["status"] == 0).all()
        total += want["n_decisions"]
        share = want["accepted"].sum() / float(want["n_decisions"])
        assert 0.05 < share < 0.999, (po.gpu_case_id(q), share)             # the chains do move, and do refuse
    assert total > 1e5


def test_invariances_of_the_restatement():
    """a problem alone, in a batch and in a reversed batch; one call against two through `end` / `first_step`; thin and
    keep_from against slices of the full chain"""
    f = po.case("llh", 5, 9, 2, 8, "box")
    pr, x0 = f["pr"], f["x0"]
    ids = np.arange(5) + 40
    full = po.sample(pr, x0, 20, po.SEED, stream=2, chain_id=ids, first_step=100)
    rev = {k: (v[::-1] if isinstance(v, np.ndarray) and v.shape[:1] == (5,) and k != "ips" else v)
           for k, v in pr.items()}
    back = po.sample(rev, x0[::-1], 20, po.SEED, stream=2, chain_id=ids[::-1], first_step=100)
    assert np.array_equal(back["chain"][::-1], full["chain"])
    one = {k: (v[2:3] if isinstance(v, np.ndarray) and k != "ips" else v) for k, v in pr.items()}
    alone = po.sample(one, x0[2:3], 20, po.SEED, stream=2, chain_id=ids[2:3], first_step=100)
    assert np.array_equal(alone["chain"][0], full["chain"][2]) and np.array_equal(alone["logp"][0], full["logp"][2])
    a = po.sample(pr, x0, 8, po.SEED, stream=2, chain_id=ids, first_step=100)
    b = po.sample(pr, a["end"], 12, po.SEED, stream=2, chain_id=ids, first_step=108)
    assert np.array_equal(np.concatenate([a["chain"], b["chain"]], axis=1), full["chain"])
    assert np.array_equal(a["accepted"] + b["accepted"], full["accepted"])
    thin = po.sample(pr, x0, 20, po.SEED, stream=2, chain_id=ids, first_step=100, keep_from=103, thin=4)
    assert np.array_equal(thin["chain"], full["chain"][:, 3::4])
    assert not np.array_equal(full["chain"][0], full["chain"][1])


# --------------------------------------------------------------------- statistical validity of the definition
@pytest.mark.parametrize("J,W", sorted(po.LENGTHS))
def test_truncated_gaussian_posterior(J, W):
    """zero response: the posterior is the Gaussian prior truncated to its box, coordinate 0 one-sided at -0.5 sigma;
    means and variances of 32 replicas against scipy.stats.truncnorm.  Lengths from the tau measured with the restatement
    (steps; `posterior_cases.TAU`): 39.1 at (J, W) = (1, 16), 48.2 at (3, 16), 130.5 at (8, 32) -> burn-in 400 / 500 /
    1400 (>= 10 tau), kept 2000 / 2500 / 6600 (>= 50 tau)."""
    arrays, mean, var, sigma = po.gauss_target(J)
    burn, keep = po.LENGTHS[(J, W)]
    assert burn >= 10 * po.TAU[(J, W)] and keep >= 50 * po.TAU[(J, W)]
    m, v, out = po.replica_moments(arrays, "llh", J, W, burn, keep, mean + 0.3 * sigma, sigma)
    assert (out["status"] == 0).all()
    po.check_moments(m, mean, np.sqrt(var), "gauss J=%d mean" % J)
    po.check_moments(v, var, var, "gauss J=%d variance" % J)


@pytest.mark.parametrize("d", (0, 3))
def test_poisson_posterior_of_one_bin(d):
    """J = 1, one bin, mu = E + R eta, a flat prior on a box, llh with d counts: mean and variance of eta against the
    truncated gamma law in mu (scipy.special.gammainc); d = 0 is the exponential pressed against the lower bound.
    Lengths of (J, W) = (1, 16): tau 39.1 steps (the d = 0 target's, the largest) -> burn-in 400, kept 2000."""
    arrays, mean, var = po.poisson_target(d)
    burn, keep = po.LENGTHS[(1, 16)]
    m, v, out = po.replica_moments(arrays, "llh", 1, 16, burn, keep, np.array([mean]), np.array([np.sqrt(var)]))
    assert (out["status"] == 0).all()
    po.check_moments(m, np.array([mean]), np.sqrt(var), "poisson d=%d mean" % d)
    po.check_moments(v, np.array([var]), var, "poisson d=%d variance" % d)


def test_autocorr_time_of_an_ar1_series():
    """tau = (1 + rho) / (1 - rho) for x_t = rho x_(t-1) + e_t"""
    from pisa_amd.analysis import ensemble as en

    rs = np.random.RandomState(3)
    for rho in (0.5, 0.9):
        e = rs.randn(200000)
        x = np.empty_like(e)
        x[0] = e[0]
        for t in range(1, len(e)):
            x[t] = rho * x[t - 1] + e[t]
        tau = en.autocorr_time(x)
        assert abs(tau / ((1 + rho) / (1 - rho)) - 1.0) < 0.1, (rho, tau)


# ----------------------------------------------------------------------------- refusals before any device access
def test_every_refusal_comes_before_any_device_access():
    import __graft_entry__ as g

    g.build()
    from pisa_amd import _lib

    lib = _lib.lib()
    for name, rc in po.invalid_calls(lib):
        assert rc == -1, name
    p = ctypes.c_void_p(4096)

    def at(**kw):
        a = dict(mu=p, sigma=None, R=p, J=2, eta=p, method=0, B=5, T=3, seed=1, stream=0, first=0, out=p, stat=p)
        a.update(kw)
        return lib.pisa_hip_fluctuate_linear_at(a["mu"], a["sigma"], a["R"], a["J"], a["eta"], a["method"], a["B"],
                                                a["T"], a["seed"], a["stream"], a["first"], a["out"], a["stat"], None)

    for name, kw in (("scaled_poisson", dict(method=1)), ("gauss without sigma", dict(method=2)), ("J 0", dict(J=0)),
                     ("J 9", dict(J=9)), ("NULL eta", dict(eta=None)), ("NULL mu", dict(mu=None)),
                     ("no trials", dict(T=0)), ("trial numbers beyond 2^32", dict(first=2 ** 32 - 2)),
                     ("method 4", dict(method=4)), ("NULL out", dict(out=None)), ("NULL status", dict(stat=None))):
        assert at(**kw) == -1, name


# ------------------------------------------------------------------------- the drivers on the restatement solver
def _toy(metric="llh", ips=(10.0, 4.0)):
    """the toy grid of tests/test_host_observed.py with a box, and an observed map: one Poisson draw of point 4"""
    from pisa_amd.analysis import ensemble as en
    from tests import ensemble_cases as ec

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    K, B = hist.shape
    x = np.linspace(-1.0, 1.0, B)
    R = np.stack([hist, hist * x[None, :]], axis=1)
    ips = np.array(ips)
    center = np.tile(np.array([[0.05, 0.0]]), (K, 1)) * (ips > 0)
    share = float(np.sum((ips * center[0]) ** 2)) * (1.0 if metric in ("chi2", "mod_chi2") else -0.5)
    prior_at_point = np.full(K, share)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty + prior_at_point, metric)
    resp = en.NuisanceResponse(("norm", "tilt"), R, ips, center, prior_at_point, np.full((K, 2), [1.0, 0.0]),
                               lower=np.array([-0.15, -0.5]), upper=np.array([0.1, 0.5]))
    observed = np.random.RandomState(5).poisson(hist[4] + 0.04 * R[4, 0] + 0.1 * R[4, 1]).astype(np.float64)
    return en, grid, resp, hist, sumw2, R, observed


def test_posterior_sample_starts_runs_and_continues():
    en, grid, resp, hist, sumw2, R, observed = _toy()
    solver = po.NumpySolver()
    W, n_keep = 8, 5
    s = en.posterior_sample(observed, grid, "llh", resp, points=[2, 4, 7], n_keep=n_keep, n_walkers=W, thin=3, n_burn=6,
                            random_state=11, solver=solver)
    names = [c[0] for c in solver.calls]
    assert names == ["profiled_matrix", "hesse", "draw_linear", "draw_linear", "draw_linear", "posterior"]
    assert s.eta.shape == (3, n_keep * W, 2) and s.logp.shape == (3, n_keep * W) and s.values.shape == s.eta.shape
    assert s.points == [2, 4, 7] and s.thin == 3 and s.n_burn == 6 and s.seed == 11 and s.n_walkers == W
    assert s.tau.shape == (3, 2) and s.acceptance.shape == (3,) and not s.status.any()
    assert np.all((s.acceptance > 0.1) & (s.acceptance < 1.0))
    assert np.all((s.eta >= resp.lower) & (s.eta <= resp.upper))
    assert np.array_equal(s.values, np.array([1.0, 0.0]) + s.eta)
    # the starts: normals about the fit inside the box, stream 0x40000000 + k, the spread the fit's sigma
    fit = en.fit_observed(observed, grid, "llh", resp, po.NumpySolver(), covariance=True)
    starts = [c for c in solver.calls if c[0] == "draw_linear"]
    assert [c[2:] for c in starts] == [(W, 0x40000000 + k, 0) for k in (2, 4, 7)]
    x0 = np.empty((3, W, 2))
    for i, k in enumerate((2, 4, 7)):
        scale = np.minimum(fit["sigma"][k], (resp.upper - resp.lower) / 4.0)
        assert np.array_equal(en._start_scales(resp, k, fit["cov"][k], resp.lower, resp.upper), scale)
        x0[i] = po.NumpySolver().draw_linear(hist[k], R[k], None, "poisson", W, 11, 0x40000000 + k, scale, fit["eta"][k],
                                             resp.lower, resp.upper)["eta"]
    # one call of n_burn + n_keep thin steps, every thin-th kept, flattened step-major; chain id = the point
    direct = po.NumpySolver().posterior("llh", observed[None, :], hist, R, x0, 6 + n_keep * 3, 11,
                                        t_of=np.zeros(3, dtype=int), k_of=[2, 4, 7], inv_prior_sigma=resp.inv_prior_sigma,
                                        center=resp.center, lower=resp.lower, upper=resp.upper, chain_id=[2, 4, 7],
                                        keep_from=6 + 2, thin=3)
    assert np.array_equal(s.eta, direct["chain"].reshape(3, n_keep * W, 2))
    assert np.array_equal(s.eta[:, :W], direct["chain"][:, 0])
    # a subset of points reproduces the full run's rows
    one = en.posterior_sample(observed, grid, "llh", resp, points=[4], n_keep=n_keep, n_walkers=W, thin=3, n_burn=6,
                              random_state=11, solver=po.NumpySolver())
    assert np.array_equal(one.eta[0], s.eta[1]) and np.array_equal(one.logp[0], s.logp[1])
    # helpers
    assert s.mean().shape == (3, 2) and s.cov().shape == (3, 2, 2)
    lo, hi = s.interval(0.9)
    assert np.all(lo <= s.mean()) and np.all(s.mean() <= hi) and np.all(lo >= resp.lower) and np.all(hi <= resp.upper)
    # the pilot is the burn-in and the chain continues from its end: equal to one call with the thin it found
    solver = po.NumpySolver()
    auto = en.posterior_sample(observed, grid, "llh", resp, points=[4], n_keep=4, n_walkers=W, pilot_steps=40,
                               random_state=11, solver=solver)
    calls = [c for c in solver.calls if c[0] == "posterior"]
    assert calls[0][2:] == (40, 0, 20, 1) and calls[1][2:] == (4 * auto.thin, 40, 40 + auto.thin - 1, auto.thin)
    assert auto.n_burn == 40 and auto.thin >= 1 and not auto.reliable.any()          # 20 steps are no 50 tau
    fixed = en.posterior_sample(observed, grid, "llh", resp, points=[4], n_keep=4, n_walkers=W, thin=auto.thin, n_burn=40,
                                random_state=11, solver=po.NumpySolver())
    assert np.array_equal(auto.eta, fixed.eta)


def test_posterior_sample_refusals_and_start_scales():
    en, grid, resp, hist, sumw2, R, observed = _toy()
    solver = po.NumpySolver()
    kw = dict(n_keep=2, thin=1, n_burn=0, random_state=1, solver=solver)
    for bad in (dict(n_walkers=7), dict(n_walkers=2), dict(n_walkers=258), dict(points=[9]), dict(n_keep=0),
                dict(thin=0)):
        with pytest.raises(ValueError):
            en.posterior_sample(observed, grid, "llh", resp, **dict(dict(kw, n_walkers=8), **bad))
    with pytest.raises(ValueError, match="not among"):
        en.posterior_sample(observed, grid, "nope", resp, n_walkers=8, **kw)
    with pytest.raises(ValueError, match="MC-uncertainty"):
        en.posterior_sample(observed, grid, "mcllh_mean", resp, n_walkers=8, **kw)
    with pytest.raises(ValueError, match="response="):
        en.posterior_sample(observed, grid, "llh", None, n_walkers=8, **kw)
    # no variance, no prior, no finite range: the parameter is named
    free = en.NuisanceResponse(("norm", "tilt"), R, [10.0, 0.0], resp.center, None, None, lower=np.array([-0.15, -np.inf]))
    with pytest.raises(ValueError, match="'tilt'"):
        en._start_scales(free, 3, None, free.lower, None)
    nan = np.full((2, 2), np.nan)
    assert np.array_equal(en._start_scales(resp, 0, None, resp.lower, resp.upper), [0.0625, 0.25])   # prior 0.1 cut to
    # a quarter of the box 0.25; prior 0.25
    assert np.array_equal(en._start_scales(resp, 0, np.zeros((2, 2)), np.array([0.0, -0.5]), np.array([0.0, 0.5])),
                          [0.0, 0.25])                                                  # pinned: 0
    boxed = en.NuisanceResponse(("norm", "tilt"), R, [0.0, 0.0], None, None, None, lower=np.array([-0.4, -0.8]),
                                upper=np.array([0.4, 0.8]))
    assert np.array_equal(en._start_scales(boxed, 0, nan * 0 + 0, boxed.lower, boxed.upper), [0.1, 0.2])   # box / 8


@pytest.mark.parametrize("method", ("poisson", "gauss+poisson"))
def test_truths_trial_n_is_generated_at_row_n(method):
    en, grid, resp, hist, sumw2, R, observed = _toy()
    solver = po.NumpySolver()
    k, T = 5, 12
    rs = np.random.RandomState(2)
    rows = np.clip(0.05 * rs.randn(20, 2), resp.lower, resp.upper)
    sigma = None if method == "poisson" else np.sqrt(sumw2[k])
    kw = dict(method=method, response=resp, truths=rows)
    got, used = en.pseudo_data(grid, k, T, 8, generator="device", solver=solver, return_truth=True, **kw)
    assert [c[0] for c in solver.calls] == ["draw_linear_at"] and np.array_equal(used, rows[:T])
    want = solver.draw_linear_at(hist[k], R[k], sigma, method, rows[:T], 8, k)["data"]
    assert np.array_equal(got, want)
    # row n alone: the same entry
    for n in (0, 7, 11):
        alone = solver.draw_linear_at(hist[k], R[k], sigma, method, rows[n:n + 1], 8, k, first_trial=n)["data"]
        assert np.array_equal(alone[0], got[n])
    # the host generator: the mean at row t and the method's own calls on the one RandomState
    got = en.pseudo_data(grid, k, T, 8, solver=solver, **kw)
    rs = np.random.RandomState(8)
    want = np.stack([en._host_row(en._linear_mean(hist[k], R[k], rows[t]), sigma, method, rs) for t in range(T)])
    assert np.array_equal(got, want)
    # every row the fitted displacements: nuisance="profiled", on both generators
    eta_obs = en.fit_observed(observed, grid, "llh", resp, solver)["eta"]
    same = np.tile(eta_obs[k], (T, 1))
    for generator in en.GENERATORS:
        a = en.pseudo_data(grid, k, T, 8, generator=generator, solver=solver, method=method, response=resp, truths=same)
        b = en.pseudo_data(grid, k, T, 8, generator=generator, solver=solver, method=method, response=resp,
                           nuisance="profiled", observed=observed)
        assert np.array_equal(a, b), generator
    # a mapping and a posterior sample give their point's rows
    assert np.array_equal(en.pseudo_data(grid, k, T, 8, generator="device", solver=solver, method=method, response=resp,
                                         truths={k: rows}), en.pseudo_data(grid, k, T, 8, generator="device",
                                                                           solver=solver, **kw))


def test_feldman_cousins_at_truths_does_not_depend_on_the_chunks():
    metric, T, cl, seed = "llh", 24, (0.6827, 0.90), 1
    en, grid, resp, hist, sumw2, R, observed = _toy(metric)
    points = [0, 5]
    sample = en.posterior_sample(observed, grid, metric, resp, points=points, n_keep=3, n_walkers=8, thin=2, n_burn=4,
                                 random_state=3, solver=po.NumpySolver())
    assert len(sample) == 24
    for generator in en.GENERATORS:
        solver = po.NumpySolver()
        kw = dict(true_points=points, solver=solver, generator=generator, response=resp, truths=sample)
        crit, info = en.feldman_cousins(grid, metric, T, cl, seed, **kw)
        assert crit.shape == (2, 2) and np.array_equal(info["truths_used"], [T, T]) and info["flagged"].shape == (2,)
        assert ("draw_linear_at" in [c[0] for c in solver.calls]) == (generator == "device")
        for i, k0 in enumerate(points):
            rs = np.random.RandomState([seed, k0]) if generator == "host" else seed
            data = en.pseudo_data(grid, k0, T, rs, generator=generator, solver=solver, response=resp, truths=sample)
            assert np.array_equal(en.critical_values(en.delta_metric(data, grid, metric, k0, solver, resp), cl), crit[i])
        one, _ = en.feldman_cousins(grid, metric, T, cl, seed, **dict(kw, true_points=[5]))
        assert np.array_equal(one[0], crit[1])
        by_rows, _ = en.feldman_cousins(grid, metric, T, cl, seed, **dict(kw, truths={0: sample.eta[0], 5: sample.eta[1]}))
        assert np.array_equal(by_rows, crit)
        if generator == "device":
            chunked = po.NumpySolver()
            got, _ = en.feldman_cousins(grid, metric, T, cl, seed, **dict(kw, solver=chunked),
                                        chunk_bytes=7 * 8 * hist.shape[1])
            assert np.array_equal(got, crit)
            assert [c[2:] for c in chunked.calls if c[0] == "draw_linear_at"][:4] == [(7, 0, 0), (7, 0, 7), (7, 0, 14),
                                                                                      (3, 0, 21)]
    fixed, info = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points, solver=po.NumpySolver(),
                                     response=resp)
    assert set(info) == {"flagged"} and not np.array_equal(fixed, crit)


def test_what_truths_refuses():
    from tests import truth_cases as tc

    en, grid, resp, hist, sumw2, R, observed = _toy()
    solver = po.NumpySolver()
    rows = np.zeros((10, 2))
    ok = dict(generator="device", solver=solver, response=resp, truths=rows)
    en.pseudo_data(grid, 3, 10, 1, **ok)
    for bad, match in ((dict(response=None), "needs response="), (dict(nuisance="prior"), "leave nuisance"),
                       (dict(nuisance="profiled", observed=observed), "leave nuisance"),
                       (dict(observed=observed), "leave nuisance"), (dict(method="scaled_poisson"), "scaled_poisson"),
                       (dict(truths=np.zeros((10, 3))), r"\[n, 2\]"), (dict(truths=np.zeros(10)), r"\[n, 2\]"),
                       (dict(truths={4: rows}), "no rows for point 3"), (dict(generator="nope"), "not among"),
                       (dict(truths=np.full((10, 2), np.nan)), "NaN"),
                       (dict(solver=tc.NumpyTruthSolver()), "draw_linear_at")):
        with pytest.raises(ValueError, match=match):
            en.pseudo_data(grid, 3, 10, 1, **dict(ok, **bad))
    with pytest.raises(ValueError, match="2 rows more"):
        en.pseudo_data(grid, 3, 12, 1, **ok)
    with pytest.raises(ValueError, match="outside the grid"):
        en.pseudo_data(grid, 9, 10, 1, **ok)
    sample = en.posterior_sample(observed, grid, "llh", resp, points=[3], n_keep=2, n_walkers=8, thin=5, n_burn=2,
                                 random_state=3, solver=po.NumpySolver())
    with pytest.raises(ValueError, match="needs 5 steps more"):      # 20 trials, 16 rows: 4 rows = 1 kept step of thin 5
        en.pseudo_data(grid, 3, 20, 1, **dict(ok, truths=sample))
    with pytest.raises(ValueError, match="needs 10 steps more"):     # 9 rows: two kept steps of 8 walkers
        en.pseudo_data(grid, 3, 25, 1, **dict(ok, truths=sample))
    with pytest.raises(ValueError, match="not point 4"):
        en.pseudo_data(grid, 4, 4, 1, **dict(ok, truths=sample))
    hist_mc, sumw2_mc, pts, pen = __import__("tests.ensemble_cases", fromlist=["x"]).toy_grid("mcllh_mean")
    mc_grid = en.TemplateGrid(hist_mc, sumw2_mc, pts, None, None, "mcllh_mean")
    with pytest.raises(ValueError, match="MC-uncertainty"):
        en.pseudo_data(mc_grid, 3, 10, 1, **ok)
    for bad, match in ((dict(nuisance="prior"), "leave nuisance"), (dict(truths={0: rows}), "no rows for point 5"),
                       (dict(response=None), "needs response=")):
        with pytest.raises(ValueError, match=match):
            en.feldman_cousins(grid, "llh", 10, (0.9,), 1, true_points=[0, 5],
                               **dict(dict(ok, truths={0: rows, 5: rows}), **bad))
    with pytest.raises(ValueError, match="rows more"):
        en.feldman_cousins(grid, "llh", 11, (0.9,), 1, true_points=[0], **dict(ok, truths={0: rows}))
    # nuisance="posterior" stays an unknown name
    with pytest.raises(ValueError, match="not among"):
        en.pseudo_data(grid, 3, 10, 1, generator="device", solver=solver, response=resp, nuisance="posterior")
    assert en.NUISANCE == ("fixed", "prior", "profiled", "fitted")
