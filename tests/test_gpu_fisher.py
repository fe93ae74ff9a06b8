"""Fisher matrix and pull method on the device (`pisa_hip_fisher`, `HotPathEngine.fisher_many`,
`DistributionMaker._fisher_templates`, pisa_amd/utils/fisher_matrix.py and pull_method.py):
  * the reference's own results (tests/golden/fisher_ref.npz);
  * the engine's one-sweep and point-by-point paths against a numpy restatement of the reference's loop on the
    engine's single-point maps, bit for bit;
  * `get_fisher_matrix` / `calculate_pulls` on example_hip.cfg against a serial restatement on
    `get_outputs(return_sum=True)`, on the sweep path and on the fallback;
  * the error cases and 2 / 3 ranks against one."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fisher_ref.npz")


def reference_matrix(grads, hist0, var0):
    """fisher_matrix.py build_fisher_matrix's loop (gradients in the caller's order)"""
    ne = np.nonzero(hist0)
    g = np.asarray(grads)[:, ne[0]]
    sig = np.sqrt(var0)[ne]
    f = np.zeros((g.shape[0], g.shape[0]))
    for bg, bv in zip(g.T, sig):
        f += np.outer(bg, bg) / bv
    return f, ne


def host_total(rows):
    """MapSet.total(): rows added in index order, from row 0"""
    t = rows[0].copy()
    for r in rows[1:]:
        t += r
    return t


class _M:
    def __init__(self, h, v):
        self.nominal_values, self.variances = h, v


class _S(dict):
    def __init__(self, h, v):
        super().__init__(total=_M(h, v))


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("key", ["p1", "p3", "p8", "big"])
def test_goldens(key):
    from pisa_amd import kernels as K
    from pisa_amd.utils.fisher_matrix import FisherMatrix, build_fisher_matrix
    from pisa_amd.utils.pull_method import calculate_pulls

    g = np.load(GOLD)
    pts, var, vals, truth = g[key + "_points"], g[key + "_var"], g[key + "_vals"], g[key + "_truth"]
    names, srt = list(g[key + "_names"]), list(g[key + "_sorted"])
    n_par = len(names)
    v = np.zeros_like(pts)
    v[0] = var
    dx = [float(vals[p][0] - vals[p][1]) for p in range(n_par)]
    res = K.fisher(K.to_device(pts), K.to_device(v), [2 + 2 * p for p in range(n_par)],
                   [1 + 2 * p for p in range(n_par)], dx, truth=torch.as_tensor(truth))
    assert res["status"] == 0 and res["nonempty"] == g[key + "_nonempty"].size
    grad = res["grad"].cpu().numpy()
    assert np.array_equal(grad, g[key + "_grads"])
    order = [names.index(n) for n in srt]
    m = res["matrix"].cpu().numpy()[np.ix_(order, order)]
    np.testing.assert_allclose(m, g[key + "_matrix"], rtol=1e-12, atol=0)
    assert np.array_equal(m, m.T)
    fm = FisherMatrix(m, srt, list(g[key + "_best"]))
    pulls = np.asarray(np.dot(fm.covariance, res["pull"].cpu().numpy()[order])).ravel()
    np.testing.assert_allclose(pulls, g[key + "_pulls"], rtol=1e-12, atol=1e-300)
    # the public functions on MapSet-like inputs
    gd = {n: g[key + "_grads"][i] for i, n in enumerate(names)}
    fid = _S(pts[0], var)
    f2, ne = build_fisher_matrix(gd, fid, types.SimpleNamespace(nominal_values=list(g[key + "_best"])))
    assert f2.parameters == srt and np.array_equal(ne[0], g[key + "_nonempty"])
    np.testing.assert_allclose(np.asarray(f2.matrix), g[key + "_matrix"], rtol=1e-12, atol=0)
    pl = calculate_pulls(f2, _S(truth, truth), fid, {"total": gd}, ne)
    assert [n for n, _ in pl] == srt
    np.testing.assert_allclose([x for _, x in pl], g[key + "_pulls"], rtol=1e-12, atol=1e-300)


def test_maps_without_errors_and_singular_matrices_raise():
    from pisa_amd.utils.fisher_matrix import build_fisher_matrix
    from pisa_amd.utils.pull_method import calculate_pulls

    g = np.load(GOLD)
    pts, var = g["p3_points"], g["p3_var"]
    gd = {n: g["p3_grads"][i] for i, n in enumerate(g["p3_names"])}
    bp = types.SimpleNamespace(nominal_values=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="without error"):
        build_fisher_matrix(gd, _S(pts[0], np.zeros_like(var)), bp)
    # a parameter the templates do not depend on: zero gradient, singular matrix
    gd0 = dict(gd)
    gd0[list(gd)[1]] = np.zeros_like(pts[0])
    with pytest.raises(ValueError, match="singular"):
        build_fisher_matrix(gd0, _S(pts[0], var), bp)
    f, ne = build_fisher_matrix(gd, _S(pts[0], var), bp)
    with pytest.raises(ValueError, match="nonempty"):
        calculate_pulls(f, _S(pts[0], var), _S(pts[0], var), {"total": gd}, (ne[0][1:],))


# ------------------------------------------------------------------ engine
def _engine_case(out_binning, n_events, n_par, scales=False, seed=3):
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=n_events, grid=(60, 40), out_binning=out_binning, seed=seed)
    st = synthetic.DeviceState(wl, compact=True)
    st.make_pseudo_data(wl.osc_params(), seed=0)
    rs = np.random.RandomState(seed)
    fid = dict(theta23_deg=42.0, dm31=2.457e-3, deltacp_deg=180.0)
    keys = list(fid)
    steps = dict(theta23_deg=1.0, dm31=5e-5, deltacp_deg=15.0)
    pts, sc, pairs, dx = [wl.osc_params(**fid)], [np.ones(len(st.cont))], [], []
    cur = dict(fid)
    cur_sc = np.ones(len(st.cont))
    for p in range(n_par):
        k = keys[p % 3]
        hi, lo = cur[k] + steps[k] * (1 + 0.1 * p), cur[k] - steps[k] * (1 + 0.07 * p)
        for v in (hi, lo):          # the reference's order: points of p carry the earlier ones' last values
            cur[k] = v
            if scales:
                cur_sc = cur_sc.copy()
                cur_sc[p % len(cur_sc)] = 1.0 + 0.05 * rs.rand()
            pts.append(wl.osc_params(**cur))
            sc.append(cur_sc)
        pairs.append((2 + 2 * p, 1 + 2 * p))
        dx.append(hi - lo)
    return st, pts, (np.asarray(sc) if scales else None), pairs, dx


def _restatement(st, pts, scales, pairs, dx, truth=None):
    hist, var = [], None
    for i, p in enumerate(pts):
        if scales is not None:
            for name, s in zip(st.names, scales[i]):
                st.set_scale(name, s)
        st.eval_host(p, "llh")
        h, s2 = st.maps()
        hist.append(host_total(h))
        if i == 0:
            var = host_total(s2)
    grads = [(hist[hi] - hist[lo]) / d for (lo, hi), d in zip(pairs, dx)]
    f, ne = reference_matrix(grads, hist[0], var)
    d = None
    if truth is not None:
        sig = np.sqrt(var)[ne]
        d = np.array([np.sum(np.multiply(truth - hist[0], g)[ne] / sig) for g in grads])
    return f, np.asarray(grads), ne, hist, d


@pytest.mark.parametrize("case", ["p2_scales", "p8_two_chunks", "fine3d_point_by_point", "empty_bins"])
def test_engine_matches_the_reference_loop_bit_for_bit(case):
    binning, n_events, n_par, scales, sweeps = dict(
        p2_scales=("dragon", 12 * 20011, 2, True, 1),
        p8_two_chunks=("dragon", 12 * 20011, 8, False, 2),
        fine3d_point_by_point=("fine3d", 12 * 4001, 3, False, 0),
        empty_bins=("example3d", 12 * 40, 3, False, 1))[case]
    st, pts, sc, pairs, dx = _engine_case(binning, n_events, n_par, scales)
    if sweeps:
        assert st.sweep_capable()
    truth = st.data.cpu().numpy()
    res = st.fisher_many(pts, pairs, dx, scales=sc, truth=truth)
    assert res["sweeps"] == sweeps and res["status"] == 0
    f, grads, ne, hist, d = _restatement(st, pts, sc, pairs, dx, truth)
    if case == "empty_bins":
        assert 0 < ne[0].size < st.n_bins
    assert res["nonempty"] == ne[0].size
    assert np.array_equal(res["grad"].cpu().numpy(), grads)
    assert np.array_equal(res["totals"].cpu().numpy(), np.stack(hist))
    assert np.array_equal(res["matrix"].cpu().numpy(), f)
    np.testing.assert_allclose(res["pull"].cpu().numpy(), d, rtol=1e-12, atol=1e-300)


def test_engine_unused_parameter_gives_a_singular_matrix():
    from pisa_amd.utils.fisher_matrix import FisherMatrix

    st, pts, _, pairs, dx = _engine_case("dragon", 12 * 2000, 2)
    pts = pts[:3] + [pts[0], pts[0]]         # parameter 1's two points: the fiducial twice
    res = st.fisher_many(pts, pairs, dx)
    m = res["matrix"].cpu().numpy()
    assert not res["grad"][1].any() and m[1].tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match="singular"):
        FisherMatrix(m, ["a", "b"], [0, 0])


# ------------------------------------------------------------------ config pipeline
def _maker(free):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    return dm


def _test_vals(dm):
    out = {}
    for i, p in enumerate(dm.params.free):
        v = p.value
        out[p.name] = [v * (1.0 + 0.01 * (i + 1)), v * (1.0 - 0.013 * (i + 1))] if v.magnitude != 0 else \
            [v + 0.01, v - 0.02]
    return out


def _serial(dm, tv):
    """get_fisher_matrix restated on get_outputs(return_sum=True), the reference's loop"""
    fid = dm.get_outputs(return_sum=True)["total"]
    h0, v0 = fid.hist.copy(), fid.variances.copy()
    names = list(dm.params.free.names)
    grads = {}
    for name in names:
        pm = []
        for v in tv[name]:
            dm.params[name].value = v
            pm.append((v, dm.get_outputs(return_sum=True)["total"].hist.copy()))
        (lo, tlo), (hi, thi) = sorted(pm, key=lambda q: q[0])
        grads[name] = np.divide(np.subtract(thi.ravel(), tlo.ravel()), (hi - lo).magnitude)
    srt = sorted(names)
    f, ne = reference_matrix([grads[n] for n in srt], h0.ravel(), v0.ravel())
    return f, grads, h0, v0, ne, [dm.params[n].value.magnitude for n in names]


@pytest.mark.parametrize("free,sweep", [(("theta23", "deltam31", "aeff_scale"), True),
                                        (("theta23", "deltam31", "aeff_scale", "delta_index"), False)])
def test_get_fisher_matrix_on_the_config_pipeline(free, sweep):
    from pisa_amd.analysis.analysis import Counter
    from pisa_amd.utils.fisher_matrix import get_fisher_matrix
    from pisa_amd.utils.pull_method import calculate_pulls

    dm = _maker(free)
    tv = _test_vals(dm)
    start = {p.name: p.value for p in dm.params.free}
    f_ref, g_ref, h0, v0, ne_ref, final_ref = _serial(dm, tv)
    for n, v in start.items():
        dm.params[n].value = v
    dm.get_outputs(return_sum=True)
    eng = dm.pipelines[0]["hist"]._engine
    calls = []
    orig = eng.maps_many
    eng.maps_many = lambda *a, **k: calls.append(1) or orig(*a, **k)
    counter = Counter()
    try:
        fisher, gm, fid, ne = get_fisher_matrix(dm, tv, counter)
    finally:
        del eng.maps_many
    assert counter.count == 1 + 2 * len(free)
    assert len(calls) == (1 if sweep else 0)
    assert fisher.parameters == sorted(dm.params.free.names)
    assert np.array_equal(np.asarray(fisher.matrix), f_ref)
    for n in dm.params.free.names:
        assert np.array_equal(gm["total"][n], g_ref[n]), n
    assert np.array_equal(fid["total"].hist, h0) and np.array_equal(fid["total"].variances, v0)
    assert np.array_equal(ne[0], ne_ref[0])
    assert [dm.params[n].value.magnitude for n in dm.params.free.names] == final_ref
    assert fisher.best_fits == list(dm.params.free.nominal_values)
    # pulls on a fluctuated truth
    truth = fid.fluctuate("poisson", random_state=3)
    got = calculate_pulls(fisher, truth, fid, gm, ne)
    dmap = (truth["total"].hist - h0).ravel()[ne]
    sig = np.sqrt(v0).ravel()[ne]
    d = [np.divide(np.multiply(dmap, g_ref[n][ne]), sig).sum() for n in fisher.parameters]
    want = np.asarray(np.dot(fisher.covariance, d)).ravel()
    assert [n for n, _ in got] == fisher.parameters
    np.testing.assert_allclose([x for _, x in got], want, rtol=1e-12, atol=1e-300)


def test_gradients_and_bad_test_values_on_the_config_pipeline():
    from pisa_amd.utils.fisher_matrix import get_fisher_matrix
    from pisa_amd.utils.pull_method import get_derivative_map, get_gradients

    dm = _maker(("theta23", "deltam31"))
    tv = _test_vals(dm)
    pmaps, gm = get_gradients("theta23", dm, tv["theta23"])
    assert sorted(pmaps) == sorted(v.magnitude for v in tv["theta23"])      # keyed by magnitudes
    assert np.array_equal(get_derivative_map(pmaps), gm)
    bad = dict(tv, deltam31=tv["deltam31"] + [tv["deltam31"][0]])
    with pytest.raises(ValueError):
        get_fisher_matrix(dm, bad, 0)
    with pytest.raises(ValueError):
        get_fisher_matrix(dm, dict(tv, deltam31=[tv["deltam31"][0]] * 2), 0)


# ------------------------------------------------------------------ ranks
def _fisher_ranks(n_ranks, out_dir):
    import json
    import socket
    import subprocess
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "fisher_dist_cases.py"), str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.setdefault("OMP_NUM_THREADS", "1")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-4000:]
    return [json.load(open(os.path.join(str(out_dir), "fisher_r%d.json" % r))) for r in range(n_ranks)]


def test_two_and_three_ranks_on_one_device_reproduce_the_single_rank_bits(tmp_path):
    one = _fisher_ranks(1, tmp_path / "one")[0]
    assert one["sweeps"] == 2 and len(one["matrix"]) == 64
    for n in (2, 3):
        for r in _fisher_ranks(n, tmp_path / ("r%d" % n)):
            assert r["world"] == n and r["sweeps"] == 2
            assert r["matrix"] == one["matrix"] and r["grad"] == one["grad"]
