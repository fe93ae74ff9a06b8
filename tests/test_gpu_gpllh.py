"""The generalized Poisson-gamma likelihood on the device: goldens of the reference (tests/golden/gpllh_ref.npz),
the likelihood.generalized_llh_params service, the fused tail of the engine against the unfused kernels, several
points per sweep, and the errors."""
import os
from collections import OrderedDict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gpllh_ref.npz")


def _golden():
    g = np.load(GOLDEN)
    return g, [str(n) for n in g["cases"]]


def _binning(n_bins):
    from pisa_amd.core.binning import MultiDimBinning, OneDimBinning

    return MultiDimBinning([OneDimBinning("reco_energy", bin_edges=np.arange(n_bins + 1, dtype=float) + 1.0)])


def _mapsets(g, name):
    from pisa_amd.core.map import Map, MapSet

    b = _binning(g[name + "__data"].size)
    out = OrderedDict()
    for key, src in (("weights", "wsum"), ("llh_alphas", "alpha"), ("llh_betas", "beta"), ("n_mc_events", "n_mc")):
        out[key] = MapSet([Map("c%d" % c, row, b) for c, row in enumerate(g[name + "__" + src])])
    return Map("data", g[name + "__data"], b), out


def test_goldens_per_bin_and_total():
    g, names = _golden()
    for name in names:
        data, ev = _mapsets(g, name)
        empty = g[name + "__empty"].tolist() or None
        per_bin = data.generalized_poisson_llh(ev, empty_bins=empty, binned=True)
        want = g[name + "__per_bin"].copy()
        # the one deliberate deviation: k = 0 in the Poisson branch is the limit -sum w (the reference: 0 log 0 = NaN)
        dev = (g[name + "__branch"] == 1) & (g[name + "__data"] == 0)
        assert np.all(np.isnan(want[dev]))
        want[dev] = -g[name + "__wsum"].sum(axis=0)[dev]
        np.testing.assert_allclose(per_bin, want, rtol=1e-11, atol=1e-11, err_msg=name)
        for special in (1.0, np.log(1e-300), np.log(1e-10)):
            assert np.array_equal(per_bin == special, want == special), (name, special)
        total = data.generalized_poisson_llh(ev, empty_bins=empty)
        np.testing.assert_allclose(total, g[name + "__total"][0] if not dev.any() else want.sum(), rtol=1e-10,
                                   err_msg=name)


def _stage_on(g, name, overlap=False):
    from pisa_amd.core.container import Container, ContainerSet
    from pisa_amd.stages.likelihood.generalized_llh_params import generalized_llh_params

    n_bins = g[name + "__data"].size
    b = _binning(n_bins)
    sizes = g[name + "__sizes"]
    w_all, bins_all = g[name + "__weights"], g[name + "__bins"]
    cs, lo = [], 0
    for c, n in enumerate(sizes):
        cont = Container("c%d" % c)
        w, bins = w_all[lo:lo + n], bins_all[lo:lo + n]
        lo += n
        cont["weights"] = w.copy()
        if g[name + "__has_kfold"][0]:
            cont["kfold_mask"] = g[name + "__kfold"][lo - n:lo].astype(np.int64)
        for i in range(n_bins):
            cont["bin_%d_mask" % i] = (bins == i).astype(np.int64)
        if overlap:
            # one more event list holding every event of bin 0 again: the lists are no longer disjoint
            cont["bin_%d_mask" % (n_bins - 1)] = ((bins == n_bins - 1) | (bins == 0)).astype(np.int64)
        cs.append(cont)
    st = generalized_llh_params(apply_mode=b)
    st.data = ContainerSet("data", cs)
    st.setup()
    st.run()
    return st


def test_stage_on_the_golden_inputs():
    g, names = _golden()
    for name in names:
        st = _stage_on(g, name)
        for c, cont in enumerate(st.data.containers):
            cont.representation = st.apply_mode
            for key, src in (("llh_alphas", "alpha"), ("llh_betas", "beta"), ("weights", "wsum"),
                             ("old_sum", "old_sum"), ("n_mc_events", "n_mc")):
                np.testing.assert_allclose(np.asarray(cont[key]).ravel(), g[name + "__" + src][c], rtol=1e-13,
                                           atol=0, err_msg="%s %s %d" % (name, key, c))
            assert cont["mean_adjustment"] == pytest.approx(g[name + "__adjust"][c], rel=1e-13, abs=0)
            assert np.all(np.asarray(cont["hs_scales"]) == 0)


def test_stage_disjoint_and_overlapping_lists_agree():
    g, _ = _golden()
    name = "lowmc"
    a = _stage_on(g, name)
    b = _stage_on(g, name, overlap=True)
    assert all(v["disjoint"] for v in a._lists.values()) and not all(v["disjoint"] for v in b._lists.values())
    last = g[name + "__data"].size - 1
    for ca, cb in zip(a.data.containers, b.data.containers):
        ca.representation = a.apply_mode
        cb.representation = b.apply_mode
        for key in ("llh_alphas", "llh_betas", "weights", "old_sum"):
            x, y = np.asarray(ca[key]).ravel(), np.asarray(cb[key]).ravel()
            assert np.array_equal(x[:last], y[:last]), key


def test_stage_negative_weight_raises():
    g, _ = _golden()
    with pytest.raises(ValueError):
        gg = {k: g[k] for k in g.files}
        gg["single__weights"] = gg["single__weights"].copy()
        gg["single__weights"][3] = -1.0
        _stage_on(gg, "single")


def _engine(n_events, k_max, seed=3):
    """an engine on the synthetic workload, data = the template scaled to a largest count of about k_max"""
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=n_events, grid=(24, 16), out_binning="dragon", seed=seed)
    st = synthetic.DeviceState(wl)
    p = wl.osc_params(theta23_deg=45.0, dm31=2.4e-3)
    st.make_pseudo_data(p, seed=1)
    st.accumulate(p)
    st.allreduce()
    st.finalize()
    t = st.ws.hist.sum(dim=0).cpu().numpy()
    st.set_data(np.floor(t * (k_max / t.max())))
    st.configure_gpllh()
    return wl, st


def _points(wl):
    return [wl.osc_params(theta23_deg=t, dm31=d) for t, d in ((45.0, 2.4e-3), (42.0, 2.5e-3), (48.5, 2.3e-3))]


@pytest.mark.parametrize("n_events,k_max", [(20000, 300.0), (400000, 2000.0)])
def test_fused_tail_equals_the_unfused_kernels_bit_for_bit(n_events, k_max):
    import torch

    from pisa_amd import kernels as K

    wl, st = _engine(n_events, k_max)
    g = st._gpllh
    mixture = (g["n_mc_host"] <= 100).any(axis=0)
    assert mixture.any() if n_events < 100000 else True
    for p in _points(wl):
        v = st.eval_host(p, "generalized_poisson_llh")
        st.check_status()
        hist, sumw2 = (t.clone() for t in (st.ws.hist, st.ws.sumw2))
        alpha, beta, wsum = K.gpllh_params(hist, sumw2, g["n_mc"], g["adjust"])
        total, per_bin = K.generalized_poisson_llh(st.data, wsum, alpha, beta, g["n_mc"], g["empty"])
        assert v == float(total.item())
        assert torch.equal(per_bin, g["per_bin"][0])
        # and repeatable, through every entry point
        assert st.eval_host(p, "generalized_poisson_llh") == v
        assert float(st.eval(p, "generalized_poisson_llh").item()) == v
        assert not np.isnan(v)


def test_eval_many_equals_eval_host_per_point():
    wl, st = _engine(20000, 300.0)
    pts = _points(wl)
    one = [st.eval_host(p, "generalized_poisson_llh") for p in pts]
    many = st.eval_many(pts, "generalized_poisson_llh")
    st.check_status()
    assert many == one
    assert st.eval_many(pts, "generalized_poisson_llh") == many
    llh = st.eval_many(pts, "llh")            # the other kinds are untouched on the same engine
    assert llh == [st.eval_host(p, "llh") for p in pts]


def test_engine_refuses_unconfigured_use_and_post_histogram_scales():
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=5000, grid=(24, 16), out_binning="dragon", seed=5)
    st = synthetic.DeviceState(wl)
    p = wl.osc_params(theta23_deg=45.0, dm31=2.4e-3)
    st.make_pseudo_data(p, seed=1)
    with pytest.raises(RuntimeError, match="configure_gpllh"):
        st.eval_host(p, "generalized_poisson_llh")
    st.configure_gpllh()
    st.front()
    import torch

    scale = torch.ones((len(st.cont), st.n_bins), dtype=torch.float64, device=st.dev)
    with pytest.raises(ValueError):
        st.tail_host("generalized_poisson_llh", scale=scale)


def test_negative_data_raises():
    wl, st = _engine(20000, 300.0)
    d = st.data.clone()
    d[2] = -3.0
    st.data = d
    st.eval_host(_points(wl)[0], "generalized_poisson_llh")
    with pytest.raises(ValueError):
        st.check_status()


def test_stage_follows_a_kfold_mask_changed_after_set_up():
    """the reference multiplies `kfold_mask` in on every apply: a new mask changes alpha (its event counts) and the
    sums, while `n_mc_events` and the mean adjustment stay the set-up's"""
    g, _ = _golden()
    st = _stage_on(g, "kfold")
    c = st.data.containers[0]
    c.representation = st.apply_mode
    a0, n0 = np.array(c["llh_alphas"]).ravel(), np.array(c["n_mc_events"]).ravel()
    n = g["kfold__sizes"]
    lo = 0
    for i, ci in enumerate(st.data.containers):
        # (an upstream stage writes the event weights of every evaluation; the service leaves binned ones behind)
        ci.representation = "events"
        ci["weights"] = g["kfold__weights"][lo:lo + n[i]].copy()
        lo += n[i]
    kf = np.asarray(c["kfold_mask"]).copy()
    c["kfold_mask"] = np.ones_like(kf)
    st.run()
    c.representation = st.apply_mode
    sums = np.array(c["old_sum"]).ravel()
    n = g["kfold__sizes"][0]
    w, bins = g["kfold__weights"][:n], g["kfold__bins"][:n]
    np.testing.assert_allclose(sums, [w[bins == i].sum() for i in range(sums.size)], rtol=1e-13)
    assert np.array_equal(np.array(c["n_mc_events"]).ravel(), n0)
    assert not np.array_equal(np.array(c["llh_alphas"]).ravel(), a0)


_CFG_STAGES = """
[utils.add_indices]
calc_mode = events
apply_mode = reco_binning

[likelihood.generalized_llh_params]
apply_mode = reco_binning
"""


def _pipelines(tmp_path, n_events):
    from pisa_amd.core.distribution_maker import DistributionMaker
    from pisa_amd.utils.resources import find_resource

    text = open(find_resource("settings/pipeline/example_hip.cfg")).read()
    text = text.replace("param.n_events = 1.2e5", "param.n_events = %g" % n_events)
    hist_cfg = tmp_path / ("hist_%d.cfg" % n_events)
    hist_cfg.write_text(text)
    gp = text.replace("osc.prob3, aeff.aeff, utils.hist", "osc.prob3, aeff.aeff, utils.add_indices, likelihood.generalized_llh_params")
    gp = gp.replace("output_key = weights, errors", "output_key = weights") + _CFG_STAGES
    gp_cfg = tmp_path / ("gpllh_%d.cfg" % n_events)
    gp_cfg.write_text(gp)
    return DistributionMaker(str(hist_cfg)), DistributionMaker(str(gp_cfg))


@pytest.mark.parametrize("n_events,k_max", [(1.2e4, 300.0), (1.2e6, 300.0)])
def test_cfg_pipeline_through_the_stage_equals_the_engine(tmp_path, n_events, k_max):
    """events -> osc.prob3 -> aeff.aeff -> utils.add_indices -> likelihood.generalized_llh_params, evaluated through
    Map.generalized_poisson_llh, against the engine of the utils.hist pipeline on the same events (its own MC counts,
    its own sums) at three parameter points"""
    from pisa_amd.core.map import Map, MapSet
    from pisa_amd.core.units import ureg

    dm_h, dm_g = _pipelines(tmp_path, n_events)
    template = dm_h.get_outputs(return_sum=True).maps[0]
    t = template.hist
    data = Map("data", np.floor(t * (k_max / t.max())), template.binning)
    eng = dm_h.pipelines[0]["hist"]._engine
    n_mc, _ = eng.configure_gpllh()
    eng.set_data(data.hist)
    if n_events < 1e5:
        assert (n_mc <= 100).any(axis=0).all()
    else:
        assert (n_mc > 100).all(axis=0).any()
    for theta23, dm31 in ((45.0, 2.4e-3), (41.0, 2.55e-3), (49.0, 2.3e-3)):
        for dm in (dm_h, dm_g):
            dm.params.theta23.value = theta23 * ureg.degree
            dm.params.deltam31.value = dm31 * ureg.eV ** 2
        dm_h.get_outputs(return_sum=True)
        want = eng.tail_host("generalized_poisson_llh")
        eng.check_status()
        dm_g.get_outputs(return_sum=True)
        pipe = dm_g.pipelines[0]
        ev = OrderedDict()
        for key in ("weights", "llh_alphas", "llh_betas", "n_mc_events"):
            maps = []
            for c in pipe.data.containers:
                c.representation = pipe.output_binning
                maps.append(Map(c.name, np.asarray(c[key], dtype=np.float64).reshape(data.hist.shape), data.binning))
            ev[key] = MapSet(maps)
        assert np.array_equal(np.stack([m.hist.ravel() for m in ev["n_mc_events"].maps]), n_mc)
        got = data.generalized_poisson_llh(ev)
        np.testing.assert_allclose(got, want, rtol=1e-12)


def _gpllh_ranks(n_ranks, out_dir):
    import json
    import socket
    import subprocess
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "gpllh_dist_cases.py"), str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.setdefault("OMP_NUM_THREADS", "1")
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-4000:]
    return [json.load(open(os.path.join(str(out_dir), "gpllh_r%d.json" % r))) for r in range(n_ranks)]


def test_two_and_three_ranks_on_one_device_reproduce_the_single_rank_bits(tmp_path):
    one = _gpllh_ranks(1, tmp_path / "one")[0]
    assert len(one["values"]) == 3 and all(np.isfinite(float.fromhex(v)) for v in one["values"])
    for n in (2, 3):
        for r in _gpllh_ranks(n, tmp_path / ("r%d" % n)):
            assert r["world"] == n
            assert r["n_mc"] == one["n_mc"]
            assert r["values"] == one["values"] and r["many"] == one["many"]
