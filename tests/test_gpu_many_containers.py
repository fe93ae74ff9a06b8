"""Evaluations with more containers than one kernel launch takes.  The launchers cut the container list into groups
(16 for the fused accumulation, the multi-point sweep, its workgroup plan, event-mode prob3 per sign, the node flux
tables and the flux refreshes; 24 for `weight_chain_multi`; one tail workgroup for n_cont x n_bins <= 4096) and issue
a launch per group.  Every other test runs 12 containers or fewer, i.e. one group.

References:
  * split engines: the same containers as engines of at most 12 containers each.  A container's limbs are exact
    integer sums that do not depend on the other containers, so the maps must agree BIT FOR BIT, and the LLH must be
    `kernels.metric` on the stacked split maps, bit for bit;
  * the CPU oracle (oracle/pipeline_oracle.py) at the gates of the existing tests, with the extended-precision referee
    for the LLH (oracle/referee.py);
  * for the generalized Poisson-gamma likelihood, eq. 91 in 40-digit arithmetic (tests/test_host_gpllh.py), and for the
    Fisher matrix the restatement of the reference's loop (tests/test_gpu_fisher.py).
Empty containers sit at indices 15, 16 and last, where a group boundary can lose or shift them."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRID = (40, 30)
COLUMNS = ("true_energy", "true_coszen", "reco_energy", "reco_coszen", "pid", "nu_flux", "weighted_aeff",
           "initial_weights")


def names_for(n):
    """n unique container names that cycle through the 12 flavours and signs: nue_cc_s0 ... nutaubar_nc_s0, nue_cc_s1,
    ... (`synthetic.flav_nubar` reads flavour and sign from substrings)"""
    from pisa_amd.synthetic import NAMES

    return tuple("%s_s%d" % (NAMES[i % len(NAMES)], i // len(NAMES)) for i in range(n))


def edges(n):
    """the empty containers of an n-container case: the last of the first group, the first of the second, the last"""
    return (15, 16, n - 1)


def workload(names, n_per=20000, binning="dragon", empty=(), seed=7):
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=n_per * len(names), grid=GRID, out_binning=binning, seed=seed, names=names)
    for i in empty:
        ev = wl.events[i]
        for k in COLUMNS:
            ev[k] = ev[k][:0]
        ev["sample"] = [s[:0] for s in ev["sample"]]
    return wl


def sub_workload(wl, events):
    part = copy.copy(wl)
    part.events = events
    return part


def split_maps(wl, p, **kw):
    """maps of the containers of `wl` from engines of at most 12 containers each, stacked in container order"""
    from pisa_amd import synthetic

    hs, ss = [], []
    for lo in range(0, len(wl.events), 12):
        st = synthetic.DeviceState(sub_workload(wl, wl.events[lo:lo + 12]), **kw)
        st.accumulate(p)
        st.check_status()
        h, s2 = st.finalize()
        hs.append(h.clone())
        ss.append(s2.clone())
    return torch.cat(hs), torch.cat(ss)


def check_oracle(oracle, wl, hist, sumw2, data, llh, events_mode=False, rtol=1e-12):
    from oracle.pipeline_oracle import oracle_eval, oracle_eval_events
    from oracle.referee import llh_referee

    ref = (oracle_eval_events if events_mode else oracle_eval)(wl, containers=wl.events)
    ref_h = np.asarray(ref["hist"]).reshape(hist.shape)
    ref_s2 = np.asarray(ref["sumw2"]).reshape(sumw2.shape)
    np.testing.assert_allclose(hist, ref_h, rtol=rtol, atol=1e-300)
    np.testing.assert_allclose(sumw2, ref_s2, rtol=rtol, atol=1e-300)
    _, want = oracle.metric("llh", data, ref_h.sum(axis=0))
    r = llh_referee(data, hist.sum(axis=0), ref_h.sum(axis=0), llh, want)
    assert r["pure_1e-10_relative_met"] or r["met"], r


def attach_node_flux(wl, seed=2):
    """flux on the calc grid per container, and the per-event flux looked up from it (what the oracle and the
    per-event forms read)"""
    from pisa_amd import kernels as K

    g = wl.grid
    ee, cc = np.meshgrid(g.energy, g.coszen, indexing="ij")
    rs = np.random.RandomState(seed)
    for ev in wl.events:
        f_mu = 1e4 * ee ** -2.7 * (1 + 0.5 * cc ** 2) * (0.8 + 0.4 * rs.rand(*ee.shape))
        fn = np.stack([f_mu * (0.5 - 0.2 * cc), f_mu], axis=-1).reshape(-1, 2)
        ev["nu_flux_nodes"] = fn
        if len(ev["true_energy"]):
            node = K.event_indices([K.to_device(np.log(ev["true_energy"])), K.to_device(ev["true_coszen"])],
                                   g.binning).cpu().numpy()
            assert node.min() >= 0
            ev["nu_flux"] = fn[node]


FORMS = dict(idx16=dict(compact=True), exact40=dict(compact=False), coord=dict(indexed=False),
             node_flux=dict(compact=True, node_flux=True))


# ------------------------------------------------------------------ a. single point, every form
@pytest.mark.parametrize("n", [32, 33])
def test_single_point_every_form_equals_split_engines_and_oracle(n, oracle):
    """dragon (128 bins): 32 containers still take the fused tail (4096 accumulators), 33 the unfused one.  Every
    form of the event columns against the split engines (bits) and the oracle; the one-call evaluator against the
    three separate calls, with a scale moved past the first group"""
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    wl = workload(names_for(n), empty=edges(n))
    attach_node_flux(wl)
    p0 = wl.osc_params()
    p = wl.osc_params(theta23_deg=47.0, dm31=2.52e-3, deltacp_deg=60.0)
    data = None
    for form, kw in FORMS.items():
        st = synthetic.DeviceState(wl, **kw)
        assert len(st.cont) == n
        if data is None:
            data = st.make_pseudo_data(p0, seed=1)
        else:
            st.set_data(data)
        assert (len(st.cont) * st.n_bins <= K.FINALIZE_METRIC_MAX) == (n == 32)
        llh = st.eval_host(p, "llh")
        st.check_status()
        h, s2 = st.maps()
        hs, ss = split_maps(wl, p, **kw)
        assert np.array_equal(h, hs.cpu().numpy()), form
        assert np.array_equal(s2, ss.cpu().numpy()), form
        for i in edges(n):
            assert not h[i].any() and not s2[i].any(), (form, i)
        assert h[16:].sum() > 0 and h[17].sum() > 0
        assert llh == float(K.metric("llh", st.data, hs, ss).item()), form
        assert float(st.eval(p, "llh").item()) == llh, form
        check_oracle(oracle, wl, h, s2, data, llh)
    # one C-ABI call against the separate calls (idx16 and the 40 B form)
    rs = np.random.RandomState(4)
    pts = [wl.osc_params(theta23_deg=38 + 14 * rs.rand(), dm31=2.2e-3 + 6e-4 * rs.rand()) for _ in range(3)]
    for form in ("idx16", "exact40"):
        a = synthetic.DeviceState(wl, **FORMS[form])
        b = synthetic.DeviceState(wl, **FORMS[form])
        b.one_call = False
        a.set_data(data)
        b.set_data(data)
        for kind in ("llh", "mod_chi2", "chi2"):
            for q in pts:
                va, vb = a.eval_host(q, kind), b.eval_host(q, kind)
                assert va == vb and np.isfinite(va), (form, kind, va, vb)
        assert (a._evaluator is not None) == (n == 32) and b._evaluator is None
        before = a.eval_host(pts[0], "llh")
        for st in (a, b):
            st.set_scale(st.names[20], 0.6 * st.cont[20].scale)
        va, vb = a.eval_host(pts[0], "llh"), b.eval_host(pts[0], "llh")
        assert va == vb != before, form
        # the same scale in a fresh engine of the split reference
        scaled = [dict(ev) for ev in wl.events]
        scaled[20]["scale"] = a.cont[20].scale
        hs, ss = split_maps(sub_workload(wl, scaled), pts[0], **FORMS[form])
        assert va == float(K.metric("llh", a.data, hs, ss).item())
        assert np.array_equal(a.maps()[0], hs.cpu().numpy())
        a.check_status()
        b.check_status()


def test_whole_second_group_empty():
    """24 containers, 16 .. 23 without events: the second launch group has nothing to do, the first keeps its
    bits (split engines), and the empty rows stay zero, on the single-point, coordinate and sweep paths"""
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    n = 24
    wl = workload(names_for(n), n_per=15000, empty=range(16, n))
    p = wl.osc_params(theta23_deg=45.0)
    for form in ("idx16", "exact40", "coord"):
        st = synthetic.DeviceState(wl, **FORMS[form])
        st.make_pseudo_data(wl.osc_params(), seed=1)
        llh = st.eval_host(p, "llh")
        st.check_status()
        h, s2 = st.maps()
        hs, ss = split_maps(wl, p, **FORMS[form])
        assert np.array_equal(h, hs.cpu().numpy()) and np.array_equal(s2, ss.cpu().numpy()), form
        assert not h[16:].any() and h[:16].sum() > 0
        assert llh == float(K.metric("llh", st.data, hs, ss).item())
        if form == "idx16":
            pts = [p, wl.osc_params(theta23_deg=40.0), wl.osc_params(dm31=2.6e-3)]
            assert st.eval_many(pts, "llh") == [st.eval_host(q, "llh") for q in pts]
            m = st.maps_many(pts)
            assert m["sweeps"] == 1 and not m["hist"][:, 16:].any()


# ------------------------------------------------------------------ b. several points per sweep
@pytest.mark.parametrize("n", [32, 33])
def test_eval_many_and_maps_many_with_a_scale_per_point_and_container(n):
    """K = 3, 9, 17 points (17: two chunks of MAX_POINTS), every (point, container) pair with an aeff scale of its
    own: each point's value and maps are those of `eval_host` with the same scales set, bit for bit.  n = 32 takes
    the sweep with its fused tail; n = 33 the sweep for the maps (no tail bound) and point by point for the values"""
    from pisa_amd import synthetic

    wl = workload(names_for(n), empty=edges(n), seed=11)
    st = synthetic.DeviceState(wl, compact=True)
    st.make_pseudo_data(wl.osc_params(), seed=0)
    assert st.sweep_capable() and st.multi_capable() == (n == 32)
    base = np.array([c.scale for c in st.cont])
    rs = np.random.RandomState(3)
    for k in (3, 9, 17):
        pts = [wl.osc_params(theta23_deg=31.0 + 28.0 * rs.rand(), dm31=1e-3 + 6e-3 * rs.rand(),
                             deltacp_deg=360.0 * rs.rand()) for _ in range(k)]
        scales = base[None, :] * (0.5 + rs.rand(k, n))
        got = st.eval_many(pts, "llh", scales=scales)
        maps = st.maps_many(pts, scales=scales)
        assert maps["sweeps"] == (1 if k <= 16 else 2)
        st.check_status()
        for i, (q, sc) in enumerate(zip(pts, scales)):
            for name, v in zip(st.names, sc):
                st.set_scale(name, v)
            assert got[i] == st.eval_host(q, "llh"), (k, i)
            h, s2 = st.maps()
            assert np.array_equal(maps["hist"][i].cpu().numpy(), h), (k, i)
            assert np.array_equal(maps["sumw2"][i].cpu().numpy(), s2), (k, i)
            assert h[17:].sum() > 0
        for name, v in zip(st.names, base):
            st.set_scale(name, v)


# ------------------------------------------------------------------ c. 4 800 bins
def test_fine3d_partitioned_order_past_the_first_group(oracle):
    """4 800 output bins, 25 containers: the partitioned window order of the containers past 16 is laid out for
    the workgroups of the SECOND launch (`pisa_hip_hist_workgroups` plans each group on its own), and gives the
    limbs of the general window path, of the split engines and, within the gates, the oracle's maps"""
    import ctypes as C

    from pisa_amd import _lib
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    n = 25
    wl = workload(names_for(n), binning="fine3d", empty=edges(n), seed=3)
    sizes = [len(ev["true_energy"]) for ev in wl.events]
    wgs, tail = (C.c_int32 * n)(), (C.c_int32 * (n - 16))()
    lib = _lib.lib()
    assert lib.pisa_hip_hist_workgroups((C.c_int64 * n)(*sizes), n, wgs) == 0
    assert lib.pisa_hip_hist_workgroups((C.c_int64 * (n - 16))(*sizes[16:]), n - 16, tail) == 0
    assert list(wgs)[16:] == list(tail)
    assert all((w > 0) == (s > 0) for w, s in zip(wgs, sizes))
    p0 = wl.osc_params()
    p = wl.osc_params(theta23_deg=44.0)         # (the oracle reads the matrices of the last call)
    part = synthetic.DeviceState(wl, compact=True)
    assert part.index16 and all(bool(c.d_part_start) == (c.n_events > 0) for c in part.cont)
    data = part.make_pseudo_data(p0, seed=0)
    part.accumulate(p)
    part.check_status()
    limbs = part.ws.limbs.clone()
    llh = part.eval_host(p, "llh")
    h, s2 = part.maps()
    general = synthetic.DeviceState(wl, compact=True, block_order=False)
    assert not any(c.d_part_start for c in general.cont)
    general.accumulate(p)
    assert torch.equal(general.ws.limbs, limbs)
    hs, ss = split_maps(wl, p, compact=True)
    assert np.array_equal(h, hs.cpu().numpy()) and np.array_equal(s2, ss.cpu().numpy())
    assert h[17:].sum() > 0
    assert llh == float(K.metric("llh", part.data, hs, ss).item())
    check_oracle(oracle, wl, h, s2, data, llh)


# ------------------------------------------------------------------ d. event-by-event oscillation
def test_event_mode_past_the_per_sign_flush(oracle):
    """20 containers: 18 neutrinos and 2 antineutrinos (indices 3 and 19), so that the neutrino launch flushes after
    its 16th container (index 16) and carries on with 17 and 18.  Oracle (event-by-event propagation) at the gate of
    the existing event-mode tests, and the split engines bit for bit"""
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    nu = [nm for nm in synthetic.NAMES if "bar" not in nm]
    names = ["%s_s%d" % (nu[i % 6], i // 6) for i in range(18)]
    names.insert(3, "numubar_cc_s0")
    names.append("nuebar_nc_s0")
    n = len(names)
    wl = workload(tuple(names), n_per=15000, empty=(15, 16), seed=5)
    assert [ev["nubar"] for ev in wl.events].count(-1) == 2
    p0 = wl.osc_params()
    p = wl.osc_params(theta23_deg=46.0, dm31=2.5e-3)
    st = synthetic.DeviceState(wl, osc_mode="events")
    data = st.make_pseudo_data(p0, seed=1)
    llh = st.eval_host(p, "llh")
    st.check_status()
    h, s2 = st.maps()
    assert not h[15].any() and not h[16].any() and h[17].sum() > 0 and h[18].sum() > 0 and h[19].sum() > 0
    hs, ss = split_maps(wl, p, osc_mode="events")
    assert np.array_equal(h, hs.cpu().numpy()) and np.array_equal(s2, ss.cpu().numpy())
    assert llh == float(K.metric("llh", st.data, hs, ss).item())
    assert n * st.n_bins <= K.FINALIZE_METRIC_MAX
    check_oracle(oracle, wl, h, s2, data, llh, events_mode=True, rtol=1e-10)


# ------------------------------------------------------------------ e. flux refreshes
def test_flux_refreshes_past_the_first_group_equal_a_fresh_engine():
    """25 containers: `update_flux_many` (fold of new per-event fluxes), `update_flux_barr` (one-pass Barr refresh)
    and `update_flux_nodes` (node flux tables) each leave the bits of an engine built with the new fluxes"""
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    n = 25
    wl = workload(names_for(n), empty=edges(n), seed=13)
    attach_node_flux(wl, seed=6)
    p = wl.osc_params(theta23_deg=46.0)

    def fresh(fluxes, **kw):
        evs = [dict(ev) for ev in wl.events]
        for ev, f in zip(evs, fluxes):
            ev["nu_flux" if not kw.get("node_flux") else "nu_flux_nodes"] = f
        st = synthetic.DeviceState(sub_workload(wl, evs), **kw)
        st.accumulate(p)
        return st

    for index16 in (True, False):
        # per-event fluxes, folded in one launch per 16 containers
        rs = np.random.RandomState(3)
        new = [ev["nu_flux"] * (0.5 + rs.rand(*ev["nu_flux"].shape)) for ev in wl.events]
        a = synthetic.DeviceState(wl, compact=True, index16=index16)
        a.update_flux_many([(i, K.to_device(f)) for i, f in enumerate(new)])
        a.accumulate(p)
        b = fresh(new, compact=True, index16=index16)
        assert torch.equal(a.ws.limbs, b.ws.limbs), index16
        for wa, wb in zip(a._wflux, b._wflux):
            assert torch.equal(wa, wb)
        assert int(a.ws.limbs[17:].abs().sum().item()) > 0
        # Barr: one-pass refresh against barr_simple_multi (container by container: barr_simple) + a fresh engine
        cols = [(K.to_device(ev["true_energy"]), K.to_device(ev["true_coszen"]), K.to_device(ev["nu_flux"]),
                 K.to_device(ev["nu_flux"] * 0.7)) for ev in wl.events]
        c = synthetic.DeviceState(wl, compact=True, index16=index16)
        c.enable_barr(cols)
        outs = [torch.empty((e.numel(), 2), dtype=torch.float64, device=e.device) for e, _, _, _ in cols]
        sets = K.barr_sets([col + (ev["nubar"], out) for col, ev, out in zip(cols, wl.events, outs)])
        ps = (1.03, 0.97, 0.04, 0.3, -0.2)
        K.barr_simple_multi(sets, *ps)
        for (e, cz, nu, nub), ev, out in zip(cols, wl.events, outs):
            assert torch.equal(out, K.barr_simple(e, cz, nu, nub, ev["nubar"], *ps))
        c.update_flux_barr(*ps)
        c.accumulate(p)
        d = fresh([o.cpu().numpy() for o in outs], compact=True, index16=index16)
        for wc, wd in zip(c._wflux, d._wflux):
            assert torch.equal(wc, wd)
        assert torch.equal(c.ws.limbs, d.ws.limbs), index16
    # flux on the calc grid: the per-container tables are formed one launch per 16 containers
    rs = np.random.RandomState(8)
    new_nodes = [ev["nu_flux_nodes"] * (0.7 + 0.6 * rs.rand(1, 2)) for ev in wl.events]
    e = synthetic.DeviceState(wl, compact=True, node_flux=True)
    for i, f in enumerate(new_nodes):
        e.update_flux_nodes(i, K.to_device(f))
    e.accumulate(p)
    f = fresh(new_nodes, compact=True, node_flux=True)
    assert torch.equal(e.ws.limbs, f.ws.limbs)
    assert torch.equal(e._own_tables, f._own_tables)
    assert int(e.ws.limbs[17:].abs().sum().item()) > 0


def test_weight_chain_multi_past_its_group():
    """`pisa_hip_weight_chain_multi` (24 sets per launch) for 25 and 49 containers, every shape of the chain
    (reset / -> osc / -> aeff / -> osc -> aeff), empty sets at 23, 24 and last: w0 * ((f_e p_e) + (f_mu p_mu)) *
    (aeff * scale) in numpy, bit for bit (the kernels are built without contraction)"""
    from pisa_amd import kernels as K

    rs = np.random.RandomState(9)
    for n_sets in (25, 49):
        items, want = [], []
        for k in range(n_sets):
            n = 0 if k in (23, 24, n_sets - 1) else int(rs.randint(1, 3000))
            w0, flux, pe, pmu, aeff = rs.rand(n), rs.rand(n, 2), rs.rand(n), rs.rand(n), rs.rand(n)
            scale = 1.0 + rs.rand()
            shape = k % 4
            w = w0.copy()
            if shape in (1, 3):
                w = w * ((flux[:, 0] * pe) + (flux[:, 1] * pmu))
            if shape in (2, 3):
                w = w * (aeff * scale)
            want.append(w)
            dev = [K.to_device(x) for x in (w0, flux, pe, pmu, aeff)]
            items.append((dev[0], dev[1] if shape in (1, 3) else None, dev[2], dev[3],
                          dev[4] if shape in (2, 3) else None, scale))
        block, views = K.weight_chain_multi(items)
        assert block.numel() == sum(len(w) for w in want)
        for k, (v, w) in enumerate(zip(views, want)):
            assert np.array_equal(v.cpu().numpy(), w), (n_sets, k)


# ------------------------------------------------------------------ f. a config pipeline with 26 outputs
def test_event_pipeline_with_26_outputs_replays_the_stage_protocol(tmp_path, oracle):
    """example_hip.cfg with 26 output_names (flux.barr_simple in one `barr_simple_multi` call, the fused engine
    past its first group): the Stage protocol and the replay plan give the same maps, errors and metrics bit for
    bit over osc, aeff and flux moves, and both meet the oracle's gate of the 12-output pipeline"""
    from pisa_amd.core.pipeline import Pipeline
    from pisa_amd.utils.resources import find_resource
    from tests.test_gpu_pipeline import _oracle_event_pipeline, _scan

    names = names_for(26)
    text = open(find_resource("settings/pipeline/example_hip.cfg")).read()
    old = [ln for ln in text.splitlines() if ln.startswith("output_names")]
    assert len(old) == 1
    text = text.replace(old[0], "output_names = " + ", ".join(names))
    text = text.replace("param.n_events = 1.2e5", "param.n_events = %d" % (26 * 8000))
    cfg = tmp_path / "example_hip_26.cfg"
    cfg.write_text(text)
    pipe = Pipeline(str(cfg))
    maps = pipe.get_outputs()
    assert maps.names == list(names) and pipe["hist"].fused_last_eval
    data = sum(maps).fluctuate("poisson", random_state=0)
    points = [(42.3, 2.457e-3, 1.0, 0.0), (47.0, 2.6e-3, 1.4, 0.0), (44.0, 2.3e-3, 0.9, 0.05),
              (51.0, 2.5e-3, 0.9, -0.04)]
    slow = _scan(pipe, False, data, points)
    fast = _scan(pipe, True, data, points)
    assert pipe._plan is not None and pipe._plan._barr_ready
    for (l0, c0, h0, e0), (l1, c1, h1, e1) in zip(slow, fast):
        assert l0 == l1 and c0 == c1
        for x, y in zip(h0 + e0, h1 + e1):
            np.testing.assert_array_equal(x, y)
    t23, dm31, scale, didx = points[-1]
    ref_h, ref_e = _oracle_event_pipeline(oracle, pipe, flux_params=(1.0, 1.0, didx, 0.0, 0.0), theta23_deg=t23,
                                          aeff_scale=scale, dm31=dm31)
    for name, hist, err in zip(names, fast[-1][2], fast[-1][3]):
        np.testing.assert_allclose(hist, ref_h[name], rtol=1e-11, atol=1e-300, err_msg=name)
        np.testing.assert_allclose(err, ref_e[name], rtol=1e-11, atol=1e-300, err_msg=name)
    assert fast[-1][2][25].sum() > 0


# ------------------------------------------------------------------ g. generalized Poisson-gamma likelihood
def _gpllh_host(hist, sumw2, n_mc, adjust, data):
    """generalized_llh_params + eq. 91 per bin (tests/test_host_gpllh.py), with the rules of the device code
    (pseudo-weight for an empty bin, the Poisson branch when every container has more than 100 MC events, NaN -> 1,
    log(1e-300) below 1e-300)"""
    from tests.test_host_gpllh import eq91

    n_c, n_bins = hist.shape
    empty = ~(n_mc > 0)
    sw = np.where(empty, 0.001, hist)
    sw2 = np.where(empty, 0.001 * 0.001, sumw2)
    n = np.where(empty, 1.0, n_mc)
    mean, var_z = sw / n, sw2 / n
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = np.where(var_z != 0.0, mean / var_z, 1.0)
        alpha = np.where(var_z != 0.0, (n + adjust[:, None]) * ((mean * mean) / var_z), (n + adjust[:, None]) * 0.001)
    out, branches = np.empty(n_bins), set()
    for b in range(n_bins):
        k = int(data[b])
        if (n_mc[:, b] > 100.0).all():
            branches.add("poisson")
            W = 0.0
            for c in range(n_c):
                W += sw[c, b]
            out[b] = -W if k == 0 else k * np.log(W) - W - (k * np.log(k) - k)
            continue
        branches.add("mixture")
        m = np.isfinite(alpha[:, b]) & np.isfinite(beta[:, b])
        v = float(eq91(k, alpha[m, b], beta[m, b]))
        out[b] = np.log(v) if v > 1e-300 else np.log(1e-300)
    return out, branches


@pytest.mark.parametrize("n", [17, 33])
def test_generalized_poisson_llh_past_16_containers(n):
    """the fused gpllh tail over 17 and 33 containers (the goldens stop at 16) against eq. 91 in 40 digits on the
    engine's own maps, per bin and in total; several points per sweep equal point by point"""
    from pisa_amd import synthetic

    # (17 containers: no empty one, and enough events that some bins take the Poisson branch; 33: every bin mixes)
    wl = workload(names_for(n), n_per=80000 if n == 17 else 20000, empty=edges(n) if n == 33 else (), seed=17)
    st = synthetic.DeviceState(wl, compact=True)
    p = wl.osc_params(theta23_deg=45.0, dm31=2.4e-3)
    st.accumulate(p)
    st.finalize()
    t = st.ws.hist.sum(dim=0).cpu().numpy()
    st.set_data(np.floor(t * (40.0 / t.max())))
    n_mc, adjust = st.configure_gpllh()
    pts = [p, wl.osc_params(theta23_deg=42.0, dm31=2.5e-3), wl.osc_params(theta23_deg=48.5, dm31=2.3e-3)]
    one = []
    for q in pts:
        v = st.eval_host(q, "generalized_poisson_llh")
        st.check_status()
        per_bin = st._gpllh["per_bin"][0].cpu().numpy().copy()
        h, s2 = st.maps()
        want, branches = _gpllh_host(h, s2, n_mc, adjust, st.data.cpu().numpy())
        np.testing.assert_allclose(per_bin, want, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(v, want.sum(), rtol=1e-10)
        assert "mixture" in branches and (n == 33 or "poisson" in branches)
        one.append(v)
    assert st.eval_many(pts, "generalized_poisson_llh") == one
    st.check_status()


# ------------------------------------------------------------------ h. Fisher matrix
@pytest.mark.parametrize("n", [17, 33])
def test_fisher_many_past_the_first_group(n):
    """`fisher_many` on 17 and 33 container rows (one sweep for the 5 templates, scales per point and container)
    against the restatement of the reference's loop on the single-point maps, bit for bit"""
    from pisa_amd import synthetic
    from tests.test_gpu_fisher import _restatement

    wl = workload(names_for(n), empty=edges(n) if n == 33 else (), seed=19)
    st = synthetic.DeviceState(wl, compact=True)
    st.make_pseudo_data(wl.osc_params(), seed=0)
    assert st.sweep_capable()
    fid = dict(theta23_deg=42.0, dm31=2.457e-3, deltacp_deg=180.0)
    hi_lo = [("theta23_deg", 43.0, 41.07), ("dm31", 2.457e-3 + 5.5e-5, 2.457e-3 - 5.35e-5)]
    pts, pairs, dx, cur = [wl.osc_params(**fid)], [], [], dict(fid)
    for p, (k, hi, lo) in enumerate(hi_lo):
        for v in (hi, lo):
            cur[k] = v
            pts.append(wl.osc_params(**cur))
        pairs.append((2 + 2 * p, 1 + 2 * p))
        dx.append(hi - lo)
    base = np.array([c.scale for c in st.cont])
    scales = base[None, :] * (0.9 + 0.2 * np.random.RandomState(5).rand(len(pts), n))
    truth = st.data.cpu().numpy()
    res = st.fisher_many(pts, pairs, dx, scales=scales, truth=truth)
    assert res["sweeps"] == 1 and res["status"] == 0
    assert res["hist"].shape == (len(pts), n, st.n_bins)
    f, grads, ne, hist, d = _restatement(st, pts, scales, pairs, dx, truth)
    assert res["nonempty"] == ne[0].size
    assert np.array_equal(res["grad"].cpu().numpy(), grads)
    assert np.array_equal(res["totals"].cpu().numpy(), np.stack(hist))
    assert np.array_equal(res["matrix"].cpu().numpy(), f)
    np.testing.assert_allclose(res["pull"].cpu().numpy(), d, rtol=1e-12, atol=1e-300)
    assert res["hist"][:, 16:].sum() > 0
