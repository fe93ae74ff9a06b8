"""The accumulate plan (`pisa_hip_hist_plan_*`, `pisa_hip_reweight_hist_planned`): the list of 256-event blocks that can
deposit is exactly what the index column says, the planned sweep leaves the same raw limbs and the same status word as
`pisa_hip_reweight_hist[_acc]` -- both equal to the exact sums of hand-built cases --, a stale plan is refused, and an
engine returns the same bits through every path (one call / separate calls, planned / un-planned, idle events resident
/ dropped).

Hand-built containers in the 16-bit index form: dragon binning (128 bins, LDS accumulators), a 4 x 4 calc grid, gather
tables (P_e, P_mu) = (1, 0) and flux pairs (w, 0) with scale 1, so an event's weight is w exactly; w is an integer in
1..7, so a deposit is w << 20 (and w^2 << 20) units of limb 3 and nothing else (LSB of the format 2^-116, limb j at
2^(32 j - 116)): the expected limbs are integer sums, no rounding anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_BINS, N_NODES, NL = 128, 16, 6
IDLE = 0xFFFF
PATTERNS = ("idle", "all", "alternating", "first", "last", "single", "node_out")
COUNTS = (1, 255, 256, 257, 4096 - 1, 4096 + 1, 16 * 256 * 3 + 5)


def _lib():
    from pisa_amd import _lib

    return _lib


def _binnings():
    L = _lib()
    from pisa_amd import synthetic

    d = synthetic.DRAGON
    return L.make_binning([0.0, -1.0], [1.0, 1.0], [4, 4]), L.make_binning(d["mins"], d["maxs"], d["nbins"])


def _blocks_of(pattern, n_blocks):
    if isinstance(pattern, tuple):                    # ("spread", k): k depositing blocks, every third one
        return list(range(0, n_blocks, 3))[: pattern[1]]
    return {"idle": [], "all": list(range(n_blocks)), "alternating": list(range(0, n_blocks, 2)), "first": [0],
            "last": [n_blocks - 1], "single": [n_blocks // 2], "node_out": [n_blocks // 2]}[pattern]


def _columns(n, pattern, nan=None):
    """index words [n_pad], flux pairs [n_pad, 2] of one container; nan: "idle" / "dep" puts a NaN pair into an idle /
    a depositing event (the valid-bin, node-0xffff event of "node_out")"""
    n_blocks = (n + 255) // 256
    n_pad = 256 * n_blocks
    e = np.arange(n_pad)
    bins = np.full(n_pad, IDLE, np.uint32)
    nodes = np.full(n_pad, IDLE, np.uint32)
    for b in _blocks_of(pattern, n_blocks):
        lo, hi = 256 * b, min(256 * b + 256, n)
        if pattern in ("single", "node_out"):
            lo = min(lo + 77, hi - 1)
            hi = lo + 1
        bins[lo:hi] = e[lo:hi] % N_BINS
        nodes[lo:hi] = IDLE if pattern == "node_out" else e[lo:hi] % N_NODES
    # idle events keep a node and a non-zero flux pair: only the bin half decides
    nodes[:n] = np.where(bins[:n] == IDLE, e[:n] % N_NODES, nodes[:n])
    idx = nodes | (bins << 16)
    idx[n:] = 0xFFFFFFFF
    flux = np.zeros((n_pad, 2))
    flux[:n, 0] = 1 + e[:n] % 7
    if nan is not None:
        live = np.flatnonzero(bins[:n] != IDLE)
        idle = np.flatnonzero(bins[:n] == IDLE)
        listed = np.isin(idle // 256, live // 256)     # an idle event of a block the sweep reads, if there is one
        at = (idle[listed] if listed.any() else idle)[-1] if nan == "idle" else live[-1]
        flux[at] = np.nan
    return idx.astype(np.uint32), flux


def _expected(idx, flux, n):
    """(limbs [N_BINS, 2, NL] int64, listed blocks) of one container from its columns"""
    bins, nodes = idx[:n] >> 16, idx[:n] & 0xFFFF
    w = np.where(nodes == IDLE, 0, np.nan_to_num(flux[:n, 0])).astype(np.int64)
    ok = bins != IDLE
    limbs = np.zeros((N_BINS, 2, NL), np.int64)
    np.add.at(limbs[:, 0, 3], bins[ok], w[ok] << 20)
    np.add.at(limbs[:, 1, 3], bins[ok], (w[ok] * w[ok]) << 20)
    marked = ((idx >> 16) != IDLE).reshape(-1, 256).any(axis=1)
    return limbs, np.flatnonzero(marked).astype(np.int32)


class _Launch:
    """containers (n, pattern) on the device, their plan, and the two calls"""

    def __init__(self, spec, nan=None):
        L = _lib()
        from pisa_amd import kernels as K

        self.L, self.K, self.lib = L, K, L.lib()
        self.grid, self.outb = _binnings()
        self.keep, self.cols = [], []
        self.cont = (L.Container * len(spec))()
        for c, (n, pattern) in enumerate(spec):
            idx, flux = _columns(n, pattern, nan[c] if nan else None)
            self.cols.append((idx, flux, n))
            wq = np.ascontiguousarray(flux.reshape(-1, 64, 4, 2).transpose(0, 2, 1, 3))   # [block][k][lane][2]
            d_idx = torch.from_numpy(idx.view(np.int32)).cuda()
            d_wq = torch.from_numpy(wq).cuda()
            self.keep += [d_idx, d_wq]
            self.cont[c].n_events = n
            self.cont[c].d_node_bin16, self.cont[c].d_weighted_flux_q = d_idx.data_ptr(), d_wq.data_ptr()
            self.cont[c].flav, self.cont[c].nubar, self.cont[c].scale = c % 3, 1 if c % 2 == 0 else -1, 1.0
        tab = np.zeros((2, 3, N_NODES, 2))
        tab[..., 0] = 1.0
        self.tab = torch.from_numpy(tab).cuda()
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.n_cont = len(spec)
        torch.cuda.synchronize()
        self.plan = C.c_void_p()
        L.check(self.lib.pisa_hip_hist_plan_create(self.cont, self.n_cont, C.byref(self.grid), C.byref(self.outb),
                                                   C.byref(self.plan), K._stream()))

    def close(self):
        self.lib.pisa_hip_hist_plan_destroy(self.plan)
        self.plan = None

    def info(self, c):
        nb, nd, wg = C.c_int32(), C.c_int32(), C.c_int32()
        self.L.check(self.lib.pisa_hip_hist_plan_info(self.plan, c, C.byref(nb), C.byref(nd), C.byref(wg), None))
        blocks = np.full(max(nd.value, 1), -1, np.int32)
        self.L.check(self.lib.pisa_hip_hist_plan_info(self.plan, c, None, None, None, blocks.ctypes.data_as(C.c_void_p)))
        return nb.value, wg.value, blocks[: nd.value]

    def limbs(self, fill=0):
        return torch.full((self.n_cont, N_BINS, 2, NL), fill, dtype=torch.int64, device="cuda")

    def run(self, planned, limbs, clear_first=True, n_cont=None, cont=None, status=0):
        """status of the call; limbs are written in place, the device status word (`status` before the call) is in
        `self.status`"""
        self.status.fill_(status)
        a = (cont if cont is not None else self.cont, self.n_cont if n_cont is None else n_cont, C.byref(self.grid), None, None,
             self.K._ptr(self.tab), C.byref(self.outb), self.K._ptr(limbs), self.K._ptr(self.status))
        if planned:
            rc = self.lib.pisa_hip_reweight_hist_planned(self.plan, *a, 1 if clear_first else 0, self.K._stream())
        else:
            fn = self.lib.pisa_hip_reweight_hist if clear_first else self.lib.pisa_hip_reweight_hist_acc
            rc = fn(*a, self.K._stream())
        torch.cuda.synchronize()
        return rc

    def expected(self):
        return np.stack([_expected(*col)[0] for col in self.cols])


def _check_lists(la):
    for c, (idx, flux, n) in enumerate(la.cols):
        n_blocks, wg, blocks = la.info(c)
        want = _expected(idx, flux, n)[1]
        assert n_blocks == (n + 255) // 256
        assert np.array_equal(blocks, want), (c, blocks, want)
        assert (wg == 0) == (len(want) == 0)          # no workgroup for a container that deposits nothing
        assert wg <= max(1, (len(want) + 15) // 16)   # at least one sweep (16 blocks) per workgroup


def _check_limbs(la, want_status=0):
    """planned == un-planned == exact, with and without the clear; the status word of both paths"""
    want = la.expected()
    a, b = la.limbs(fill=-7), la.limbs(fill=-7)       # (clear_first: whatever the limbs held is gone)
    assert la.run(True, a) == 0
    sa = int(la.status.item())
    assert la.run(False, b) == 0
    sb = int(la.status.item())
    assert sa == sb == want_status
    assert torch.equal(a, b)
    if want_status == 0:
        assert np.array_equal(a.cpu().numpy(), want)
        assert la.run(True, a, clear_first=False) == 0 and la.run(False, b, clear_first=False) == 0
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), 2 * want)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_listed_blocks_and_limbs_of_one_container(n, pattern):
    la = _Launch([(n, pattern)])
    try:
        assert la.plan.value
        _check_lists(la)
        if pattern == "node_out":   # listed although it deposits nothing: the bin half alone decides
            assert len(la.info(0)[2]) == 1 and not la.expected().any()
        _check_limbs(la)
    finally:
        la.close()


@pytest.mark.parametrize("outer", ["all", "alternating", "last", "single"])
def test_three_containers_with_an_idle_one_in_the_middle(outer):
    la = _Launch([(16 * 256 * 3 + 5, outer), (4096 + 1, "idle"), (257, outer)])
    try:
        _check_lists(la)
        assert la.info(1)[1] == 0
        _check_limbs(la)
    finally:
        la.close()


@pytest.mark.parametrize("k", [1, 15, 16, 17])
def test_fewer_depositing_blocks_than_a_workgroup_has_wavefronts(k):
    la = _Launch([(16 * 256 * 3 + 5, ("spread", k)), (4096 - 1, ("spread", 1))])
    try:
        _check_lists(la)
        assert len(la.info(0)[2]) == k
        _check_limbs(la)
    finally:
        la.close()


def test_wavefronts_advance_through_several_listed_blocks():
    """more than 2 x 16 x (workgroups of a launch) listed blocks in one container: every wavefront takes a second and
    most a third block of the list -- the in-loop look-up of the next block number and of the one after it"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_dep = 2 * 16 * cus + 40
    la = _Launch([(256 * 2 * n_dep - 251, "alternating"), (257, "all")])
    try:
        _check_lists(la)
        n_blocks, wg, blocks = la.info(0)
        assert len(blocks) == n_dep and 16 * wg * 2 < n_dep
        _check_limbs(la)
    finally:
        la.close()


def test_more_containers_than_one_launch_takes():
    pats = ["alternating", "all", "idle", "single", "last", "first"]
    la = _Launch([((257, 255, 4097, 1)[c % 4], pats[c % 6]) for c in range(17)])
    try:
        _check_lists(la)
        _check_limbs(la)
    finally:
        la.close()


def test_all_containers_idle():
    la = _Launch([(4097, "idle"), (255, "idle"), (1, "idle")])
    try:
        _check_lists(la)
        _check_limbs(la)     # zero with the clear
        held = la.limbs(fill=5)
        assert la.run(True, held, clear_first=False) == 0 and int(la.status.item()) == 0
        assert bool((held == 5).all())
    finally:
        la.close()


@pytest.mark.parametrize("pattern,nan,status", [("alternating", "idle", 0), ("alternating", "dep", 1), ("node_out", "dep", 1),
                                                ("node_out", "idle", 0)])
def test_status_word_is_unchanged(pattern, nan, status):
    la = _Launch([(4097, "all"), (4097, pattern)], nan=[None, nan])
    try:
        _check_lists(la)
        _check_limbs(la, want_status=status)
    finally:
        la.close()


def test_stale_plans_are_refused():
    la = _Launch([(4097, "alternating"), (257, "all"), (255, "first")])
    try:
        L = la.L
        limbs = la.limbs()
        assert la.run(True, limbs, n_cont=2) == -1     # PISA_HIP_ERR_INVALID
        changed = (L.Container * 3)(*la.cont)
        changed[1].n_events = 256
        assert la.run(True, limbs, cont=changed) == -1
        assert la.run(True, limbs) == 0
    finally:
        la.close()


def test_planned_call_validates_by_itself():
    """a binning or calc grid of another size than the plan's, a container without its index column, a flavour that
    does not exist: refused, with the caller's limbs and status word as they were"""
    la = _Launch([(4097, "alternating"), (257, "all")])
    try:
        L = la.L
        limbs = la.limbs(fill=5)
        grid, outb = la.grid, la.outb

        def refused(cont=None):
            rc = la.run(True, limbs, cont=cont, status=0x40)     # (a bit no kernel sets)
            return rc == -1 and bool((limbs == 5).all()) and int(la.status.item()) == 0x40   # PISA_HIP_ERR_INVALID

        la.outb = L.make_binning([0.0, -1.0], [1.0, 1.0], [8, 8])      # 64 bins, the plan's binning has 128
        assert refused()
        la.outb, la.grid = outb, L.make_binning([0.0, -1.0], [1.0, 1.0], [4, 5])   # 20 nodes, the plan's grid 16
        assert refused()
        la.grid = grid
        stripped = (L.Container * 2)(*la.cont)
        stripped[1].d_node_bin16 = None
        assert refused(stripped)
        flavour = (L.Container * 2)(*la.cont)
        flavour[0].flav = 3
        assert refused(flavour)
        assert la.run(True, limbs) == 0 and np.array_equal(limbs.cpu().numpy(), la.expected())
    finally:
        la.close()


def test_planned_launch_records_the_profile_events():
    """`pisa_hip_profile_events`: the planned call records the pair around its launch (bench.py times the sweep with it)"""
    la = _Launch([(4097, "all"), (257, "alternating")])
    try:
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(); stop.record()          # materialise the handles
        torch.cuda.synchronize()
        empty = start.elapsed_time(stop)
        assert empty < 1.0                     # back to back: nothing in between
        assert la.lib.pisa_hip_profile_events(start.cuda_event, stop.cuda_event) == 0
        try:
            assert la.run(True, la.limbs()) == 0
        finally:
            assert la.lib.pisa_hip_profile_events(None, None) == 0
        dt = start.elapsed_time(stop)
        assert dt > 0.0 and dt != empty        # recorded again, with the launch in between
        assert la.run(True, la.limbs()) == 0   # disabled: the pair keeps its last recording
        assert start.elapsed_time(stop) == dt
    finally:
        la.close()


# ---------------------------------------------------------------------------------------------- engine level
def _engines(wl, node_flux=False):
    from pisa_amd import synthetic

    kw = dict(compact=True, node_flux=node_flux)
    e = {"one_call": synthetic.DeviceState(wl, **kw), "separate": synthetic.DeviceState(wl, **kw),
         "unplanned": synthetic.DeviceState(wl, **kw), "dropped": synthetic.DeviceState(wl, drop_unbinned=True, **kw)}
    e["separate"].one_call = False
    e["unplanned"].hist_plan = False
    return e


def _same_everywhere(engines, points):
    ref = None
    for p in points:
        got = {}
        for name, st in engines.items():
            v = st.eval_host(p)
            st.check_status()
            got[name] = (v, st.maps()[0].tobytes(), st.maps()[1].tobytes())
        ref = got["unplanned"]
        assert ref[0] == ref[0] and any(ref[1])
        for name, g in got.items():
            assert g[0] == ref[0], (name, g[0], ref[0])
            assert g[1] == ref[1] and g[2] == ref[2], name
    return ref[0]


@pytest.mark.parametrize("n_events", [3000, 40000])
def test_engine_paths_agree_bit_for_bit(n_events):
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=n_events, grid=(60, 40), out_binning="dragon", seed=5)
    eng = _engines(wl)
    data = eng["unplanned"].make_pseudo_data(wl.osc_params(), seed=0)
    for st in eng.values():
        st.set_data(data)
    pts = [wl.osc_params(theta23_deg=t, dm31=d) for t, d in ((41.0, 2.4e-3), (45.0, 2.5e-3), (49.5, 2.3e-3))]
    v0 = _same_everywhere(eng, pts)
    sep = eng["separate"]
    assert sep._hist_plan is not None and sep._hist_plan["handle"] is not None
    assert eng["unplanned"]._hist_plan is None and eng["unplanned"]._evaluator is None
    assert eng["one_call"]._evaluator is not None
    # every event the dropped engine keeps lies in a listed block; the resident order leaves whole blocks idle
    lib = _lib().lib()
    blocks = listed = 0
    for c in range(len(sep.cont)):
        nb, nd = C.c_int32(), C.c_int32()
        _lib().check(lib.pisa_hip_hist_plan_info(sep._hist_plan["handle"], c, C.byref(nb), C.byref(nd), None, None))
        assert nb.value == (sep.cont[c].n_events + 255) // 256
        assert (eng["dropped"].cont[c].n_events + 255) // 256 <= nd.value <= nb.value
        blocks, listed = blocks + nb.value, listed + nd.value
    if n_events == 40000:
        assert listed < blocks
    handle = sep._hist_plan["handle"]
    i = 4
    new_flux = K.to_device(wl.events[i]["nu_flux"] * np.array([0.9, 1.2]))
    for st in eng.values():
        st.update_flux(i, new_flux)
    v1 = _same_everywhere(eng, pts)
    assert v1 != v0 and sep._hist_plan["handle"] is handle
    for st in eng.values():
        st.set_scale(wl.names[2], 1.7 * st.cont[2].scale)
    v2 = _same_everywhere(eng, pts)
    assert v2 != v1 and sep._hist_plan["handle"] is handle
    sep.containers_changed()
    _same_everywhere(eng, pts)
    assert sep._hist_plan["handle"] is not handle and sep._hist_plan["gen"] == sep._cont_gen
    for st in eng.values():
        st.close()


def test_engine_paths_agree_with_flux_on_the_nodes():
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=40000, grid=(60, 40), out_binning="dragon", seed=6)
    g = wl.grid
    ee, cc = np.meshgrid(g.energy, g.coszen, indexing="ij")
    rs = np.random.RandomState(2)
    for ev in wl.events:
        f_mu = 1e4 * ee ** -2.7 * (1 + 0.5 * cc ** 2) * (0.8 + 0.4 * rs.rand(*ee.shape))
        fn = np.stack([f_mu * (0.5 - 0.2 * cc), f_mu], axis=-1).reshape(-1, 2)
        node = K.event_indices([K.to_device(np.log(ev["true_energy"])), K.to_device(ev["true_coszen"])], g.binning).cpu().numpy()
        assert node.min() >= 0
        ev["nu_flux"], ev["nu_flux_nodes"] = fn[node], fn
    eng = _engines(wl, node_flux=True)
    data = eng["unplanned"].make_pseudo_data(wl.osc_params(), seed=0)
    for st in eng.values():
        st.set_data(data)
    pts = [wl.osc_params(theta23_deg=t) for t in (41.0, 45.0, 49.5)]
    v0 = _same_everywhere(eng, pts)
    handle = eng["one_call"]._hist_plan["handle"]
    assert handle is not None
    for st in eng.values():
        st.set_scale(wl.names[1], 0.6 * st.cont[1].scale)
    assert _same_everywhere(eng, pts) != v0 and eng["one_call"]._hist_plan["handle"] is handle
    for st in eng.values():
        st.close()


def test_no_plan_beyond_the_lds_accumulators():
    """fine3d (4 800 bins): the window path keeps to the existing calls"""
    from pisa_amd import kernels as K
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=40000, grid=(60, 40), out_binning="fine3d", seed=7)
    a, b = synthetic.DeviceState(wl, compact=True), synthetic.DeviceState(wl, compact=True)
    b.hist_plan = False
    plan = C.c_void_p(1)
    _lib().check(_lib().lib().pisa_hip_hist_plan_create(a._cont_arr, len(a._cont_arr), C.byref(a.grid.binning),
                                                        C.byref(a.out_binning), C.byref(plan), K._stream()))
    assert not plan.value
    p = wl.osc_params(theta23_deg=44.0)
    a.accumulate(p)
    b.accumulate(p)
    assert a._hist_plan is not None and a._hist_plan["handle"] is None
    assert torch.equal(a.ws.limbs, b.ws.limbs) and bool((a.ws.limbs != 0).any())
    a.check_status()
