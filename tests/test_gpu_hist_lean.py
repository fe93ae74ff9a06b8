"""The planned sweep's lean body (`hist_planned_kernel`, csrc/hist_planned.hip: what `pisa_hip_reweight_hist_planned`
launches): blocks the plan did not mark run without the 0xffff guards, a half-sweep whose weights all pass ONE combined
range test (2^-26 <= w < 2^38: w and w w both in the fast range of `deposit_units`) deposits without a branch, anything
else takes the shared per-deposit code.  Whatever path a sweep takes, the limbs are the exact sums and the status word
says whether a weight was refused -- and they are the limbs of `pisa_hip_reweight_hist` (no plan, generic body).

Hand-built containers in the 16-bit index form as in tests/test_gpu_hist_plan.py: gather tables (P_e, P_mu) = (1, 0),
flux pairs (w, 0), scale 1, so the kernel's weight of an event is w itself, bit for bit (an event outside the calc grid,
node 0xffff, gets P = 0 and weight 0).  Event e of block b sits in lane (e % 256) // 4, position e % 4 of the lane's quad;
events 0, 1 of the quads form the first half-sweep, 2, 3 the second.  Expected limbs: Python integers
(tests/limb_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import limb_cases as LC

pytestmark = pytest.mark.gpu

N_NODES = 16
IDLE = 0xFFFF
LO, HI = 2.0 ** -26, 2.0 ** 38          # the combined test's range [LO, HI)


def _lean_fast(w):
    """what the combined test stands for: w and fl(w w) both take the branch-free form"""
    return LC.kernel_is_fast(w) and LC.kernel_is_fast(np.float64(w) * np.float64(w))


def _largest_lds_bins():
    from pisa_amd import _lib

    lib = _lib.lib()
    n = 1
    while lib.pisa_hip_hist_window_bins(2 * n) == 0:
        n *= 2
    lo, hi = n, 2 * n          # window_bins(lo) == 0 < window_bins(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.pisa_hip_hist_window_bins(mid) == 0 else (lo, mid)
    return lo


class _Cont:
    """one container: per event a weight, a bin (-1: outside the binning) and a node (-1: outside the calc grid)"""

    def __init__(self, w, bins, nodes=None):
        self.w = np.asarray(w, dtype=np.float64)
        self.bins = np.asarray(bins, dtype=np.int64)
        self.nodes = np.arange(len(self.w)) % N_NODES if nodes is None else np.asarray(nodes, dtype=np.int64)
        assert len(self.w) == len(self.bins) == len(self.nodes)

    def columns(self):
        n = len(self.w)
        n_pad = 256 * ((n + 255) // 256)
        idx = np.full(n_pad, 0xFFFFFFFF, np.uint32)
        idx[:n] = (np.where(self.nodes < 0, IDLE, self.nodes) | (np.where(self.bins < 0, IDLE, self.bins) << 16)).astype(np.uint32)
        flux = np.zeros((n_pad, 2))
        flux[:n, 0] = self.w
        return idx, np.ascontiguousarray(flux.reshape(-1, 64, 4, 2).transpose(0, 2, 1, 3))   # [block][k][lane][2]

    def expected(self, n_bins):
        """((H, S) exact sums of units, refused): a refused quantity (NaN, |x| >= 2^76) deposits nothing and sets the
        status word; the other quantity of the event and every other event are summed as usual"""
        w = np.where(self.nodes < 0, 0.0, self.w)
        with np.errstate(all="ignore"):
            w2 = w * w
        live = self.bins >= 0
        ok1 = np.array([LC.accepted(x) for x in w])
        ok2 = np.array([LC.accepted(x) for x in w2])
        H, S = LC.exact_sums(np.where(ok1 & ok2, w, 0.0), np.where(live & ok1 & ok2, self.bins, -1), n_bins)
        for x, x2, b, a1, a2 in zip(w.tolist(), w2.tolist(), self.bins.tolist(), ok1, ok2):
            if b >= 0 and not (a1 and a2):
                H[b] += LC.units(x) if a1 else 0
                S[b] += LC.units(x2) if a2 else 0
        return (H, S), bool((live & ~(ok1 & ok2)).any())


class _Launch:
    def __init__(self, conts, n_bins):
        from pisa_amd import _lib as L
        from pisa_amd import kernels as K

        self.L, self.K, self.lib = L, K, L.lib()
        self.conts, self.n_bins, self.n_cont = conts, n_bins, len(conts)
        self.grid = L.make_binning([0.0, -1.0], [1.0, 1.0], [4, 4])
        self.outb = L.make_binning([0.0], [1.0], [n_bins])
        assert self.lib.pisa_hip_hist_window_bins(n_bins) == 0
        self.keep = []
        self.cont = (L.Container * self.n_cont)()
        for c, ct in enumerate(conts):
            idx, wq = ct.columns()
            d_idx, d_wq = torch.from_numpy(idx.view(np.int32)).cuda(), torch.from_numpy(wq).cuda()
            self.keep += [d_idx, d_wq]
            self.cont[c].n_events = len(ct.w)
            self.cont[c].d_node_bin16, self.cont[c].d_weighted_flux_q = d_idx.data_ptr(), d_wq.data_ptr()
            self.cont[c].flav, self.cont[c].nubar, self.cont[c].scale = c % 3, 1 if c % 2 == 0 else -1, 1.0
        tab = np.zeros((2, 3, N_NODES, 2))
        tab[..., 0] = 1.0
        self.tab = torch.from_numpy(tab).cuda()
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.plan = C.c_void_p()
        L.check(self.lib.pisa_hip_hist_plan_create(self.cont, self.n_cont, C.byref(self.grid), C.byref(self.outb),
                                                   C.byref(self.plan), K._stream()))
        assert self.plan.value

    def close(self):
        self.lib.pisa_hip_hist_plan_destroy(self.plan)
        self.plan = None

    def run(self, planned):
        """(raw limbs, status word) of one call"""
        limbs = torch.full((self.n_cont, self.n_bins, 2, LC.NL), -3, dtype=torch.int64, device="cuda")
        self.status.zero_()
        a = (self.cont, self.n_cont, C.byref(self.grid), None, None, self.K._ptr(self.tab), C.byref(self.outb),
             self.K._ptr(limbs), self.K._ptr(self.status))
        if planned:
            rc = self.lib.pisa_hip_reweight_hist_planned(self.plan, *a, 1, self.K._stream())
        else:
            rc = self.lib.pisa_hip_reweight_hist(*a, self.K._stream())
        torch.cuda.synchronize()
        assert rc == 0
        return limbs, int(self.status.item())

    def listed(self, c):
        nd = C.c_int32()
        self.L.check(self.lib.pisa_hip_hist_plan_info(self.plan, c, None, C.byref(nd), None, None))
        blocks = np.full(max(nd.value, 1), -1, np.int32)
        self.L.check(self.lib.pisa_hip_hist_plan_info(self.plan, c, None, None, None, blocks.ctypes.data_as(C.c_void_p)))
        return blocks[: nd.value]


def _check(conts, n_bins, want_status=None):
    la = _Launch(conts, n_bins)
    try:
        exp = [ct.expected(n_bins) for ct in conts]
        status = 1 if any(r for _, r in exp) else 0
        if want_status is not None:
            assert status == want_status      # (the case holds what it was built to hold)
        for c, ct in enumerate(conts):         # the list holds block NUMBERS: the sweep's mark is not part of them
            want = np.flatnonzero((np.pad(ct.bins, (0, -len(ct.bins) % 256), constant_values=-1) >= 0).reshape(-1, 256).any(axis=1))
            assert np.array_equal(la.listed(c), want.astype(np.int32))
        a, sa = la.run(True)
        b, sb = la.run(False)
        assert sa == sb == status
        assert torch.equal(a, b)               # the same digits were deposited: raw limbs, not only their value
        assert np.array_equal(LC.canonical(a).cpu().numpy(), LC.sums_to_limbs([s for s, _ in exp]))
    finally:
        la.close()


def _fast_weights(n, seed):
    """positive, exponents -20 .. 33: w and w w far inside the fast range"""
    rs = np.random.RandomState(seed)
    m = (rs.randint(0, 1 << 26, size=n).astype(np.int64) << 26) | rs.randint(0, 1 << 26, size=n) | (1 << 52)
    return np.array([LC.mant(int(mi), int(ei)) for mi, ei in zip(m, rs.randint(-20, 34, size=n))])


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("n_dep", [1, 63, 255, 256, 257, 511, 1025])
def test_topped_up_block_has_idle_lanes_in_every_position(n_dep):
    """n_dep depositing events behind one idle block: the full blocks are unmarked, the topped-up one is marked -- one
    event in it (a whole idle half-quad in lane 0), 63 (lane 15 ends after three events), 255 (one idle event), none"""
    w = np.concatenate([np.full(256, 3.0), _fast_weights(n_dep, n_dep)])
    bins = np.concatenate([np.full(256, -1), np.arange(n_dep) % 30])
    _check([_Cont(w, bins)], 30, want_status=0)


def test_one_event_outside_the_calc_grid_in_the_middle_of_the_list():
    n = 256 * 5
    w = _fast_weights(n, 3)
    nodes = np.arange(n) % N_NODES
    nodes[256 * 2 + 4 * 21 + 2] = -1                    # block 2 of 0 .. 4, lane 21, third event of its quad
    _check([_Cont(w, np.arange(n) % 30, nodes)], 30, want_status=0)


def test_weight_families_in_twelve_containers():
    fam = LC.weight_families()
    conts = []
    for k, name in enumerate(LC.FAMILY_ORDER):
        w = fam[name]
        bins = np.full(len(w), 7) if name in LC.ONE_BIN else 5 * (k % 6) + np.arange(len(w)) % 5
        conts.append(_Cont(w, bins))
    assert len(conts) == 12
    # "fast_only" fills whole blocks that no wavefront leaves the branch-free path in
    assert all(_lean_fast(x) for x in fam["fast_only"]) and len(fam["fast_only"]) >= 4 * 256
    _check(conts, 30, want_status=0)


EDGES = {
    "below_lo": (float(np.nextafter(LO, 0.0)), True, False),      # w fast, w w just below 2^-52: not
    "at_lo": (LO, True, True),
    "below_hi": (float(np.nextafter(HI, 0.0)), True, True),       # w w just below 2^76
    "bottom_of_w": (2.0 ** -52, True, False),
    "below_w": (float(np.nextafter(2.0 ** -52, 0.0)), False, False),
    "negative": (-1.5, False, True),                              # w w fast, w not
    "negative_small": (-(2.0 ** -40), False, False),
    "zero": (0.0, False, False),
    "minus_zero": (-0.0, False, False),
}


def test_the_edge_table_says_what_it_means():
    """(no kernel: the combined range is exactly where w and w w are both fast, on every edge value and on a scan of
    all exponents with the smallest, the largest and a middle mantissa)"""
    for name, (w, f1, f2) in EDGES.items():
        assert (LC.kernel_is_fast(w), LC.kernel_is_fast(np.float64(w) * np.float64(w))) == (f1, f2), name
    for e in range(-140, 100):
        for m in ((1 << 52), LC.M_ONES, LC.M_ALT_A):
            for s in (1.0, -1.0):
                w = s * LC.mant(m, e)
                if LO <= w < HI:
                    assert _lean_fast(w), w          # inside the combined range: both fast (what the kernel relies on)
                elif LC.accepted(w * w):
                    assert not _lean_fast(w), w      # (and the range gives nothing away)


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("where", ["one_event_first_half", "one_event_second_half", "whole_lane", "every_lane"])
def test_one_weight_at_an_edge_of_the_combined_test(edge, where):
    """three unmarked blocks of fast weights; in the middle one the edge value sits in ONE event of ONE lane (the other
    63 lanes, and the lane's other events, are fast), in a lane's whole quad, or in one event of every lane"""
    n = 256 * 3
    w = _fast_weights(n, 11)
    x = EDGES[edge][0]
    at = {"one_event_first_half": [256 + 4 * 37 + 1], "one_event_second_half": [256 + 4 * 5 + 3],
          "whole_lane": [256 + 4 * 63 + k for k in range(4)], "every_lane": [256 + 4 * l + 2 for l in range(64)]}[where]
    w[at] = x
    assert sum(not _lean_fast(v) for v in w) == (0 if _lean_fast(x) else len(at))
    _check([_Cont(w, np.arange(n) % 128)], 128, want_status=0)


@pytest.mark.parametrize("bad", ["square_refused", "at_hi", "both_refused", "nan", "inf"])
@pytest.mark.parametrize("marked", [False, True])
def test_refused_weights_set_the_status_and_leave_the_other_sums(bad, marked):
    """|w| >= 2^38: the square is refused, w itself is deposited; |w| >= 2^76, NaN, Inf: neither -- in an unmarked block
    (the lean body's general half-sweep) and in a marked one (an idle event in the block: the guarded body)"""
    n = 256 * 3
    w = _fast_weights(n, 13)
    bins = np.arange(n) % 30
    x = {"square_refused": -(2.0 ** 50), "at_hi": HI, "both_refused": 2.0 ** 76, "nan": np.nan, "inf": np.inf}[bad]
    w[256 + 4 * 9 + 0] = x
    if marked:
        bins[256 + 4 * 40 + 1] = -1
    _check([_Cont(w, bins)], 30, want_status=1)


@pytest.mark.parametrize("n_bins", [1, 30, 128, "largest"])
def test_every_bin_count_with_lds_accumulators(n_bins):
    if n_bins == "largest":
        n_bins = _largest_lds_bins()
        assert n_bins == 682
    fam = LC.weight_families()
    w = np.concatenate([fam["fast_only"][:1024], fam["mixed"], _fast_weights(777, 5)])
    rs = np.random.RandomState(n_bins)
    bins = np.concatenate([np.arange(1024) % n_bins, rs.randint(0, n_bins, size=len(w) - 1024)])
    bins[-1] = bins[0] = n_bins - 1
    _check([_Cont(w, bins)], n_bins, want_status=0)


def test_three_containers_with_an_idle_one_in_the_middle():
    fam = LC.weight_families()
    a = _Cont(fam["fast_only"], np.arange(len(fam["fast_only"])) % 30)
    idle = _Cont(np.full(600, 2.5), np.full(600, -1))
    b = _Cont(fam["mixed"], np.arange(len(fam["mixed"])) % 29)
    _check([a, idle, b], 30, want_status=0)


def test_scale_changed_through_the_evaluator_between_two_evaluations():
    """the engine's one-call path (its evaluator holds the plan and the scales) against the un-planned calls, before
    and after `set_scale`: value and maps bit for bit"""
    from pisa_amd import synthetic

    wl = synthetic.Workload(n_events=3000, grid=(24, 16), out_binning="dragon", seed=9)
    one, ref = synthetic.DeviceState(wl, compact=True), synthetic.DeviceState(wl, compact=True)
    ref.hist_plan = False
    data = ref.make_pseudo_data(wl.osc_params(), seed=0)
    p = wl.osc_params(theta23_deg=47.0, dm31=2.45e-3)
    seen = []
    for step in range(2):
        got = []
        for st in (one, ref):
            st.set_data(data)
            if step == 1:
                st.set_scale(wl.names[1], 1.3 * st.cont[1].scale)
            v = st.eval_host(p)
            st.check_status()
            got.append((v, st.maps()[0].tobytes(), st.maps()[1].tobytes()))
        assert got[0] == got[1] and got[0][0] == got[0][0]
        seen.append(got[0])
    assert one._evaluator is not None and ref._evaluator is None
    assert seen[0] != seen[1]
    one.close()
    ref.close()
