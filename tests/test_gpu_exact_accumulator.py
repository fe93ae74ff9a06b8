"""The exact accumulator at its edges, in every kernel form.

DEPOSIT.  Each form of the fused kernel (`hist_accumulate_kernel<1|2|3|5|7>`, with and without LDS
accumulators, the LDS window with its global-atomic fallback, the two-window partitioned sweep), the
sweep kernel `hist_accumulate_multi_kernel<1..8>` and the generic histogram (MODE 0) is handed weights
whose BIT PATTERNS are chosen: `initial_weights` = the weight, weighted_aeff = 1, nu_flux = (1, 1), scale 1
and probability tables (P_e, P_mu) = (1, 0) written by hand, so every product of every form's weight chain
is by 1 or 0.  The limbs each form leaves must be, after carry normalisation, the digits of
    H = sum units(w),   S = sum units(fl(w w)),   units(x) = sign(x) floor(|x| 2^116)
computed in Python integers (`tests/limb_cases.py`, pinned on the CPU by `tests/test_host_limbs.py`), and
the maps H / 2^116, S / 2^116 correctly rounded.  No tolerance anywhere.  All forms equal one reference,
so all forms agree with each other.

Which launch a form reaches is asserted, not assumed: `_launch_mode` restates the choice of
`reweight_hist_impl` from the columns a container carries, `pisa_hip_hist_window_bins` says whether the
binning has LDS accumulators or a window, and `n_part` of a container whether it runs the partitioned sweep.

DECODE.  The accumulators of `test_limb_decoder_is_correctly_rounded_on_adversarial_accumulators` and the
limbs the deposit tests produce go through every fused tail (`finalize_metric_kernel<KIND, 1|4|16>`, its
multi-point form, `finalize_gpllh_kernel`), each of which numbers its items in its own way.

A weight whose fl(w w) rounds UP to 2^76 while |w| < 2^38 does not exist (tests/test_host_limbs.py shows the
square of the double below 2^38 rounds down); the probes are |w| = 2^38, +-inf and NaN."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import limb_cases as LC

pytestmark = pytest.mark.gpu

GRID = (16, 12)
NAN = float("nan")


# ---------------------------------------------------------------------------------- workloads
def _bin_centres(ob, flat):
    """regularised sample coordinates of the centres of the flat (C-order) bins `flat`"""
    nb = ob["nbins"]
    idx = np.unravel_index(np.asarray(flat, dtype=np.int64), nb)
    return [ob["mins"][k] + (idx[k] + 0.5) * (ob["maxs"][k] - ob["mins"][k]) / nb[k] for k in range(len(nb))]


_families = functools.lru_cache(maxsize=None)(LC.weight_families)


class _Case:
    """one synthetic workload: container c holds family FAMILY_ORDER[c] on bins of `bins`, plus three events per
    container that must deposit nothing (outside the calc grid, outside the binning, a NaN coordinate) and
    `n_idle` more outside the binning (what the partitioned order tops its partitions up with)"""

    def __init__(self, binning, bins, n_idle=0, families=LC.FAMILY_ORDER, seed=1):
        from pisa_amd import synthetic

        rs = np.random.RandomState(seed)
        fam = _families()
        names = synthetic.NAMES[:len(families)]
        wl = synthetic.Workload(n_events=len(names), grid=GRID, out_binning=binning, seed=0, names=names)
        ob, grid = wl.ob, wl.grid
        events, self.w0, self.ref_bins = [], [], []
        for c, (name, f) in enumerate(zip(names, families)):
            w = fam[f] if isinstance(f, str) else np.asarray(f, dtype=np.float64)
            n = len(w)
            b = np.full(n, bins[c % len(bins)]) if f in LC.ONE_BIN else np.array([bins[(i + c) % len(bins)] for i in range(n)])
            keep = 1 if f == "single" else 0      # the one-event container stays a one-event container
            if f == "fast_only" and not n_idle:
                keep = 1                          # ... and no event of this one leaves the fast path, not even with w = 0
            n_dead = 0 if keep else 3 + n_idle
            w = np.concatenate([w, np.full(n_dead, 2.0 ** 30)])
            w[n + 3:] = 1.0
            cols = [np.concatenate([col, np.full(n_dead, col[0] if n else 0.0)]) for col in _bin_centres(ob, b)]
            e = grid.energy[rs.randint(0, GRID[0], size=n + n_dead)].copy()
            cz = grid.coszen[rs.randint(0, GRID[1], size=n + n_dead)].copy()
            ref_b = np.concatenate([b, np.full(n_dead, -1)])
            if n_dead:
                e[n] = 5000.0                              # outside the calc grid, inside the binning
                cols[0][n + 1] = ob["maxs"][0] + 1.0       # outside the binning
                cols[-1][n + 2] = NAN                      # a NaN coordinate is outside too
                cols[0][n + 3:] = ob["mins"][0] - 1.0
            flav, nubar = synthetic.flav_nubar(name)
            events.append(dict(name=name, flav=flav, nubar=nubar, true_energy=e, true_coszen=cz,
                               nu_flux=np.ones((n + n_dead, 2)), weighted_aeff=np.ones(n + n_dead), initial_weights=w,
                               nu_flux_nodes=np.ones((grid.size, 2)), sample=cols, scale=1.0))
            self.w0.append(w)
            self.ref_bins.append(ref_b)
        wl.events = events
        wl.n_per, wl.n_events = None, sum(len(w) for w in self.w0)
        self.wl, self.n_bins, self.families = wl, wl.n_bins, families

    @functools.lru_cache(maxsize=None)
    def sums(self, point=None):
        """exact (H, S) per container; `point` = i: the weights of point i of the sweep kernel, table value 2^-i and
        container scale 2^_scale_exp(i, c), formed as the kernel forms them"""
        out = []
        for c, (w0, b) in enumerate(zip(self.w0, self.ref_bins)):
            w = w0
            if point is not None:
                w = ((w0 * 2.0 ** -point) + (w0 * 0.0)) * 2.0 ** _scale_exp(point, c)
            out.append(LC.exact_sums(w, b, self.n_bins))
        return out

    @functools.lru_cache(maxsize=None)
    def limbs(self, point=None):
        return torch.from_numpy(LC.sums_to_limbs(self.sums(point)))

    @functools.lru_cache(maxsize=None)
    def maps(self, point=None):
        return LC.sums_to_maps(self.sums(point))

    @functools.lru_cache(maxsize=None)
    def over(self, point=None):
        """(hist, sumw2) masks of the sums beyond the range: only sums of squares of the "cancel_carry" families"""
        over_h, over_s = LC.sums_out_of_range(self.sums(point))
        assert not over_h.any()
        assert all(str(self.families[c]).startswith("cancel_carry") for c in np.nonzero(over_s.any(axis=1))[0])
        return over_h, over_s


def _scale_exp(point, c):
    """exponent of the per-point container scale: never above the point's table exponent, so that no weight grows"""
    return (c + point) % (point + 1)


def _window_edges(n_bins, width=672):
    out = []
    for lo in range(0, n_bins, width):
        out += [lo, min(lo + width, n_bins) - 1]
    return out


@functools.lru_cache(maxsize=None)
def _case(binning):
    if binning == "dragon":          # 128 bins: LDS accumulators
        return _Case("dragon", [0, 1, 63, 64, 127])
    if binning == "example3d":       # 200 bins: fewer points of the sweep kernel per pass
        return _Case("example3d", [0, 99, 100, 199, 57])
    assert binning == "fine3d"       # 4 800 bins: first and last bin of every 672-bin window
    return _Case("fine3d", _window_edges(4800), n_idle=2100)


def _unit_tables(st):
    """(P_e, P_mu) = (1, 0) on every node, in every table a form may read"""
    for t in (st.prob_nu, st.prob_nubar):
        t.zero_()
        t[:, 0, :] = 1.0
    st.pepmu[..., 0] = 1.0
    st.pepmu[..., 1] = 0.0


def _launch_mode(st):
    """the MODE `reweight_hist_impl` (csrc/hist.hip) picks for the columns this engine's containers carry"""
    n_bins, n_nodes = st.n_bins, st.grid.size
    has_tab = st.indexed                 # `accumulate` hands the gather tables to the indexed forms only

    def of(c):
        if has_tab and c.d_node_bin16 and c.d_weighted_flux_q and n_bins < 0xFFFF and n_nodes < 0xFFFF:
            return 7
        if has_tab and c.d_node_bin and c.d_weighted_flux:
            return 5
        if has_tab and c.d_node_bin and c.d_aeff_w0 and c.d_nu_flux:
            return 3
        if has_tab and c.d_node and c.d_bin:
            return 2
        return 1

    modes = {of(c) for c in st.cont}
    assert len(modes) == 1, modes
    return modes.pop()


def _state(case, **kw):
    from pisa_amd import synthetic

    st = synthetic.DeviceState(case.wl, **kw)
    _unit_tables(st)
    return st


def _check_form(case, st, mode, window):
    from pisa_amd import _lib

    assert _launch_mode(st) == mode
    assert _lib.lib().pisa_hip_hist_window_bins(st.n_bins) == window
    st.accumulate()
    torch.cuda.synchronize()
    st.check_status()                     # the in-range families leave the status word at 0
    got = LC.canonical(st.ws.limbs).cpu()
    want = case.limbs()
    bad = torch.nonzero((got != want).any(dim=-1))
    assert bad.numel() == 0, [(case.families[c], b, "sumw2" if q else "hist", got[c, b, q].tolist(), want[c, b, q].tolist())
                              for c, b, q in bad[:6].tolist()]
    hist, sumw2 = st.finalize()
    _check_maps(case, st, hist.cpu().numpy(), sumw2.cpu().numpy())


def _check_maps(case, st, hist, sumw2, point=None, status=True):
    """the maps are the correctly rounded exact sums; a sum beyond 2^76 (the squares of the "cancel_carry" families)
    has no map: the decoder says so in the status word"""
    over_h, over_s = case.over(point)
    if status and over_s.any():
        with pytest.raises(OverflowError):
            st.check_status()
    elif status:
        st.check_status()
    want_h, want_s = case.maps(point)
    assert np.array_equal(hist[~over_h], want_h[~over_h]) and np.array_equal(sumw2[~over_s], want_s[~over_s])


# ---------------------------------------------------------------------------------- single-point forms
DRAGON_FORMS = {
    "mode3_40B": (3, dict()),
    "mode2_unpacked": (2, dict(packed=False)),
    "mode5_compact": (5, dict(compact=True, index16=False)),
    "mode7_index16": (7, dict(compact=True)),
    "mode1_coordinates": (1, dict(indexed=False)),
    "mode7_node_flux": (7, dict(compact=True, node_flux=True)),
    "mode7_unsorted": (7, dict(compact=True, sort_events=False)),
    "mode7_no_block_order": (7, dict(compact=True, block_order=False)),
}
FINE_FORMS = {
    "mode7_partitioned": (7, dict(compact=True)),
    "mode7_node_order_window": (7, dict(compact=True, sort_events="node")),
    "mode3_window": (3, dict()),
    "mode5_window": (5, dict(compact=True, index16=False)),
    "mode1_global_atomics": (1, dict(indexed=False)),
    "mode2_global_atomics": (2, dict(packed=False)),
}


@pytest.mark.parametrize("form", sorted(DRAGON_FORMS))
def test_deposit_is_exact_with_lds_accumulators(form):
    """128 bins: every deposit is an LDS deposit (two replicas; eight for the coordinate form).  Container sizes are
    odd, even and one, so the odd-tail branches of the pair forms run"""
    mode, kw = DRAGON_FORMS[form]
    case = _case("dragon")
    assert any(len(w) % 2 for w in case.w0) and any(len(w) == 1 for w in case.w0)
    st = _state(case, **kw)
    assert all(c.n_part == 0 for c in st.cont)
    _check_form(case, st, mode, 0)


@pytest.mark.parametrize("form", sorted(FINE_FORMS))
def test_deposit_is_exact_beyond_the_lds_accumulators(form):
    """4 800 bins, families on the first and last bin of every 672-bin window: the partitioned two-window sweep (one
    workgroup works through all eight partitions, so windows are recycled), the general window path (LDS inside the
    window that starts at the chunk's lowest bin, global atomics outside) and the forms without LDS accumulators"""
    mode, kw = FINE_FORMS[form]
    case = _case("fine3d")
    st = _state(case, **kw)
    parts = [int(c.n_part) for c in st.cont]
    if form == "mode7_partitioned":
        # every container but the one-event one is laid out in partitions = the kernel's LDS windows
        assert [p > 0 for p in parts] == [f != "single" for f in case.families], parts
        assert all(int(c.part_width) == 672 for c, p in zip(st.cont, parts) if p)
    else:
        assert not any(parts)
    _check_form(case, st, mode, 672)


def test_accumulating_on_top_adds_the_same_sums_again():
    """`pisa_hip_reweight_hist_acc` (what follows a tail that cleared the limbs) on limbs that hold sums already"""
    case = _case("dragon")
    st = _state(case, compact=True)
    st.accumulate()
    st._limbs_zero = True            # the next launch takes the `_acc` entry: no clear
    st.accumulate()
    torch.cuda.synchronize()
    st.check_status()
    twice = torch.from_numpy(LC.sums_to_limbs([([2 * v for v in H], [2 * v for v in S]) for H, S in case.sums()]))
    assert torch.equal(LC.canonical(st.ws.limbs).cpu(), twice)


# ---------------------------------------------------------------------------------- range probes
PROBES = {"w2_leaves_the_range": 2.0 ** 38, "w2_leaves_the_range_negative": -(2.0 ** 38), "plus_inf": math.inf,
          "minus_inf": -math.inf, "nan": NAN}


def _probe_case(binning, w, n_idle):
    n_bins = {"dragon": 128, "fine3d": 4800}[binning]
    return _Case(binning, [n_bins - 1, 0, 1], n_idle=n_idle, families=([w, 1.0, -2.0, 0.5],))


@pytest.mark.parametrize("form", sorted(DRAGON_FORMS) + sorted(FINE_FORMS))
def test_out_of_range_weights_are_refused(form):
    """each probe in an accumulation of its own (the status word is sticky): 2^38, whose square 2^76 leaves the range
    while the weight is inside, +-inf and NaN raise OverflowError; the double below 2^38 is accepted, exactly"""
    binning, (mode, kw) = ("dragon", DRAGON_FORMS[form]) if form in DRAGON_FORMS else ("fine3d", FINE_FORMS[form])
    n_idle = 600 if binning == "fine3d" else 0
    for name, w in PROBES.items():
        st = _state(_probe_case(binning, w, n_idle), **kw)
        assert _launch_mode(st) == mode
        st.accumulate()
        with pytest.raises(OverflowError):
            st.check_status()
        assert int(st.ws.status.item()) == 0, name       # (reading it clears it)
    ok = _probe_case(binning, float(np.nextafter(2.0 ** 38, 0.0)), n_idle)
    st = _state(ok, **kw)
    if form == "mode7_partitioned":
        assert int(st.cont[0].n_part) > 0
    st.accumulate()
    st.check_status()
    assert torch.equal(LC.canonical(st.ws.limbs).cpu(), ok.limbs())


# ---------------------------------------------------------------------------------- the sweep kernel
def _sweep(st, case, k):
    """`pisa_hip_reweight_hist_multi` alone, through the C ABI: point i reads (2^-i, 0) from the interleaved tables
    and scales container c by 2^_scale_exp(i, c); returns the workspace"""
    from pisa_amd import _lib
    from pisa_amd import kernels as K

    w = st._multi_ws(k)
    n_c = len(st.cont)
    for i in range(k):
        w["tables"][..., i, 0] = 2.0 ** -i
        w["tables"][..., i, 1] = 0.0
    scales = (C.c_double * (k * n_c))(*[2.0 ** _scale_exp(i, c) for i in range(k) for c in range(n_c)])
    _lib.check(_lib.lib().pisa_hip_reweight_hist_multi(
        st._cont_arr, n_c, C.byref(st.grid.binning), C.c_void_p(w["tables"].data_ptr()), k, C.cast(scales, C.c_void_p),
        C.byref(st.out_binning), C.c_void_p(w["limbs"].data_ptr()), 1, C.c_void_p(st.ws.status.data_ptr()), K._stream()))
    torch.cuda.synchronize()
    return w


@pytest.fixture(scope="module")
def sweep_states():
    return {b: _state(_case(b), compact=True) for b in ("dragon", "example3d")}


@pytest.mark.parametrize("binning,k", [("dragon", k) for k in range(1, 10)] + [("example3d", k) for k in (4, 7, 9)])
def test_sweep_kernel_deposits_every_point_exactly(sweep_states, binning, k):
    """K = 1 .. 8 at 128 bins: the eight instantiations in one pass each; K = 9: two passes (5 + 4 points).  200 bins
    (six points fit one pass): K = 4 in one pass, K = 7 and 9 in two (4 + 3, 5 + 4).  Powers of two in the tables and scales keep the products exact and give every point a limb set of its
    own (the digit cuts of the families move by up to K - 1 bits)"""
    from pisa_amd import _lib
    from pisa_amd import kernels as K

    case, st = _case(binning), sweep_states[binning]
    assert _launch_mode(st) == 7 and st.sweep_capable()
    per_pass = _lib.lib().pisa_hip_multi_points_per_pass(st.n_bins)
    assert per_pass == (8 if binning == "dragon" else 6)
    w = _sweep(st, case, k)
    st.check_status()
    n_c = len(st.cont)
    hist = torch.empty((k, n_c, st.n_bins), dtype=torch.float64, device=st.dev)
    sumw2 = torch.empty_like(hist)
    _lib.check(_lib.lib().pisa_hip_hist_finalize(C.c_void_p(w["limbs"].data_ptr()), k * n_c, st.n_bins, C.c_void_p(hist.data_ptr()),
                                                 C.c_void_p(sumw2.data_ptr()), C.c_void_p(st.ws.status.data_ptr()), K._stream()))
    if any(case.over(i)[1].any() for i in range(k)):     # one launch decodes all points
        with pytest.raises(OverflowError):
            st.check_status()
    else:
        st.check_status()
    got = LC.canonical(w["limbs"]).cpu()
    for i in range(k):
        want = case.limbs(i)
        bad = torch.nonzero((got[i] != want).any(dim=-1))
        assert bad.numel() == 0, [(i, case.families[c], b, q, got[i, c, b, q].tolist(), want[c, b, q].tolist())
                                  for c, b, q in bad[:6].tolist()]
        _check_maps(case, st, hist[i].cpu().numpy(), sumw2[i].cpu().numpy(), i, status=False)
    # point 0 (table value 1, scales 1) is the single-point reference, and no two points share a limb set
    assert torch.equal(case.limbs(0), case.limbs())
    assert len({case.limbs(i).numpy().tobytes() for i in range(k)}) == k
    w["limbs"].zero_()
    w["zero"] = True


def test_sweep_kernel_refuses_out_of_range_weights():
    """the probes through the sweep kernel, and a weight that only one point's scale takes out of the range"""
    from pisa_amd import _lib
    from pisa_amd import kernels as K

    for name, bad in list(PROBES.items()) + [("scaled_out", 2.0 ** 37)]:
        case = _probe_case("dragon", bad, 0)
        st = _state(case, compact=True)
        w = st._multi_ws(2)
        w["tables"][..., 0] = 1.0
        w["tables"][..., 1] = 0.0
        scales = (C.c_double * 2)(1.0, 2.0 if name == "scaled_out" else 1.0)
        _lib.check(_lib.lib().pisa_hip_reweight_hist_multi(
            st._cont_arr, 1, C.byref(st.grid.binning), C.c_void_p(w["tables"].data_ptr()), 2, C.cast(scales, C.c_void_p),
            C.byref(st.out_binning), C.c_void_p(w["limbs"].data_ptr()), 1, C.c_void_p(st.ws.status.data_ptr()), K._stream()))
        with pytest.raises(OverflowError):
            st.check_status()
        if name == "scaled_out":      # the point whose scale is 1 holds exact sums all the same
            assert torch.equal(LC.canonical(w["limbs"][0]).cpu(), case.limbs())


# ---------------------------------------------------------------------------------- the generic histogram
@pytest.mark.parametrize("n_bins", [257, 1000])
def test_generic_histogram_is_exact(n_bins):
    """`histogram_regular` (MODE 0: second quantity = the count, so |w| up to the double below 2^76 is accepted) with
    LDS accumulators (257 bins, eight replicas) and without (1 000 bins: global atomics), pairs with 16-byte loads and
    the element loop of unaligned columns: every bin is the correctly rounded exact sum"""
    from pisa_amd import _lib
    from pisa_amd import kernels as K

    assert (_lib.lib().pisa_hip_hist_window_bins(n_bins) == 0) == (n_bins == 257)
    fam = dict(_families())
    top = float(np.nextafter(2.0 ** 76, 0.0))
    fam["range_top"] = np.array([top, -top, top, 2.0 ** 75, -LC.mant(LC.M_ALT_A, 75), -(2.0 ** 60), 2.0 ** 38])
    step = n_bins // (len(fam) + 1)
    ws, bs = [], []
    for f, name in enumerate(sorted(fam)):
        own = [f * step + o for o in (0, 1, step // 2, step - 2, step - 1)]
        n = len(fam[name])
        bs.append(np.full(n, own[0]) if name in LC.ONE_BIN else np.array([own[i % 5] for i in range(n)]))
        ws.append(fam[name])
    n_out = 4 - sum(len(v) for v in ws) % 2                              # events outside the binning (an even count in all)
    w = np.concatenate(ws + [np.array([2.0 ** 70, -3.0, 1.0, NAN][-n_out:])])
    b = np.concatenate(bs + [np.full(n_out, -1)])
    x = np.where(b >= 0, (b + 0.5) / n_bins, [-0.5] * (len(b) - 1) + [NAN])
    x[-3], x[-2] = 1.0, -1e-9                                             # the upper edge is outside (half-open)
    assert len(w) % 2 == 0
    H, _ = LC.exact_sums(w, b, n_bins, second="count")
    want = np.array([LC.value_of(v) for v in H])
    binning = _lib.make_binning([0.0], [1.0], [n_bins])
    xd, wd = K.to_device(np.concatenate([[0.5], x])), K.to_device(np.concatenate([[0.0], w]))
    for lo in (0, 1):        # lo = 1: columns 8 bytes off a 16-byte boundary (the element loop) and an even count
        xs, wts = xd[lo:], wd[lo:]
        assert (xs.data_ptr() % 16 == 0) == (lo == 0)
        got = K.histogram_regular([xs], wts, binning).cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(int(i), got[i], want[i]) for i in bad[:6]]
    # the counts, and the average through them
    cnt = K.histogram_regular([xd[1:]], None, binning).cpu().numpy()
    assert np.array_equal(cnt, np.bincount(b[b >= 0], minlength=n_bins).astype(np.float64))
    for bad_w in (2.0 ** 76, -(2.0 ** 76), math.inf, -math.inf, NAN):
        with pytest.raises(OverflowError):
            K.histogram_regular([xd[:4]], K.to_device(np.array([1.0, bad_w, 2.0, 3.0])), binning)


# ---------------------------------------------------------------------------------- decode through the tails
BLOCK = (3, 251)          # containers x bins of a block of accumulators: no multiple of 4 or 16, several rounds of 256 threads


def _adversarial_blocks():
    cases = LC.adversarial_accumulators()
    tot = [LC.limbs_total(c) for c in cases]
    lim = 1 << (76 + LC.LSB)
    classes = {"nonneg": [c for c, t in zip(cases, tot) if 0 <= t < lim],
               "neg": [c for c, t in zip(cases, tot) if -lim < t < 0],
               "out": [c for c, t in zip(cases, tot) if abs(t) >= lim]}
    assert all(len(v) > 400 for v in classes.values()), {k: len(v) for k, v in classes.items()}
    n = BLOCK[0] * BLOCK[1]
    blocks = []
    for name, cs in classes.items():
        for lo in range(0, len(cs), n):
            chunk = (cs[lo:lo + n] + cs)[:n]                 # the last chunk is filled up from the front
            arr = np.zeros(BLOCK + (2, 6), dtype=np.int64)
            flat = np.array(chunk, dtype=object).astype(np.int64)
            arr[:, :, 0, :] = flat.reshape(BLOCK + (6,))
            arr[:, :, 1, :] = flat[::-1].reshape(BLOCK + (6,))    # the second quantity: the same accumulators reversed
            blocks.append((name, arr))
    return blocks


def _expect(arr):
    """what a tail must leave for a block of accumulators: the maps (correctly rounded), which accumulators are inside
    the range, and -- where all are -- whether a template bin / any sum is negative"""
    from pisa_amd.engine import limbs_to_float

    n_c, n_b = arr.shape[:2]
    lim = 1 << (76 + LC.LSB)
    maps, oks = [], []
    for q in (0, 1):
        maps.append(np.array([[limbs_to_float(arr[c, b, q].tolist()) for b in range(n_b)] for c in range(n_c)]))
        oks.append(np.array([[abs(LC.limbs_total(arr[c, b, q].tolist())) < lim for b in range(n_b)] for c in range(n_c)]))
    h, s = maps
    in_range = bool(oks[0].all() and oks[1].all())
    lam = h[0].copy()
    for m in range(1, n_c):          # the kernel's own order of additions
        lam = lam + h[m]
    return dict(arr=arr, hist=h, sumw2=s, ok_h=oks[0], ok_s=oks[1], in_range=in_range,
                negative=bool((lam < 0).any()) if in_range else None,
                negative_any=bool((h < 0).any() or (s < 0).any()) if in_range else None)


@pytest.fixture(scope="module")
def decode_blocks():
    out = [(name, _expect(arr)) for name, arr in _adversarial_blocks()]
    assert all(e["in_range"] == (n != "out") for n, e in out)
    assert all(e["negative"] == (n == "neg") for n, e in out if e["in_range"])
    # what the deposit tests produce: raw (un-normalised) limbs of two kernel forms, with negative and cancelling totals.
    # "deposit": as they are (two sums of squares are beyond the range); "deposit_hist": the second quantity replaced
    # by the first of the containers in reverse order, so that every accumulator is inside
    case = _case("dragon")
    for kw in (dict(), dict(compact=True)):
        st = _state(case, **kw)
        st.accumulate()
        torch.cuda.synchronize()
        st.check_status()
        raw = st.ws.limbs.cpu().numpy()
        e = _expect(raw)
        want_h, want_s = case.maps()
        over_h, over_s = case.over()
        assert np.array_equal(e["ok_h"], ~over_h) and np.array_equal(e["ok_s"], ~over_s) and not e["in_range"]
        assert np.array_equal(e["hist"], want_h) and np.array_equal(e["sumw2"][~over_s], want_s[~over_s])
        out.append(("deposit", e))
        both = raw.copy()
        both[:, :, 1, :] = raw[::-1, :, 0, :]
        e = _expect(both)
        assert e["in_range"] and e["negative"] and e["negative_any"]
        out.append(("deposit_hist", e))
    assert {n for n, _ in out} == {"nonneg", "neg", "out", "deposit", "deposit_hist"}
    return out


def _join(parts):
    p = [float(v) for v in parts]
    w = len(p) // 2
    while w >= 1:            # the kernel's reduction tree, its last levels
        for i in range(w):
            p[i] = p[i] + p[i + w]
        w //= 2
    return p[0]


def _run_tail(entry, kind, blocks, n_parts=1):
    """one tail launch over `blocks` (one point each); returns (hist, sumw2, limbs after, status, metric status, values)"""
    from pisa_amd import _lib
    from pisa_amd import kernels as K

    lib, dev = _lib.lib(), K.device()
    n_pts = len(blocks)
    n_c, n_b = blocks[0]["arr"].shape[:2]
    limbs = torch.from_numpy(np.stack([b["arr"] for b in blocks])).to(dev)
    hist = torch.full((n_pts, n_c, n_b), -7.0, dtype=torch.float64, device=dev)
    sumw2 = torch.full_like(hist, -7.0)
    data = torch.full((n_b,), 3.0, dtype=torch.float64, device=dev)
    tot = torch.full((n_pts * 16,), 123.0, dtype=torch.float64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    mst = torch.zeros(1, dtype=torch.int32, device=dev)
    if entry == "single":
        assert n_pts == 1
        rc = lib.pisa_hip_finalize_metric(limbs.data_ptr(), n_c, n_b, hist.data_ptr(), sumw2.data_ptr(), K.METRIC_KIND[kind],
                                          data.data_ptr(), tot.data_ptr(), st.data_ptr(), mst.data_ptr(), 1, None)
    elif entry == "gpllh":
        n_mc = torch.full((n_c, n_b), 200.0, dtype=torch.float64, device=dev)
        adjust = torch.zeros(n_c, dtype=torch.float64, device=dev)
        per_bin = torch.zeros((n_pts, n_b), dtype=torch.float64, device=dev)
        done = torch.zeros(n_pts, dtype=torch.int32, device=dev)
        rc = lib.pisa_hip_finalize_gpllh(limbs.data_ptr(), n_pts, n_c, n_b, hist.data_ptr(), sumw2.data_ptr(), data.data_ptr(),
                                         n_mc.data_ptr(), adjust.data_ptr(), None, per_bin.data_ptr(), None, 4, done.data_ptr(),
                                         tot.data_ptr(), st.data_ptr(), mst.data_ptr(), 1, None)
    else:
        head = (limbs.data_ptr(), n_pts, n_c, n_b, hist.data_ptr(), sumw2.data_ptr(), K.METRIC_KIND[kind], data.data_ptr(),
                None, 0, None, tot.data_ptr())
        rest = (st.data_ptr(), mst.data_ptr(), 1, None)
        rc = lib.pisa_hip_finalize_metric_parts(*head, n_parts, *rest) if entry == "parts" else \
            lib.pisa_hip_finalize_metric_multi(*head, *rest)
    assert rc == 0
    torch.cuda.synchronize()
    t = tot.cpu().numpy()
    vals = [_join(t[i * n_parts:(i + 1) * n_parts]) for i in range(n_pts)]
    return hist.cpu().numpy(), sumw2.cpu().numpy(), limbs, int(st.item()), int(mst.item()), vals


def _check_tail(entry, kind, named, n_parts=1):
    from pisa_amd import _lib

    blocks = [e for _, e in named]
    hist, sumw2, limbs, st, mst, vals = _run_tail(entry, kind, blocks, n_parts)
    label = (entry, kind, n_parts, [n for n, _ in named])
    assert int(limbs.abs().max().item()) == 0, label                     # clear_limbs = 1
    for i, e in enumerate(blocks):
        # the maps are written as histogrammed, negative totals included; a sum beyond the range has none
        ok_h, ok_s = e["ok_h"], e["ok_s"]
        assert np.array_equal(hist[i][ok_h], e["hist"][ok_h]) and np.array_equal(sumw2[i][ok_s], e["sumw2"][ok_s]), label
        assert (hist[i] != -7.0).all() and (sumw2[i] != -7.0).all(), label
    all_in = all(e["in_range"] for e in blocks)
    assert st == (0 if all_in else 1), label                              # status bit 1: an accumulator beyond the range
    if all_in:
        negative = [e["negative_any" if entry == "gpllh" else "negative"] for e in blocks]
        assert mst == (_lib.ERR_NEGATIVE if any(negative) else 0), label
        if entry != "gpllh":
            assert [math.isnan(v) for v in vals] == negative, (label, vals)


@pytest.mark.parametrize("kind", ["llh", "poisson_llh", "chi2", "mod_chi2"])
def test_decode_through_the_one_workgroup_tail(decode_blocks, kind):
    for named in decode_blocks:
        _check_tail("single", kind, [named])


@pytest.mark.parametrize("n_parts", [4, 16])
def test_decode_through_the_split_tail(decode_blocks, n_parts):
    """bins k mod 4 / k mod 16 per workgroup, items numbered per workgroup (`item_of`)"""
    for kind in ("llh", "poisson_llh", "mod_chi2"):
        for named in decode_blocks:
            _check_tail("parts", kind, [named], n_parts)


def test_decode_through_the_multi_point_tail(decode_blocks):
    """three points holding different blocks in one launch: every point's maps, value and cleared limbs are its own"""
    by = {}
    for n, e in decode_blocks:
        by.setdefault(n, []).append((n, e))
    assert len(by["nonneg"]) >= 2 and len(by["deposit"]) == 2 and len(by["deposit_hist"]) == 2
    for kind in ("llh", "mod_chi2"):
        _check_tail("multi", kind, [by["nonneg"][0], by["neg"][0], by["nonneg"][1]])
        _check_tail("multi", kind, [by["nonneg"][1], by["nonneg"][0], by["nonneg"][1]])
        _check_tail("multi", kind, [by["neg"][0], by["out"][0], by["nonneg"][0]])
        _check_tail("multi", kind, by["deposit"] + by["deposit_hist"][:1])
        _check_tail("multi", kind, by["deposit_hist"] + by["deposit_hist"][:1])
        _check_tail("parts", kind, [by["nonneg"][0], by["neg"][0], by["nonneg"][1]], 4)


def test_decode_through_the_generalized_poisson_tail(decode_blocks):
    by = {}
    for named in decode_blocks:
        _check_tail("gpllh", None, [named])
        by.setdefault(named[0], []).append(named)
    _check_tail("gpllh", None, [by["nonneg"][0], by["neg"][0], by["nonneg"][1]])
    _check_tail("gpllh", None, [by["nonneg"][0], by["nonneg"][1]])
