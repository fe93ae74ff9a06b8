"""The generalized Poisson-gamma likelihood on the device against exact values (tests/golden/gpllh_exact.npz, eq. 91 in
60-digit arithmetic) on the families of tests/gpllh_cases.py: the lane split of the j-sum, the LDS / scratch switch,
the capacity, the branch rule at 100 MC events, skipped containers and the errors, the domain's edge, the total's fixed
order, `gpllh_params`, the bin sums, the fused tail of an evaluation against the unfused chain, and the placement of
a bin in its launch.  The gate and its derivation are in tests/gpllh_cases.py; no mpmath is needed here.

Worst ratios |got - exact| / (eps m) measured on an MI355X are recorded in DESIGN.md (the section on the generalized
likelihood); every test prints its own."""
from collections import OrderedDict

import numpy as np
import pytest

from tests import gpllh_cases as gc

pytestmark = pytest.mark.gpu

VALUE_FAMILIES = ("lane_split", "lds_switch", "cap", "branch_rule", "containers", "domain_edge", "total", "fused_lds",
                  "fused_scratch")


def _dev(a, dtype=np.float64):
    """a host array of a family (read-only, shared) as a device tensor"""
    from pisa_amd import kernels as K

    return K.to_device(np.array(a, dtype=dtype), dtype=dtype)


def _up(c):
    t = {k: _dev(c[k]) for k in ("data", "w", "alpha", "beta", "n_mc")}
    t["empty"] = _dev(c["empty"], np.uint8) if c["empty"].any() else None
    return t


def _abi(c, scratch_k, t=None):
    """pisa_hip_generalized_poisson_llh with an explicit scratch_k -> (per_bin, total, status)"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K

    t = _up(c) if t is None else t
    dev = K.device()
    n_cont, n_bins = c["w"].shape
    scratch = torch.empty(n_bins * 2 * (scratch_k + 1), dtype=torch.float64, device=dev) if scratch_k > gc.LDS_K else None
    per_bin = torch.full((n_bins,), -7.0, dtype=torch.float64, device=dev)
    total = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)               # [status, arrival counter]
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = _lib.lib().pisa_hip_generalized_poisson_llh(
        ptr(t["data"]), ptr(t["w"]), ptr(t["alpha"]), ptr(t["beta"]), ptr(t["n_mc"]), n_cont, n_bins, ptr(t["empty"]),
        ptr(scratch), scratch_k, per_bin.data_ptr(), st.data_ptr() + 4, total.data_ptr(), st.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(st[1].item()) == 0                                    # the arrival counter is back at zero
    return per_bin.cpu().numpy(), float(total.item()), int(st[0].item())


def _check_total(per_bin, total, ref, what):
    """bit for bit the fixed-order sum of the device's own per-bin values, and inside the exact gate"""
    want = gc.total_of(per_bin)
    assert total == want or (np.isnan(total) and np.isnan(want)), (what, total, want)
    exact, m = gc.total_gate(ref)
    if exact is None:
        return 0.0
    if np.isinf(exact):
        assert total == exact, (what, total)
        return 0.0
    g = max(gc.g_of("mixture"), gc.g_of("poisson"))
    r = abs(total - exact) / (gc.EPS * m)
    assert r <= g, "%s: total %.17g exact %.17g m %.4g: %.3g eps m > %.3g" % (what, total, exact, m, r, g)
    return r


def _restated(c, ref):
    """the restatement on the F_RESTATED bins alone (None where a call has none)"""
    sel = np.flatnonzero(ref["flag"] == gc.F_RESTATED)
    return gc.call_values(c, sel)[0] if sel.size else None


@pytest.mark.parametrize("family", VALUE_FAMILIES)
def test_per_bin_values_flags_errors_and_totals(family):
    """every call of the family through the C ABI at its scratch_k (its own, or what the Python wrapper sizes); calls
    that leave the size to the wrapper also through `kernels.generalized_poisson_llh`, where an error code raises"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K

    worst = {"mixture": 0.0, "poisson": 0.0, "total": 0.0}
    for i, c in enumerate(gc.families()[family]):
        ref = gc.exact()[(family, i)]
        what = "%s %s" % (family, c["name"])
        t = _up(c)
        per_bin, total, status = _abi(c, gc.scratch_k_of(c), t)
        w = gc.check(per_bin, status, ref, _restated(c, ref), what)
        w["total"] = _check_total(per_bin, total, ref, what)
        worst = {k: max(worst[k], w[k]) for k in worst}
        if c["scratch_k"] >= 0:
            continue
        assert K.gpllh_scratch_k(t["data"], t["n_mc"], t["empty"]) == gc.scratch_k_of(c)
        if status:
            with pytest.raises(ValueError if status == gc.ERR_NEGATIVE else _lib.PisaHipError):
                K.generalized_poisson_llh(t["data"], t["w"], t["alpha"], t["beta"], t["n_mc"], t["empty"])
        else:
            tot2, pb2 = K.generalized_poisson_llh(t["data"], t["w"], t["alpha"], t["beta"], t["n_mc"], t["empty"])
            assert np.array_equal(pb2.cpu().numpy(), per_bin, equal_nan=True) and float(tot2.item()) == total
    torch.cuda.synchronize()
    print("gpllh_exact %-14s worst ratio: mixture %.3f  poisson %.3f  total %.3f" % (
        family, worst["mixture"], worst["poisson"], worst["total"]))


def test_params_against_exact_values():
    from pisa_amd import kernels as K

    (pf, bad), ex = gc.params_family(), gc.exact()["params"]
    up = lambda d: [_dev(d[k]) for k in ("sw", "sw2", "n", "adj")]
    alpha, beta, w = (x.cpu().numpy() for x in K.gpllh_params(*up(pf)))
    g = gc.g_of("params")
    worst = 0.0
    for got, name in ((alpha, "alpha"), (beta, "beta")):
        hi, lo = ex[name + "_hi"], ex[name + "_lo"]
        over = np.isinf(hi)                   # the exact value is beyond fp64: the sum of squares is subnormal
        assert np.array_equal(np.isinf(got), over) and np.all(got[over] > 0) and not np.isnan(got).any(), name
        assert np.all(got[hi == 0] == 0)
        with np.errstate(all="ignore"):
            r = np.where(over | (hi == 0), 0.0, np.abs((got - hi) - lo) / (gc.EPS * np.abs(hi)))
        worst = max(worst, float(r.max()))
        assert r.max() <= g, (name, np.unravel_index(np.argmax(r), r.shape), r.max())
    print("gpllh_exact params         worst ratio: %.3f (relative, m = 1; G = %.2f)" % (worst, g))
    n = np.broadcast_to(pf["n"], w.shape)
    assert np.array_equal(w, np.where(n > 0, pf["sw"], gc.PSEUDO_WEIGHT))
    with pytest.raises(ValueError):
        K.gpllh_params(*up(bad))
    for col, at in (("sw", (1, 5)), ("sw2", (2, 6)), ("n", (3, 7))):         # each negative input alone
        one = {k: np.array(v) for k, v in pf.items()}
        one[col][at] = bad[col][at]
        with pytest.raises(ValueError):
            K.gpllh_params(*up(one))


def test_bin_sums_against_exact_values():
    from pisa_amd import kernels as K

    for c in gc.bin_sums_family():
        w, index, offsets = _dev(c["weights"]), _dev(c["index"], np.int64), _dev(c["offsets"], np.int64)
        if c["status"]:
            with pytest.raises(ValueError):                   # a negative or NaN weight in a LISTED event
                K.gpllh_bin_sums(w, index, offsets)
            continue
        sw, sw2 = (x.cpu().numpy() for x in K.gpllh_bin_sums(w, index, offsets))   # unlisted ones: status 0
        ex = gc.exact()["bin_sums/" + c["name"]]
        counts = np.diff(c["offsets"])
        rsw, rsw2, _ = gc.bin_sums(c["weights"], c["index"], c["offsets"])
        worst = 0.0
        for got, name, ab, rest in ((sw, "sw", "abs1", rsw), (sw2, "sw2", "abs2", rsw2)):
            err = np.abs((got - ex[name + "_hi"]) - ex[name + "_lo"])
            bound = (counts / 256.0 + 9) * gc.EPS * ex[ab]
            assert np.all(err <= bound), (name, err, bound)
            assert np.array_equal(got, rest), (name, got, rest)                    # the thread chain and the tree
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
        print("gpllh_exact bin_sums       worst error / bound: %.3f" % worst)


def _limbs(points):
    from tests import limb_cases as lc

    out = []
    for p in points:
        sums = [([lc.units(x) for x in p["sw"][c]], [lc.units(x) for x in p["sw2"][c]]) for c in range(p["sw"].shape[0])]
        assert all(lc.value_of(u) == x for (H, S), row in zip(sums, p["sw"]) for u, x in zip(H, row))
        out.append(lc.sums_to_limbs(sums))
    return np.stack(out)


@pytest.mark.parametrize("family", ["fused_lds", "fused_scratch"])
@pytest.mark.parametrize("n_points", [1, 3])
def test_fused_tail_equals_the_unfused_chain_and_the_exact_values(family, n_points):
    """pisa_hip_finalize_gpllh on limbs that hold the family's sums exactly, a different block per point: per point,
    per bin and in total bit for bit hist_finalize -> gpllh_params -> generalized_poisson_llh, and inside the exact
    gate; limbs cleared, counters back at zero, a second launch on the same counters the same bits"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K

    lib, dev = _lib.lib(), K.device()
    points = gc.families()[family][:n_points]
    p0 = points[0]
    n_c, n_b = p0["sw"].shape
    sk = int(p0["scratch_k"])
    host_limbs = _limbs(points)
    data, n_mc, adj, empty = _dev(p0["data"]), _dev(p0["n_mc"]), _dev(p0["adj"]), _dev(p0["empty"], np.uint8)
    f8 = dict(dtype=torch.float64, device=dev)
    scratch = torch.empty(n_points * n_b * 2 * (sk + 1), **f8) if sk > gc.LDS_K else None
    done = torch.zeros(n_points, dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        limbs = torch.from_numpy(host_limbs).to(dev)
        hist, sumw2 = torch.full((n_points, n_c, n_b), -7.0, **f8), torch.full((n_points, n_c, n_b), -7.0, **f8)
        per_bin, total = torch.full((n_points, n_b), -7.0, **f8), torch.full((n_points,), -7.0, **f8)
        st, mst = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.pisa_hip_finalize_gpllh(limbs.data_ptr(), n_points, n_c, n_b, hist.data_ptr(), sumw2.data_ptr(),
                                         data.data_ptr(), n_mc.data_ptr(), adj.data_ptr(), empty.data_ptr(),
                                         per_bin.data_ptr(), None if scratch is None else scratch.data_ptr(), sk,
                                         done.data_ptr(), total.data_ptr(), st.data_ptr(), mst.data_ptr(), 1, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(limbs.abs().max().item()) == 0 and int(done.abs().max().item()) == 0
        assert int(st.item()) == 0 and int(mst.item()) == 0
        runs.append((hist.cpu().numpy(), sumw2.cpu().numpy(), per_bin.cpu().numpy(), total.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    hist, sumw2, per_bin, total = runs[0]
    worst = 0.0
    for pt, p in enumerate(points):
        ref = gc.exact()[(family, pt)]
        what = "%s point %d of %d" % (family, pt, n_points)
        assert np.array_equal(hist[pt], p["sw"]) and np.array_equal(sumw2[pt], p["sw2"]), what
        # the unfused chain on the same limbs
        limbs = torch.from_numpy(host_limbs[pt]).to(dev)
        h, s2 = torch.empty((n_c, n_b), **f8), torch.empty((n_c, n_b), **f8)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        assert lib.pisa_hip_hist_finalize(limbs.data_ptr(), n_c, n_b, h.data_ptr(), s2.data_ptr(), st.data_ptr(), None) == 0
        alpha, beta, w = K.gpllh_params(h, s2, n_mc, adj)
        # IEEE operations only: the family's alpha, beta and weight sums, which the exact values belong to
        for got, col in ((alpha, "alpha"), (beta, "beta"), (w, "w")):
            assert np.array_equal(got.cpu().numpy(), p[col]), (what, col)
        t = dict(data=data, w=w, alpha=alpha, beta=beta, n_mc=n_mc, empty=empty)
        pb, tot, status = _abi(p, sk, t)
        assert status == 0 and np.array_equal(per_bin[pt], pb) and total[pt] == tot, (what, per_bin[pt], pb)
        w_ = gc.check(per_bin[pt], 0, ref, None, what)
        worst = max(worst, w_["mixture"], w_["poisson"], _check_total(per_bin[pt], float(total[pt]), ref, what))
    print("gpllh_exact %-14s fused tail, %d point(s): worst ratio %.3f" % (family, n_points, worst))


def test_a_bin_has_the_same_bits_wherever_it_is_placed():
    """the k = 1537 and k = 2049 bins of `lds_switch` alone in a 1-bin call, and in a 65-bin call whose every bin is
    on the scratch path (64 alternating copies, then the bin as the last one): a scratch offset that overlapped a
    neighbour's would change bits here"""
    c = gc.families()["lds_switch"][0]
    ref = gc.exact()[("lds_switch", 0)]
    col = lambda sel: OrderedDict((k, np.ascontiguousarray(c[k][..., sel])) for k in ("data", "w", "alpha", "beta", "n_mc", "empty"))
    solo = {}
    for b in (2, 3):
        pb, tot, status = _abi(col([b]), 2049)
        assert status == 0 and tot == pb[0]
        solo[b] = pb[0]
        assert abs((pb[0] - ref["hi"][b]) - ref["lo"][b]) <= gc.g_of("mixture") * gc.EPS * ref["m"][b]
    for last in (2, 3):
        sel = [2, 3] * 32 + [last]
        pb, tot, status = _abi(col(sel), 2049)
        assert status == 0
        assert np.array_equal(pb, np.array([solo[b] for b in sel])), (last, pb)
        assert tot == gc.total_of(pb)


def test_map_method_sizes_its_own_scratch():
    """Map.generalized_poisson_llh(binned=True) on the bins around the LDS / scratch switch, data 1536.9 and 1537.2
    among them: the Python path sizes the scratch from the data"""
    from pisa_amd.core.binning import MultiDimBinning, OneDimBinning
    from pisa_amd.core.map import Map, MapSet

    c, ref = gc.families()["lds_switch"][0], gc.exact()[("lds_switch", 0)]
    n_bins = c["data"].size
    b = MultiDimBinning([OneDimBinning("reco_energy", bin_edges=np.arange(n_bins + 1, dtype=float) + 1.0)])
    ev = OrderedDict()
    for key, src in (("weights", "w"), ("llh_alphas", "alpha"), ("llh_betas", "beta"), ("n_mc_events", "n_mc")):
        ev[key] = MapSet([Map("c%d" % i, row, b) for i, row in enumerate(c[src])])
    data = Map("data", c["data"], b)
    per_bin = np.asarray(data.generalized_poisson_llh(ev, binned=True))
    w = gc.check(per_bin, 0, ref, None, "Map lds_switch")
    total = data.generalized_poisson_llh(ev)
    _check_total(per_bin, total, ref, "Map lds_switch")
    print("gpllh_exact Map            worst ratio: mixture %.3f" % w["mixture"])
