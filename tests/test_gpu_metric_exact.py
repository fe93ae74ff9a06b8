"""The nine map metrics on the device against exact values: `pisa_hip_metric` per bin (`metric_bin` of
csrc/metric_device.hpp, `metric_bin_wide` of csrc/metric_flux.hip) on every family of tests/metric_cases.py, its totals
against a host replica of the kernels' own reduction trees, and the fused tails of hist_tail.hip
(`pisa_hip_finalize_metric[_multi|_split|_parts|_scaled]`) on the same inputs, laid out as accumulator limbs.

The gate (tests/metric_cases.py): |got - exact| <= G_kind eps (m + 1) per bin, G_kind = 4 max(1, G_REF_kind), with
G_REF_kind the worst such ratio of the reference's own fp64 values and of the CPU oracle (all below 1 but conv_llh's
1.49; measured and held on the CPU by tests/test_host_metric_cases.py).  NaN / -inf outcomes are compared as patterns.
Totals are compared with `==`: the tree is fixed, so the total is a function of the per-bin values alone.

The kernels' own worst ratios on an MI355X (every family; `pytest -s` prints them before each assertion):
    kind                    worst    gate  |  kind                    worst    gate
    llh                     0.652    4     |  signed_sqrt_mod_chi2    0.841    4
    poisson_llh             0.668    4     |  mcllh_mean              0.750    4
    chi2                    0.843    4     |  mcllh_eff               0.889    4
    mod_chi2                0.859    4     |  conv_llh                1.481    5.96
    correct_chi2            0.876    4     |
The kinds that stand on lgamma (poisson_llh, mcllh_mean, mcllh_eff) stay below the reference's own 0.902 / 0.913 / 0.902.
|total - exact sum| of the fused shapes, in eps sum_b (m_b + 1), (1, 4096) / (4, 700) / (12, 128) containers x bins:
    llh 0.037 / 0.022 / 0.061    poisson_llh 0.007 / 0.001 / 0.048    chi2 0.112 / 0.533 / 0.529    mod_chi2 1.104 / 0.797 / 0.529
"""
import math

import numpy as np
import pytest

from tests import limb_cases as lc
from tests import metric_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def L():
    from pisa_amd import _lib

    return _lib


def _dev(K, a):
    return K.to_device(np.ascontiguousarray(a, dtype=np.float64))


def _per_bin(K, kind, f):
    total, pb = K.metric(kind, _dev(K, f["k"]), _dev(K, f["lam"]), _dev(K, f["s2"]), per_bin=True)
    return float(total.item()), pb.cpu().numpy()


@pytest.mark.parametrize("kind", mc.KINDS)
def test_per_bin_values_within_the_gate_of_the_exact_ones(K, kind):
    """every family the kind is evaluated with: patterns equal to the golden's flags, every value inside the gate; the
    total is the tree's sum of those very values"""
    worst = {}
    for fam, kd in mc.pairs():
        if kd != kind:
            continue
        f = mc.families()[fam]
        total, got = _per_bin(K, kind, f)
        ref = mc.exact()[(fam, kind)]
        r = mc.gate_ratio(got, ref["hi"], ref["lo"], ref["m"], ref["flag"])
        worst[fam] = float(np.nanmax(r))
        print("%-22s %-14s worst |got - exact| / (eps (m + 1)) = %.3f   (gate %.2f)" % (kind, fam, worst[fam], mc.g_kind(kind)))
        mc.check(got, ref, mc.g_kind(kind), "%s %s" % (fam, kind))
        assert total == mc.tree_total(got) or (math.isnan(total) and math.isnan(mc.tree_total(got))), (fam, total)
    assert worst
    print("%-22s worst over the families: %.3f" % (kind, max(worst.values())))


def test_stats_functions_on_numpy_inputs_meet_the_gate(K):
    """the free functions of pisa_amd/utils/stats.py (numpy in, per-bin numpy out, `sigma=` where the reference reads
    standard deviations) on every (family, kind): the same gate"""
    from pisa_amd.utils import stats

    for fam, kind in mc.pairs():
        f = mc.families()[fam]
        shape = (2, -1) if f["k"].size % 2 == 0 else (1, -1)
        args = (f["k"].reshape(shape), f["lam"].reshape(shape))
        got = getattr(stats, kind)(*args) if kind in ("llh", "poisson_llh", "chi2") else \
            getattr(stats, kind)(*args, sigma=f["sigma"].reshape(shape))
        assert got.shape == args[0].shape
        mc.check(got.ravel(), mc.exact()[(fam, kind)], mc.g_kind(kind), "stats.%s on %s" % (kind, fam))


# ------------------------------------------------------------------------------------------- totals
def _pool(kind, n, seed):
    """n bins drawn (seeded, with repetition once the pool is used up) from every seeded family the kind runs on"""
    fams = [fam for fam in mc.SEEDED if kind in mc.kinds_of(fam)]
    cols = {c: np.concatenate([mc.families()[fam][c] for fam in fams]) for c in ("k", "lam", "s2")}
    order = np.random.RandomState(seed).permutation(cols["k"].size)
    sel = np.resize(order, n)
    return {c: v[sel] for c, v in cols.items()}


def _cut(x, n_parts):
    """x >= 0 as n_parts fp64 summands whose sum in index order is x exactly: the leading bits of x in growing
    numbers, so that every partial sum is a truncation of x (representable: each addition is exact)"""
    x = np.asarray(x, dtype=np.float64)
    mant, ex = np.frexp(x)
    prev = np.zeros_like(x)
    parts = []
    for j in range(1, n_parts + 1):
        bits = (53 * j + n_parts - 1) // n_parts
        t = np.ldexp(np.floor(np.ldexp(mant, bits)), ex - bits) if j < n_parts else x
        parts.append(t - prev)
        prev = t
    parts = np.array(parts)
    acc = np.zeros_like(x)
    for p in parts:
        acc = acc + p
    assert np.array_equal(acc, x)
    return parts


@pytest.mark.parametrize("n_bins", [1, 255, 256, 257, 4096, 4097, 6000])
def test_totals_are_the_fixed_tree_of_the_per_bin_values(K, n_bins):
    """one workgroup up to 4096 bins (thread t adds bins t, t + 256, ..., then s[t] += s[t + off], off = 128 .. 1),
    the two-stage form above (a bin per thread, the tree per workgroup, the strided pass and the tree again): the
    total equals the host replica applied to the per-bin values the device returned, bit for bit, for all nine kinds,
    one map and three (summed in index order before the formula; summands chosen so that the sum is the one map's
    expectation exactly, so the per-bin values are the one map's too); NaN bins are dropped"""
    for ik, kind in enumerate(mc.KINDS):
        p = _pool(kind, n_bins, 100 * n_bins + ik)
        total1, pb1 = K.metric(kind, _dev(K, p["k"]), _dev(K, p["lam"]), _dev(K, p["s2"]), per_bin=True)
        total3, pb3 = K.metric(kind, _dev(K, p["k"]), _dev(K, _cut(p["lam"], 3)), _dev(K, _cut(p["s2"], 3)), per_bin=True)
        pb1, pb3 = pb1.cpu().numpy(), pb3.cpu().numpy()
        assert pb1.tobytes() == pb3.tobytes(), kind
        want = mc.tree_total(pb1)
        assert math.isfinite(want)
        assert float(total1.item()) == want, (kind, n_bins, float(total1.item()), want)
        assert float(total3.item()) == want, (kind, n_bins, float(total3.item()), want)
        if kind == "llh" and n_bins >= 255:
            assert np.isnan(pb1).any()                    # (bins the sum drops)


# ------------------------------------------------------------------------------------- fused tails
def _limb_exact(x):
    """the accumulator format (LSB 2^-116, |x| < 2^76) holds x exactly"""
    n, d = float(x).as_integer_ratio()
    return lc.accepted(x) and ((abs(n) << lc.LSB) % d == 0)


_FUSED_POOL = None


def _fused_pool():
    """every bin of the seeded families (but `conv`) whose expectation is at least 2^-63 and, like its sigma^2, held
    exactly by the accumulator format -> dict(k, lam, s2, fam [name per bin], idx [index in its family])"""
    global _FUSED_POOL
    if _FUSED_POOL is None:
        rows = []
        for fam in mc.SEEDED:
            if fam == "conv":
                continue
            f = mc.families()[fam]
            for i in range(f["k"].size):
                if f["lam"][i] >= 2.0 ** -63 and _limb_exact(f["lam"][i]) and _limb_exact(f["s2"][i]):
                    rows.append((fam, i))
        _FUSED_POOL = rows
    return _FUSED_POOL


def _layout(n_cont, n_bins, seed):
    rows = _fused_pool()
    rs = np.random.RandomState(seed)
    sel = np.resize(rs.permutation(len(rows)), n_bins)
    fam = [rows[j][0] for j in sel]
    idx = np.array([rows[j][1] for j in sel])
    col = {c: np.array([mc.families()[a][c][i] for a, i in zip(fam, idx)]) for c in ("k", "lam", "s2")}
    lam_c, s2_c = _cut(col["lam"], n_cont), _cut(col["s2"], n_cont)          # [n_cont, n_bins]
    sums = [([lc.units(v) for v in lam_c[c]], [lc.units(v) for v in s2_c[c]]) for c in range(n_cont)]
    assert all(lc.value_of(u) == v for c in range(n_cont) for u, v in zip(sums[c][0], lam_c[c]))
    assert all(lc.value_of(u) == v for c in range(n_cont) for u, v in zip(sums[c][1], s2_c[c]))
    return dict(col, fam=fam, idx=idx, lam_c=lam_c, s2_c=s2_c, limbs=lc.sums_to_limbs(sums))


def _exact_total(lay, kind):
    """(exact sum over the live bins, sum of (m + 1) over them) from the golden"""
    ex = mc.exact()
    his, los, ms = [], [], 0.0
    for a, i in zip(lay["fam"], lay["idx"]):
        ref = ex[(a, kind)]
        if ref["flag"][i] == mc.FLAG_VALUE:
            his.append(float(ref["hi"][i]))
            los.append(float(ref["lo"][i]))
            ms += float(ref["m"][i]) + 1.0
    return math.fsum(his), math.fsum(los), ms


@pytest.mark.parametrize("n_cont,n_bins", [(1, 4096), (4, 700), (12, 128)])
def test_fused_tails_on_the_exact_cases(K, L, n_cont, n_bins):
    """the families the accumulator format holds exactly, as limbs (several containers: summands whose fp64 sum in
    index order is the intended expectation), through every fused entry.  For each: (1) the maps read back are the
    intended expectations and variances exactly; (2) the total is `pisa_hip_metric`'s total on those maps bit for bit
    (split forms joined by the caller's tree; scaled forms against the separately scaled maps plus the extra map);
    (3) unscaled, the total is within G eps sum_b (m_b + 1) of the exact sum.  Unit scales leave the expectation alone,
    so the kinds that read no variance return the unscaled total."""
    import torch

    lib = L.lib()
    dev = K.device()
    lay = _layout(n_cont, n_bins, 7 * n_cont + n_bins)
    assert len(set(lay["fam"])) >= 4 and (lay["lam_c"] == 0).any() == (n_cont > 1)
    data = _dev(K, lay["k"])
    rs = np.random.RandomState(n_bins)
    scales = {"none": None, "unit": np.ones((n_cont, n_bins)), "varied": rs.uniform(0.5, 1.5, size=(n_cont, n_bins))}
    extra = np.stack([_cut(lay["lam"], 2)[1], np.zeros(n_bins)])        # low bits of lam once more: a non-trivial sum
    one = torch.from_numpy(lay["limbs"]).to(dev)                        # [n_cont, n_bins, 2, 6]

    def separate(kind, sc, with_extra):
        lam_c, s2_c = lay["lam_c"], lay["s2_c"]
        if sc is not None:
            e = np.sqrt(s2_c) * sc
            lam_c, s2_c = np.maximum(lam_c * sc, 0.0), e * e
        if with_extra:
            lam_c, s2_c = np.concatenate([lam_c, extra[:1]]), np.concatenate([s2_c, extra[1:]])
        return float(K.metric(kind, data, _dev(K, lam_c), _dev(K, s2_c)).item())

    def fused(entry, kind, n_pts, sc, with_extra, parts=1):
        limbs = one.unsqueeze(0).repeat(n_pts, 1, 1, 1, 1).contiguous()
        hist = torch.full((n_pts, n_cont, n_bins), -7.0, dtype=torch.float64, device=dev)
        sumw2 = torch.full_like(hist, -7.0)
        tot = torch.full((n_pts * 16,), float("nan"), dtype=torch.float64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        mst = torch.zeros(1, dtype=torch.int32, device=dev)
        sc_d = None if sc is None else _dev(K, sc)
        ex_d = _dev(K, extra) if with_extra else None
        kd = K.METRIC_KIND[kind]
        scp, exp_ = (None if sc_d is None else sc_d.data_ptr()), (None if ex_d is None else ex_d.data_ptr())
        head = (limbs.data_ptr(), n_pts, n_cont, n_bins, hist.data_ptr(), sumw2.data_ptr(), kd, data.data_ptr(), scp, 0,
                exp_, tot.data_ptr())
        rest = (st.data_ptr(), mst.data_ptr(), 1, None)
        if entry == "single":
            assert n_pts == 1 and sc is None and not with_extra
            rc = lib.pisa_hip_finalize_metric(limbs.data_ptr(), n_cont, n_bins, hist.data_ptr(), sumw2.data_ptr(), kd,
                                              data.data_ptr(), tot.data_ptr(), *rest)
        elif entry == "scaled":
            assert n_pts == 1
            rc = lib.pisa_hip_finalize_metric_scaled(limbs.data_ptr(), n_cont, n_bins, hist.data_ptr(), sumw2.data_ptr(),
                                                     kd, data.data_ptr(), scp, exp_, tot.data_ptr(), *rest)
        elif entry == "parts":
            rc = lib.pisa_hip_finalize_metric_parts(*head, parts, *rest)
        else:
            rc = (lib.pisa_hip_finalize_metric_split if entry == "split" else lib.pisa_hip_finalize_metric_multi)(*head, *rest)
        assert rc == 0, (entry, kind, rc)
        torch.cuda.synchronize()
        assert int(st.item()) == 0 and int(mst.item()) == 0 and int(limbs.abs().sum().item()) == 0
        h, s = hist.cpu().numpy(), sumw2.cpu().numpy()
        for p in range(n_pts):                                               # (1) the maps, exactly
            assert h[p].tobytes() == lay["lam_c"].tobytes() and s[p].tobytes() == lay["s2_c"].tobytes(), (entry, kind)
        t = tot.cpu().numpy()
        if parts > 1:
            return [mc.join_parts(t[p * parts:(p + 1) * parts]) for p in range(n_pts)]
        return [float(v) for v in t[:n_pts]]

    for kind in mc.FUSED_KINDS:
        want = {(name, we): separate(kind, sc, we) for name, sc in scales.items() for we in (False, True)}
        assert math.isfinite(want[("none", False)])
        if kind != "mod_chi2":
            assert want[("unit", False)] == want[("none", False)]
        runs = [("single", 1, "none", False, 1), ("multi", 1, "none", False, 1), ("multi", 3, "none", False, 1),
                ("multi", 3, "varied", True, 1), ("scaled", 1, "unit", False, 1), ("scaled", 1, "varied", False, 1),
                ("scaled", 1, "varied", True, 1), ("scaled", 1, "none", True, 1)]
        if kind != "chi2":                                                   # (its all-bins rule needs every bin)
            runs += [("split", 1, "none", False, 4), ("split", 3, "varied", True, 4), ("parts", 1, "none", False, 4),
                     ("parts", 3, "none", False, 16), ("parts", 1, "varied", True, 16), ("parts", 1, "unit", False, 4)]
        for entry, n_pts, scale_name, with_extra, parts in runs:
            got = fused(entry, kind, n_pts, scales[scale_name], with_extra, parts)
            for v in got:                                                    # (2) the separate call's total, bit for bit
                assert v == want[(scale_name, with_extra)], (kind, entry, n_pts, scale_name, with_extra, parts, v,
                                                             want[(scale_name, with_extra)])
        hi, lo, msum = _exact_total(lay, kind)                               # (3) the exact sum
        err = abs((want[("none", False)] - hi) - lo)
        print("%-12s (%2d, %4d): |total - exact sum| = %.3g = %.3f eps sum(m + 1)   (gate %.2f)"
              % (kind, n_cont, n_bins, err, err / (mc.EPS * msum), mc.g_kind(kind)))
        assert err <= mc.g_kind(kind) * mc.EPS * msum
