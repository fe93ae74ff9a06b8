"""Pins tests/gpllh_cases.py and tests/golden/gpllh_exact.npz without a GPU: the committed exact values against what
the generator gives now, the figures the gate of tests/test_gpu_gpllh_exact.py is built from (G_REF per branch: the
numpy restatement of `gpllh_bin` against the exact values), that every family reaches what it is named for, the clamp's
knife edge, the restatement against the reference's own C code (tests/golden/gpllh_ref.npz), and the restatements of
`gpllh_params`, the bin sums and the total against their exact values.

`gpllh_params` and the outcome rules live in csrc/gpllh_device.hpp, which includes the HIP headers: no HIP-free
stand-alone program reaches them without a change of product code, so no sanitizer build of them is part of this file."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import gpllh_cases as gc


@pytest.fixture(scope="module")
def restated():
    """{(family, call): (per_bin, status, branch, flag)}: the restatement on every call, once"""
    return {(f, i): gc.call_values(c) for f, calls in gc.families().items() for i, c in enumerate(calls)}


def test_committed_exact_golden_is_what_the_generator_gives():
    """a sample of every family (the first, the last and every fifth bin of every call with a count below 300, two of
    the bins around the LDS / scratch switch) recomputed with mpmath; params and bin sums in full"""
    pytest.importorskip("mpmath")
    from oracle import gen_gpllh_exact as gen

    only = {}
    for f, calls in gc.families().items():
        for i, c in enumerate(calls):
            n = c["data"].size
            bins = {b for b in sorted({0, n - 1} | set(range(2, n, 5))) if not c["data"][b] >= 300 or c["edge"][b]}
            if f == "lds_switch" and i == 0:
                bins |= {1, 4}
            if bins:
                only[(f, i)] = bins
    assert {f for f, _ in only} == set(gc.FAMILY_ORDER)
    out = gen.build(1, only)
    z = np.load(gc.EXACT_FILE, allow_pickle=False)
    for (f, i), bins in only.items():
        sel = sorted(bins)
        for col in ("hi", "lo", "m", "flag"):
            key = "%s/%d/%s" % (f, i, col)
            assert out[key][sel].tobytes() == z[key][sel].tobytes(), (key, sel)
        for col in ("err", "branch") + gc.INPUT_COLUMNS:
            key = "%s/%d/%s" % (f, i, col)
            assert out[key].tobytes() == z[key].tobytes(), key
    for extra in (gen.params_exact(), gen.bin_sums_exact()):
        for key, arr in extra.items():
            assert arr.dtype == z[key].dtype and arr.tobytes() == z[key].tobytes(), key


def _worst(restated, g):
    worst = {}
    for (f, i), ref in [(k, v) for k, v in gc.exact().items() if isinstance(k, tuple)]:
        got, status, branch, flag = restated[(f, i)]
        assert np.array_equal(branch, ref["branch"]), (f, i)
        # the restatement's own outcome classes are the golden's (F_RESTATED is F_VALUE to it)
        assert np.array_equal(np.where(ref["flag"] == gc.F_RESTATED, gc.F_VALUE, ref["flag"]), flag), (f, i, flag)
        w = gc.check(got, status, ref, got, "%s %d" % (f, i), g=g)
        for br, r in w.items():
            worst[(f, br)] = max(worst.get((f, br), 0.0), r)
    return worst


def test_g_ref_is_what_the_restatement_measures(restated):
    """G_REF per branch is the worst ratio of the numpy restatement against the exact values over every family,
    rounded up by no more than 1.5; below 2 (a family on which fp64 itself exceeds 2 eps m would be ill-posed)"""
    worst = _worst(restated, 2.0)
    for f in gc.FAMILY_ORDER:
        print("%-14s mixture %.3f  poisson %.3f" % (f, worst.get((f, "mixture"), 0.0), worst.get((f, "poisson"), 0.0)))
    for br in ("mixture", "poisson"):
        w = max(v for (f, b), v in worst.items() if b == br)
        print("%-8s worst %.3f  G_REF %.2f  G %.2f" % (br, w, gc.G_REF[br], gc.g_of(br)))
        assert w <= gc.G_REF[br] <= 1.5 * w, (br, w)
        assert gc.g_of(br) == gc.KERNEL_FACTOR * max(1.0, gc.G_REF[br])


def test_domain_edge_is_recorded_not_gated_against_eq91(restated):
    """where prefac is below the normal range the double algorithm's finite values are not eq. 91's: the distance is
    printed and must be far outside the gate (else the bins would belong to another family), while prefac itself is
    subnormal or 0 in every such bin but the last (a normal prefac, delta_k underflowing)"""
    c, ref = gc.families()["domain_edge"][0], gc.exact()[("domain_edge", 0)]
    got = restated[("domain_edge", 0)][0]
    tiny = float(np.finfo(np.float64).tiny)
    for i in range(c["data"].size):
        p, d = gc.mixture_parts(int(c["data"][i]), c["alpha"][:, i], c["beta"][:, i])
        assert (p < tiny) == (i != c["data"].size - 1), (i, p)
        if ref["flag"][i] == gc.F_RESTATED:
            dist = abs((got[i] - ref["hi"][i]) - ref["lo"][i]) / (gc.EPS * ref["m"][i])
            print("domain_edge bin %d: prefac %.3g delta_k %.3g: restatement %.17g eq. 91 %.17g: %.3g eps m apart"
                  % (i, p, d, got[i], ref["hi"][i], dist))
            assert 0 < p < tiny and dist > 100 * gc.g_of("mixture")
    assert sorted(set(ref["flag"].tolist())) == [gc.F_ONE, gc.F_TINY, gc.F_INF, gc.F_RESTATED]
    assert (ref["flag"] == gc.F_RESTATED).sum() == 2


def test_families_reach_what_they_are_named_for(restated):
    fams, ex = gc.families(), gc.exact()
    flags = np.concatenate([v["flag"] for k, v in ex.items() if isinstance(k, tuple)])
    errs = np.concatenate([v["err"] for k, v in ex.items() if isinstance(k, tuple)])
    assert set(flags.tolist()) == set(range(8))                                     # every flag value
    assert set(errs.tolist()) == {0, gc.ERR_INVALID, gc.ERR_NEGATIVE}               # every error code
    # lane_split: every count beside the lane stride, with 1, 3 and 17 containers
    assert [c["alpha"].shape[0] for c in fams["lane_split"]] == [1, 3, 17]
    for c in fams["lane_split"]:
        assert c["data"].tolist() == [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193]
    # lds_switch: bins on both sides of 1536 in one launch, truncation on each side of kd > lds_k, and explicit sizes
    auto = fams["lds_switch"][0]
    assert gc.scratch_k_of(auto) == 2049 and auto["scratch_k"] == -1
    caps = [gc.bin_cap(k, 2049) for k in auto["data"]]
    assert caps == [1536, 1536, 2049, 2049, 2049, 2049] and auto["data"].tolist()[4:] == [1536.9, 1537.2]
    assert [int(k) for k in auto["data"]] == [1535, 1536, 1537, 2049, 1536, 1537]
    assert [int(c["scratch_k"]) for c in fams["lds_switch"][1:]] == [1536, 1537, 2049]
    assert sum(int((c["data"] >= 1000).sum()) for c in fams["lds_switch"][:1]) <= 8
    for c in fams["lds_switch"]:
        assert c["alpha"].shape[0] == 2 and c["alpha"].sum(axis=0).max() <= 600
    # cap: k = scratch_k evaluated, k = scratch_k + 1 INVALID, below and above 1536
    for at, beyond, sk in ((0, 1, 64), (2, 3, 1537)):
        assert fams["cap"][at]["scratch_k"] == fams["cap"][beyond]["scratch_k"] == sk
        assert fams["cap"][at]["data"].max() == sk and ex[("cap", at)]["err"].tolist() == [0, 0]
        assert fams["cap"][beyond]["data"].tolist() == [sk, sk + 1]
        assert ex[("cap", beyond)]["err"].tolist() == [0, gc.ERR_INVALID]
    # branch_rule: 100 MC events take the mixture, 101 the Poisson branch, k = 0 in each
    c, ref = fams["branch_rule"][0], ex[("branch_rule", 0)]
    assert c["n_mc"][0, :4].tolist() == [100, 101, 100, 101] and np.all(c["n_mc"][1:] == 5000)
    assert ref["branch"][:4].tolist() == [gc.BRANCH_MIXTURE, gc.BRANCH_POISSON] * 2 and c["data"][:4].tolist() == [7, 7, 0, 0]
    W = c["w"].sum(axis=0)[4:]
    for w in gc.POISSON_W:
        sel = np.isclose(W, w, rtol=1e-12)
        k = c["data"][4:][sel]
        assert (k == 0).any() and (np.abs(k - w) <= 1).any() and (k > 3 * w).any(), (w, k)
    assert np.all(ref["flag"] == gc.F_VALUE)
    # containers
    c, ref = fams["containers"][0], ex[("containers", 0)]
    skipped = ~(np.isfinite(c["alpha"]) & np.isfinite(c["beta"]))
    assert skipped[:, 0].sum() == 2 and skipped[:, 1].all() and skipped[:, 2].all()
    assert ref["flag"].tolist() == [0, gc.F_TINY, 0, gc.F_ZERO, gc.F_SMALL, 0, 0] and ref["hi"][2] == 0.0
    assert c["data"][5] == 2.7
    names = [x["name"] for x in fams["containers"]]
    want = dict(alpha_zero=gc.ERR_INVALID, alpha_negative=gc.ERR_INVALID, beta_zero=gc.ERR_INVALID,
                beta_negative=gc.ERR_INVALID, weight_negative=gc.ERR_NEGATIVE, data_negative=gc.ERR_NEGATIVE,
                data_nan=gc.ERR_NEGATIVE)
    for name, code in want.items():
        assert ex[("containers", names.index(name))]["err"].tolist() == [0, code], name
    assert [x["alpha"].shape[0] for x in fams["containers"][-4:]] == [1, 64, 65, gc.MAX_CONTAINERS]
    # total
    assert [x["data"].size for x in fams["total"][:5]] == [1, 63, 64, 65, 200]
    assert all(np.all(ex[("total", i)]["flag"] == 0) for i in range(5))
    assert ex[("total", 5)]["flag"][40] == gc.F_INF and ex[("total", 6)]["flag"][40] == gc.F_ONE
    assert gc.total_of(restated[("total", 5)][0]) == np.inf and np.isfinite(gc.total_of(restated[("total", 6)][0]))
    # fused: three different blocks per point on shared tables, both branches, pseudo-weights, an empty bin
    for f, sk in (("fused_lds", 130), ("fused_scratch", 1537)):
        pts = fams[f]
        assert len(pts) == 3 and all(p["scratch_k"] == sk for p in pts) and pts[0]["data"].max() == sk
        for p in pts[1:]:
            assert np.array_equal(p["n_mc"], pts[0]["n_mc"]) and not np.array_equal(p["sw"], pts[0]["sw"])
        assert {gc.BRANCH_POISSON, gc.BRANCH_MIXTURE} <= set(ex[(f, 0)]["branch"].tolist())
        assert (pts[0]["n_mc"] == 0).any()
    assert (ex[("fused_lds", 0)]["flag"] == gc.F_SMALL).any()


def test_no_unflagged_bin_near_the_clamp():
    """the exact value of every gated bin is more than a factor 1e5 above 1e-300, that of every clamped bin outside
    `domain_edge` more than 1e5 below (the generator asserts the second while it writes)"""
    for key, ref in gc.exact().items():
        if isinstance(key, tuple):
            sel = (ref["flag"] == gc.F_VALUE) & (ref["branch"] == gc.BRANCH_MIXTURE)
            assert np.all(ref["hi"][sel] > math.log(1e-295)), key


def test_restatement_reproduces_the_reference_goldens():
    """tests/golden/gpllh_ref.npz is the reference's own C code on nine random cases: on every mixture bin whose linear
    value `ret` is normal and above the clamp, the restatement's log value lies within the gate of the reference's (G
    of the mixture, m from the golden's alpha and k); on the others the rule outcome is the same value"""
    g = np.load(gc.REF_FILE)
    n, worst = 0, 0.0
    for name in g["cases"]:
        ret, branch, data = g[name + "__ret"], g[name + "__branch"], g[name + "__data"]
        a, b, per_bin = g[name + "__alpha"], g[name + "__beta"], g[name + "__per_bin"]
        for i in np.flatnonzero(branch == 2):
            k = int(data[i])
            value, flag = gc.outcome(*gc.mixture_parts(k, a[:, i], b[:, i]))
            if flag != gc.F_VALUE or not (np.isfinite(ret[i]) and ret[i] > 1e-295):
                assert value == per_bin[i], (name, i, value, per_bin[i])
                continue
            ok = np.isfinite(a[:, i]) & np.isfinite(b[:, i])
            r = abs(value - per_bin[i]) / (gc.EPS * (a[ok, i].sum() + k + 1.0))
            assert r <= gc.g_of("mixture"), (name, i, value, per_bin[i], r)
            n, worst = n + 1, max(worst, r)
    print("restatement against the reference's goldens: %d bins, worst ratio %.3f" % (n, worst))
    assert n > 100


def test_params_restatement_against_exact_values():
    (pf, bad), ex = gc.params_family(), gc.exact()["params"]
    alpha, beta, w, isbad = gc.params(pf["sw"], pf["sw2"], pf["n"], pf["adj"][:, None])
    assert not isbad.any() and gc.params(bad["sw"], bad["sw2"], bad["n"], bad["adj"][:, None])[3].sum() == 3
    worst = 0.0
    for got, name in ((alpha, "alpha"), (beta, "beta")):
        hi, lo = ex[name + "_hi"], ex[name + "_lo"]
        over = np.isinf(hi)
        assert np.array_equal(np.isinf(got), over), name
        with np.errstate(all="ignore"):
            r = np.where(over | (hi == 0), 0.0, np.abs((got - hi) - lo) / (gc.EPS * np.abs(hi)))
        assert np.all(got[hi == 0] == 0)
        worst = max(worst, float(r.max()))
    print("params restatement: worst %.3f eps relative, G_REF %.2f" % (worst, gc.G_REF["params"]))
    assert worst <= gc.G_REF["params"] <= 1.5 * worst
    # the columns are what the family says
    n, sw, sw2 = pf["n"][0], pf["sw"][0], pf["sw2"][0]
    assert (n == 0).sum() == 2 and ((sw2 == 0) & (n > 0)).sum() >= 2 and np.isinf(beta[:, 10:12]).all()
    eq = [4, 5, 6, 7]                                     # equal weights: alpha = n + adj up to rounding
    assert np.allclose(alpha[:, eq], n[eq] + pf["adj"][:, None], rtol=1e-14)
    assert np.all(w[:, n == 0] == gc.PSEUDO_WEIGHT) and np.all(beta[:, (sw2 == 0) & (n > 0)] == 1.0)
    assert (n[None, :] + pf["adj"][:, None]).min() < 2e-3


def test_bin_sums_restatement_against_exact_values():
    for c in gc.bin_sums_family():
        ex = gc.exact()["bin_sums/" + c["name"]]
        sw, sw2, status = gc.bin_sums(c["weights"], c["index"], c["offsets"])
        assert status == c["status"]
        counts = np.diff(c["offsets"])
        for got, name, ab in ((sw, "sw", "abs1"), (sw2, "sw2", "abs2")):
            nan = np.isnan(ex[name + "_hi"])
            assert np.array_equal(np.isnan(got), nan)
            bound = (counts / 256.0 + 9) * gc.EPS * ex[ab]
            err = np.abs((got - ex[name + "_hi"]) - ex[name + "_lo"])
            assert np.all(err[~nan] <= bound[~nan]), (c["name"], name, err, bound)
    main = gc.bin_sums_family()[0]
    counts = np.diff(main["offsets"]).tolist()
    assert counts[:7] == [0, 1, 255, 256, 257, 513, 70001]
    lists = [set(main["index"][main["offsets"][b]:main["offsets"][b + 1]].tolist()) for b in range(len(counts))]
    assert len(lists[7] & lists[8]) == 150
    wide = main["weights"][sorted(lists[9])]
    assert wide.min() < 1e-29 and wide.max() > 1e29
    listed = set(main["index"].tolist())
    unlisted = [i for i in range(main["weights"].size) if i not in listed]
    assert (main["weights"][unlisted] < 0).any() and np.isnan(main["weights"][unlisted]).any()
    assert np.all(main["weights"][sorted(listed)] >= 0)


def test_total_restatement_is_the_fixed_order_sum():
    rs = np.random.RandomState(3)
    for n in (1, 63, 64, 65, 200):
        v = rs.randn(n) * 10 ** rs.uniform(-3, 3, n)
        lanes = [0.0] * 64
        for i, x in enumerate(v.tolist()):
            lanes[i % 64] = lanes[i % 64] + x
        for m in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ m] for l in range(64)]
        assert gc.total_of(v) == lanes[0]
        assert abs(gc.total_of(v) - math.fsum(v.tolist())) <= (n / 64 + 7) * gc.EPS * np.abs(v).sum()
    assert math.isnan(gc.total_of([1.0, np.nan])) and gc.total_of([1.0, np.inf]) == np.inf
    assert Fraction(gc.total_of([0.5, 0.25])) == Fraction(3, 4)
