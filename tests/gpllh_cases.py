"""Shared pieces of the tests of the generalized Poisson-gamma likelihood (arXiv:1902.08831 eq. 91; `gpllh_bin`,
`gpllh_params`, `gpllh_publish_and_total` of csrc/gpllh_device.hpp, called by `gpllh_metric_kernel` of csrc/gpllh.hip
and by `finalize_gpllh_kernel` of csrc/hist_tail.hip, and `gpllh_bin_sums_kernel`): the case families, a numpy restatement
of the kernels' arithmetic in the kernels' own order, and the gate.  A plain helper module (no fixtures, no GPU, no
mpmath); `tests/test_host_gpllh_cases.py` pins everything here without a GPU, `tests/test_gpu_gpllh_exact.py` runs the
kernels.  The exact values (eq. 91 in mpmath at 60 digits, `python oracle/gen_gpllh_exact.py`) are committed as
tests/golden/gpllh_exact.npz.

The gate, per bin, on the LOG value the kernel returns:

    |got - exact| <= G * eps * m

    mixture bin   m = sum(alpha) + k + 1  over the containers with finite alpha and beta: pow(base, alpha) amplifies the
                  rounding of its base by alpha, the k-step recursion adds a term about linear in k
    Poisson bin   m = k |log W| + W + k log k + k + 1  (the terms the formula adds and subtracts)

G = KERNEL_FACTOR * max(1, G_REF), the rule of `metric_cases.g_kind`: G_REF is the worst ratio the numpy restatement
below (glibc's pow and log, the kernel's order of operations) reaches against the exact values over the committed
families; the factor 4 covers the device's pow and log against glibc's.  The order of every sum is the restatement's
own and needs no margin.  G_REF is measured on the CPU and never taken from the device:

    python -m pytest tests/test_host_gpllh_cases.py -k "g_ref or params_restatement" -s

Measured (numpy 2.2, glibc): mixture 0.693 (worst in `total`; `lane_split` 0.661), Poisson 0.511, gpllh_params 1.593
relative: G_REF 0.70, 0.52 and 1.60, G = 4, 4 and 6.4.  The reference's own goldens (gpllh_ref.npz, its C code on nine
random cases) lie within 1.30 eps m of the restatement.

Bins whose outcome is a rule value carry a flag instead and are compared with `==`:

    F_ONE       1.0            prefac * delta_k is NaN (0 * inf)
    F_TINY      log(1e-300)    0 <= prefac * delta_k <= 1e-300
    F_SMALL     log(1e-10)     a bin listed empty, k > 0
    F_ZERO      0              a bin listed empty, k = 0
    F_ERR       0, and the call's status is the bin's error code
    F_INF       +inf           (bins marked `edge`) prefac subnormal, delta_k = inf
    F_RESTATED  (bins marked `edge`) a finite value of no meaning: prefac is subnormal and carries few bits.  The reference's C
                code does the same, so the behaviour stays; the device is held to the gate around the RESTATEMENT's
                value there, since eq. 91 is not what the double algorithm computes.  G is still the one derived
                against the exact values on the other families.

Totals: |got - sum exact| <= G eps (sum_b m_b + sum over flagged bins |value_b|), or the propagated +inf; and bit for
bit `total_of` (lane l adds bins l, l + 64, ... then the butterfly) of the device's own per-bin values.

gpllh_params: exact alpha and beta by rational arithmetic, relative gate with m = 1.  Bin sums: exact sums of exact
products, gate (n / 256 + 9) eps sum |term| -- a thread adds at most ceil(n / 256) terms and the tree has eight
levels: a derived bound, not a measurement -- and `==` with `bin_sums`.
"""
import os
from collections import OrderedDict

import numpy as np

EPS = float(np.finfo(np.float64).eps)
KERNEL_FACTOR = 4.0
# worst ratio of the restatement against the exact values (module docstring has the measuring command)
G_REF = {"mixture": 0.70, "poisson": 0.52, "params": 1.60}

PSEUDO_WEIGHT = 0.001
TINY = 1e-300
LOG_TINY = float(np.log(1e-300))
LOG_SMALL = float(np.log(1e-10))
LDS_K = 1536
MAX_CONTAINERS = 1024
ERR_INVALID, ERR_NEGATIVE = -1, -5

F_VALUE, F_ONE, F_TINY, F_SMALL, F_ZERO, F_ERR, F_INF, F_RESTATED = range(8)
RULE_VALUE = {F_ONE: 1.0, F_TINY: LOG_TINY, F_SMALL: LOG_SMALL, F_ZERO: 0.0, F_ERR: 0.0, F_INF: float("inf")}
BRANCH_NONE, BRANCH_POISSON, BRANCH_MIXTURE = 0, 1, 2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT_FILE = os.path.join(GOLDEN, "gpllh_exact.npz")
REF_FILE = os.path.join(GOLDEN, "gpllh_ref.npz")


def g_of(branch):
    return KERNEL_FACTOR * max(1.0, G_REF[branch])


# ----------------------------------------------------------------------------------- the restatement
def wave_sum(v):
    """the xor butterfly 32 .. 1 on 64 lanes: every lane ends with the same bits"""
    v = np.array(v, dtype=np.float64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ m]
    return float(v[0])


def strided64(values):
    """lane l adds values[l], values[l + 64], ... in sequence, starting from +0.0 -> 64 partial sums"""
    v = np.asarray(values, dtype=np.float64)
    pad = np.zeros(((v.size + 63) // 64) * 64)
    pad[:v.size] = v
    live = np.zeros(pad.size, dtype=bool)
    live[:v.size] = True
    acc = np.zeros(64)
    with np.errstate(all="ignore"):
        for row, on in zip(pad.reshape(-1, 64), live.reshape(-1, 64)):
            acc = np.where(on, acc + row, acc)
    return acc


def total_of(per_bin):
    """gpllh_publish_and_total: NaN and inf propagate"""
    with np.errstate(all="ignore"):
        return wave_sum(strided64(per_bin))


def params(sw, sw2, n, adj):
    """gpllh_params as written in the header, elementwise -> (alpha, beta, wsum, bad)"""
    sw, sw2, n, adj = (np.array(np.broadcast_arrays(sw, sw2, n, adj)[i], dtype=np.float64) for i in range(4))
    bad = ~(sw >= 0.0) | ~(sw2 >= 0.0) | ~(n >= 0.0)
    pseudo = ~(n > 0.0)
    sw = np.where(pseudo, PSEUDO_WEIGHT, sw)
    sw2 = np.where(pseudo, PSEUDO_WEIGHT * PSEUDO_WEIGHT, sw2)
    n = np.where(pseudo, 1.0, n)
    with np.errstate(all="ignore"):
        mean, var_z = sw / n, sw2 / n
        zero = var_z == 0.0
        beta = np.where(zero, 1.0, mean / var_z)
        alpha = np.where(zero, (n + adj) * PSEUDO_WEIGHT, (n + adj) * ((mean * mean) / var_z))
    return alpha, beta, sw, bad


def mixture_parts(k, a, b):
    """(prefac, delta_k) of the recursion in the kernel's order, over the containers with finite alpha and beta"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok], b[ok]
    with np.errstate(all="ignore"):
        prefac = 1.0
        for ac, bc in zip(a.tolist(), b.tolist()):
            prefac = prefac * float(np.power(np.float64(1.0) / (1.0 + 1.0 / np.float64(bc)), np.float64(ac)))
        s = np.zeros(k + 1)
        idx = np.arange(1, k + 1, dtype=np.float64)
        for ac, bc in zip(a.tolist(), b.tolist()):
            s[1:] = s[1:] + ac * np.power(np.float64(1.0) / (1.0 + np.float64(bc)), idx)
        delta = np.zeros(k + 1)
        delta[0] = 1.0
        lanes = np.arange(64)
        for i in range(1, k + 1):
            part = np.zeros(64)
            for j0 in range(1, i + 1, 64):
                j = j0 + lanes
                on = j <= i
                jj = np.where(on, j, 1)
                part = np.where(on, part + s[jj] * delta[i - jj], part)
            delta[i] = wave_sum(part) / float(i)
    return prefac, float(delta[k])


def outcome(prefac, delta_k):
    """the three outcome rules of fast_pgmix on ret = prefac * delta_k -> (value, flag or F_VALUE)"""
    with np.errstate(all="ignore"):
        ret = float(np.float64(prefac) * np.float64(delta_k))
        if ret != ret:
            return 1.0, F_ONE
        if ret > TINY:
            return float(np.log(ret)), (F_INF if ret == np.inf else F_VALUE)
        if ret >= 0.0:
            return LOG_TINY, F_TINY
    return float("nan"), F_VALUE


def bin_value(kd, empty, w, a, b, n, cap):
    """gpllh_bin -> (value, error code, branch, flag); flag is F_VALUE where the value is computed, never F_RESTATED"""
    if not kd >= 0.0:
        return 0.0, ERR_NEGATIVE, BRANCH_NONE, F_ERR
    k = int(kd)                                              # np.int64(data): truncated
    if empty:
        return (LOG_SMALL, 0, BRANCH_NONE, F_SMALL) if k > 0 else (0.0, 0, BRANCH_NONE, F_ZERO)
    w, a, b, n = (np.asarray(x, dtype=np.float64) for x in (w, a, b, n))
    if np.any(~(w >= 0.0)):
        return 0.0, ERR_NEGATIVE, BRANCH_NONE, F_ERR
    if np.all(n > 100.0):
        W = 0.0
        for x in w.tolist():
            W = W + x
        if k == 0:
            return -W, 0, BRANCH_POISSON, F_VALUE
        x = float(k)
        with np.errstate(all="ignore"):
            return float(x * np.log(W) - W - (x * np.log(x) - x)), 0, BRANCH_POISSON, F_VALUE
    ok = np.isfinite(a) & np.isfinite(b)
    if np.any(ok & (~(a > 0.0) | ~(b > 0.0))) or k > cap:
        return 0.0, ERR_INVALID, BRANCH_MIXTURE, F_ERR
    v, flag = outcome(*mixture_parts(k, a, b))
    return v, 0, BRANCH_MIXTURE, flag


def scratch_k_of(call):
    """the call's scratch_k: its own, or what `kernels.gpllh_scratch_k` sizes (the largest finite count among the
    bins not listed empty with a container of at most 100 MC events)"""
    if call["scratch_k"] >= 0:
        return int(call["scratch_k"])
    mix = (call["n_mc"] <= 100.0).any(axis=0) & (call["empty"] == 0)
    k = call["data"][mix]
    k = k[np.isfinite(k)]
    return int(k.max()) if k.size else 0


def bin_cap(kd, scratch_k):
    """the capacity the launch gives a bin: the LDS part up to LDS_K, the scratch where the count is beyond it"""
    lds_k = min(scratch_k, LDS_K)
    return scratch_k if (kd > float(lds_k) and scratch_k > LDS_K) else lds_k


def call_values(call, bins=None):
    """the restatement on one call -> (per_bin, status, branch, flag) (status: the error code any bin raises)"""
    cap = scratch_k_of(call)
    n_bins = call["data"].size
    out = np.zeros(n_bins)
    branch, flag, status = np.zeros(n_bins, np.int8), np.zeros(n_bins, np.int8), 0
    for i in (range(n_bins) if bins is None else bins):
        kd = float(call["data"][i])
        out[i], err, branch[i], flag[i] = bin_value(kd, bool(call["empty"][i]), call["w"][:, i], call["alpha"][:, i],
                                                    call["beta"][:, i], call["n_mc"][:, i], bin_cap(kd, cap))
        status = err or status
    return out, status, branch, flag


def tree256(s):
    s = np.array(s, dtype=np.float64)
    off = 128
    with np.errstate(all="ignore"):
        while off > 0:
            s[:off] = s[:off] + s[off:2 * off]
            off >>= 1
    return float(s[0])


def bin_sums(weights, index, offsets):
    """gpllh_bin_sums_kernel: thread t adds every 256th listed event in sequence, then the 128 .. 1 tree
    -> (sw, sw2, status)"""
    n_bins = len(offsets) - 1
    sw, sw2, status = np.zeros(n_bins), np.zeros(n_bins), 0
    for b in range(n_bins):
        x = np.asarray(weights, dtype=np.float64)[index[offsets[b]:offsets[b + 1]]]
        if np.any(~(x >= 0.0)):
            status = ERR_NEGATIVE
        n = x.size
        pad = np.zeros(((n + 255) // 256) * 256)
        pad[:n] = x
        live = np.arange(pad.size) < n
        a1, a2 = np.zeros(256), np.zeros(256)
        with np.errstate(all="ignore"):
            for row, on in zip(pad.reshape(-1, 256), live.reshape(-1, 256)):
                a1 = np.where(on, a1 + row, a1)
                a2 = np.where(on, a2 + row * row, a2)
        sw[b], sw2[b] = tree256(a1), tree256(a2)
    return sw, sw2, status


# -------------------------------------------------------------------------------------- the families
def _call(name, data, alpha, beta, n_mc, w=None, empty=None, scratch_k=-1, edge=(), **extra):
    alpha, beta = np.atleast_2d(np.asarray(alpha, dtype=np.float64)), np.atleast_2d(np.asarray(beta, dtype=np.float64))
    data = np.asarray(data, dtype=np.float64).ravel()
    n_mc = np.broadcast_to(np.asarray(n_mc, dtype=np.float64), alpha.shape).copy()
    with np.errstate(all="ignore"):
        w = np.where(np.isfinite(alpha / beta), alpha / beta, 1.0) if w is None else np.asarray(w, dtype=np.float64)
    empty = np.zeros(data.size, np.uint8) if empty is None else np.asarray(empty, dtype=np.uint8)
    assert alpha.shape == beta.shape == w.shape == n_mc.shape == (alpha.shape[0], data.size) and empty.shape == data.shape
    c = OrderedDict(data=data, w=np.ascontiguousarray(w), alpha=np.ascontiguousarray(alpha),
                    beta=np.ascontiguousarray(beta), n_mc=n_mc, empty=empty, scratch_k=np.int64(scratch_k),
                    edge=np.zeros(data.size, np.uint8))
    c["edge"][list(edge)] = 1          # bins beyond the domain: classed by the double algorithm, not by eq. 91
    for k, v in extra.items():
        c[k] = np.ascontiguousarray(v, dtype=np.float64)
    c["name"] = name
    return c


def _draw(rs, k, n_cont, a_lo=0.5, a_hi=100.0, width=0.5):
    """alpha log-uniform, beta log-normal around sum(alpha) / max(k, 1): the mean of the mixture lies near k"""
    a = 10 ** rs.uniform(np.log10(a_lo), np.log10(a_hi), n_cont)
    b = a.sum() / max(float(k), 1.0) * np.exp(width * rs.randn(n_cont))
    return a, b


LANE_K = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
LANE_CONT = (1, 3, 17)
BIG_K = (1535.0, 1536.0, 1537.0, 2049.0, 1536.9, 1537.2)
CONT_SIZES = (1, 64, 65, 1024)
POISSON_W = (1e-3, 1.0, 1e3, 1e6)
TOTAL_BINS = (1, 63, 64, 65, 200)


def _columns(rs, ks, n_cont, **kw):
    cols = [_draw(rs, int(k), n_cont, **kw) for k in ks]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def _big_columns():
    """the six bins around the LDS / scratch switch: 2 containers, sum(alpha) = 200 (prefac stays normal: -log prefac =
    sum alpha log(1 + 1 / beta) < 500), the mean near k"""
    rs = np.random.RandomState(712)
    a = np.stack([np.array([120.0, 80.0]) * (1 + 0.01 * rs.rand(2)) for _ in BIG_K], axis=1)
    b = np.stack([a[:, i] * 2.0 / np.floor(k) * np.exp(0.1 * rs.randn(2)) for i, k in enumerate(BIG_K)], axis=1)
    return a, b


def _domain_edge():
    """prefac = (beta / (1 + beta))^alpha below the normal range.  -log prefac <= sum alpha / beta, the mean, so the
    mean is above 700 there and delta_k = P(k) / prefac cannot underflow together with prefac; the underflowing
    delta_k is shown at a normal prefac (mean 1e-3, k = 150).  One container, and two whose product is subnormal."""
    cols = [
        # (k, alphas, betas)                     prefac      delta_k       outcome
        (10, [3000.0], [3.0]),                 # 0           finite        log(1e-300)
        (1000, [3000.0], [3.0]),               # 0           inf           NaN -> 1.0
        (900, [2000.0, 1000.0], [3.0, 3.0]),   # 0           inf           NaN -> 1.0
        (1000, [3000.0], [3.66]),              # subnormal   inf           +inf
        (300, [3000.0], [3.66]),               # subnormal   2.6e234       a finite value with few correct bits
        (320, [1800.0, 1200.0], [3.66, 3.66]),  # subnormal  large         the same, prefac a product of two normal powers
        (3, [3000.0], [3.66]),                 # subnormal   4e7           log(1e-300)
        (150, [1.0], [1000.0]),                # normal      underflows    log(1e-300)
    ]
    n = max(len(c[1]) for c in cols)
    a = np.full((n, len(cols)), np.inf)
    b = np.full((n, len(cols)), np.inf)           # a missing container: non-finite, skipped
    for i, (_, ai, bi) in enumerate(cols):
        a[:len(ai), i], b[:len(bi), i] = ai, bi
    return _call("edge", [c[0] for c in cols], a, b, 50.0, w=np.ones_like(a), edge=range(len(cols)))


def _make_families():
    fam = OrderedDict()
    # lane_split: the j-sum's lane stride (64) and its multiples, 1 / 3 / 17 containers
    rs = np.random.RandomState(701)
    fam["lane_split"] = [_call("cont%d" % nc, LANE_K, *_columns(rs, LANE_K, nc), 50.0) for nc in LANE_CONT]
    # lds_switch: LDS and scratch bins in one launch, and the same bins at explicit scratch sizes
    a, b = _big_columns()
    pick = lambda name, sel, sk: _call(name, [BIG_K[i] for i in sel], a[:, sel], b[:, sel], 50.0, scratch_k=sk)
    fam["lds_switch"] = [pick("auto", [0, 1, 2, 3, 4, 5], -1), pick("k1536", [0, 1, 4], 1536),
                         pick("k1537", [0, 1, 2, 4, 5], 1537), pick("k2049", [0, 1, 2, 3, 4, 5], 2049)]
    # cap: k = scratch_k is evaluated, k = scratch_k + 1 is INVALID; in LDS and in the scratch
    rs = np.random.RandomState(703)
    a64, b64 = _columns(rs, (64, 64, 65), 2)
    fam["cap"] = [_call("lds_at", [63.0, 64.0], a64[:, :2], b64[:, :2], 50.0, scratch_k=64),
                  _call("lds_beyond", [64.0, 65.0], a64[:, 1:], b64[:, 1:], 50.0, scratch_k=64),
                  pick("scratch_at", [1, 2], 1537),
                  _call("scratch_beyond", [1537.0, 1538.0], a[:, [2, 2]], b[:, [2, 2]], 50.0, scratch_k=1537)]
    # branch_rule: > 100 MC events in every container is Poisson, 100 in one is the mixture
    rs = np.random.RandomState(704)
    ks = [7.0, 7.0, 0.0, 0.0]
    n_mc = [[100.0, 101.0, 100.0, 101.0], [5000.0] * 4, [5000.0] * 4]
    a4, b4 = _columns(rs, [7, 7, 1, 1], 3)
    w4 = a4 / b4
    Ws = []
    for W in POISSON_W:                       # k near W and far from it, k = 0 among them
        for k in sorted({np.floor(W), np.ceil(W), np.rint(W) + 1.0, 0.0, np.floor(3.0 * W) + 5.0}):
            ks.append(k)
            Ws.append(W)
    n_p = len(Ws)
    wp = rs.dirichlet(np.ones(3), n_p).T * np.array(Ws)
    fam["branch_rule"] = [_call("rule", ks, np.concatenate([a4, np.full((3, n_p), 2.0)], axis=1),
                                np.concatenate([b4, 2.0 / wp], axis=1),
                                np.concatenate([n_mc, np.full((3, n_p), 5000.0)], axis=1),
                                w=np.concatenate([w4, wp], axis=1))]
    # containers: skipped containers, bins of skipped containers only, empty bins, truncation, errors, container counts
    rs = np.random.RandomState(705)
    ks = [3.0, 4.0, 0.0, 0.0, 5.0, 2.7, 3.0]
    a7, b7 = _columns(rs, [3, 4, 1, 1, 5, 2, 3], 3)
    a7[0, 0], b7[1, 0] = np.inf, np.nan                     # two of three containers skipped
    a7[:, 1], b7[:, 2] = np.nan, np.inf                     # only skipped containers: k = 4, k = 0
    a7[2, 6], b7[2, 6] = -np.inf, -1.0                      # a skipped container is not checked for its sign
    w7 = np.ones_like(a7)
    calls = [_call("skipped", ks, a7, b7, 50.0, w=w7, empty=[0, 0, 0, 1, 1, 0, 0])]
    ag, bg = _columns(rs, [3, 3], 3)

    def bad(name, data=(3.0, 3.0), w=None, **put):
        a2, b2, w2 = ag.copy(), bg.copy(), np.ones_like(ag) if w is None else w
        for key, v in put.items():
            dict(a=a2, b=b2)[key][1, 1] = v
        return _call(name, data, a2, b2, 50.0, w=w2)

    wn = np.ones_like(ag)
    wn[2, 1] = -1e-3
    calls += [bad("alpha_zero", a=0.0), bad("alpha_negative", a=-2.0), bad("beta_zero", b=0.0),
              bad("beta_negative", b=-1.0), bad("weight_negative", w=wn), bad("data_negative", data=(3.0, -1.0)),
              bad("data_nan", data=(3.0, np.nan))]
    for nc in CONT_SIZES:
        calls.append(_call("cont%d" % nc, [2.0, 5.0], *_columns(rs, [2, 5], nc, a_lo=0.5, a_hi=2.0), 50.0))
    fam["containers"] = calls
    fam["domain_edge"] = [_domain_edge()]
    # total: the fixed-order sum of a point over 1 .. 200 bins; with a +inf bin and with the rule value 1.0
    rs = np.random.RandomState(707)
    calls = []
    for nb in TOTAL_BINS:
        ks = rs.randint(0, 40, nb)
        calls.append(_call("bins%d" % nb, ks, *_columns(rs, ks, 2), 50.0))
    e = fam["domain_edge"][0]
    for name, col in (("with_inf", 3), ("with_one", 1)):
        ks = rs.randint(0, 40, 65)
        a2, b2 = _columns(rs, ks, 1)
        ks[40], a2[:, 40], b2[:, 40] = e["data"][col], e["alpha"][:1, col], e["beta"][:1, col]
        calls.append(_call(name, ks, a2, b2, 50.0, edge=[40]))
    fam["total"] = calls
    # fused: what pisa_hip_finalize_gpllh computes from limbs, per point.  The sums are multiples of 2^-40 below 2^20,
    # exactly representable in the accumulator; alpha, beta and w are `params` of them (IEEE operations only, so the
    # device must give the same bits -- the test asserts it before it uses the exact values, which belong to them)
    for name, ks, sk in (("fused_lds", [0.0, 3.0, 64.0, 65.0, 130.0, 7.0, 2.0, 40.0], 130),
                         ("fused_scratch", [1537.0, 3.0, 64.0, 1536.0, 0.0], 1537)):
        rs = np.random.RandomState(708 + len(ks))
        ks = np.array(ks)
        n_mc = np.array([rs.randint(1, 100, ks.size), rs.randint(0, 3, ks.size), np.full(ks.size, 400)], dtype=np.float64)
        n_mc[:, 1] = 5000.0                                            # a Poisson-branch bin
        n_mc[1, 2] = 0.0                                               # a pseudo-weight
        # big counts: alpha is about n for near-equal weights; sum(alpha) near 250 keeps prefac normal
        n_mc[0, ks > 1000], n_mc[1, ks > 1000], n_mc[2, ks > 1000] = 90.0, 60.0, 150.0
        adj = np.array([0.0, 0.25, -0.5])
        calls = []
        for pt in range(3):
            nn = np.maximum(n_mc, 1.0)
            mean_w = np.maximum(ks, 1.0) / 3.0 / nn * np.exp(0.2 * rs.randn(3, ks.size))
            sw =np.round(nn * mean_w * 2.0 ** 40) / 2.0 ** 40
            sw2 = np.round(nn * mean_w ** 2 * (1.0 + 0.3 * rs.rand(3, ks.size)) * 2.0 ** 40) / 2.0 ** 40
            sw[n_mc == 0], sw2[n_mc == 0] = 0.0, 0.0
            al, be, w, isbad = params(sw, sw2, n_mc, adj[:, None])
            assert not isbad.any()
            calls.append(_call("point%d" % pt, ks, al, be, n_mc, w=w, empty=(ks == 2.0), scratch_k=sk, sw=sw, sw2=sw2,
                               adj=adj))
        fam[name] = calls
    return fam


FAMILY_ORDER = ("lane_split", "lds_switch", "cap", "branch_rule", "containers", "domain_edge", "total", "fused_lds",
                "fused_scratch")
INPUT_COLUMNS = ("data", "w", "alpha", "beta", "n_mc", "empty", "scratch_k", "edge")
_FAMILIES = None


def families():
    """{family: [call]}, a call a dict(name, data [n_bins], w / alpha / beta / n_mc [n_cont, n_bins], empty [n_bins]
    uint8, scratch_k (-1: sized as kernels.generalized_poisson_llh does)); built once, read-only"""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _make_families()
        assert tuple(_FAMILIES) == FAMILY_ORDER
        for calls in _FAMILIES.values():
            for c in calls:
                for v in c.values():
                    if isinstance(v, np.ndarray):
                        v.setflags(write=False)
    return _FAMILIES


def params_family():
    """dict(sw, sw2, n [n_cont, n_bins], adj [n_cont]) of `gpllh_params`: every row one mean adjustment, the columns
    n = 0 (pseudo-weight), var_z = 0 (all weights 0, n > 0), equal weights (mean^2 / var_z = 1 exactly), generic sums,
    n + adj small, a subnormal sum of squares (beta overflows to inf; alpha too); and a second call with one negative
    input per column"""
    rs = np.random.RandomState(709)
    adj = np.array([0.0, 0.375, -0.5, -0.999, 1e-3])
    n = np.array([0.0, 0.0, 5.0, 1.0, 1.0, 3.0, 64.0, 1000.0, 17.0, 2.0, 1.0, 1.0, 2.0])
    wq = np.array([0.0, 7.0, 0.0, 0.0, 0.3, 0.3, 1e-5, 3.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    sw = n * wq
    sw2 = n * wq * wq
    gen = slice(8, 10)
    sw[gen], sw2[gen] = 10 ** rs.uniform(-2, 2, 2), 10 ** rs.uniform(-3, 3, 2)
    sw2[10], sw2[11], sw2[12] = 1e-320, 5e-324, 1e-310            # subnormal sums of squares
    shape = (adj.size, n.size)
    full = lambda x: np.ascontiguousarray(np.broadcast_to(x, shape))
    bad = dict(sw=full(sw).copy(), sw2=full(sw2).copy(), n=full(n).copy(), adj=adj)
    bad["sw"][1, 5], bad["sw2"][2, 6], bad["n"][3, 7] = -0.3, -1.0, -1.0
    return dict(sw=full(sw), sw2=full(sw2), n=full(n), adj=adj), bad


BIN_SUM_COUNTS = (0, 1, 255, 256, 257, 513, 70001)


def bin_sums_family():
    """[dict(name, weights, index, offsets, status)]: bins listing 0 .. 70001 events, two bins sharing events, weights
    spanning 1e-30 .. 1e30 in one bin; a negative and a NaN weight unlisted (status 0) and listed (NEGATIVE)"""
    rs = np.random.RandomState(710)
    n_ev = 72000
    w = np.exp(rs.randn(n_ev))
    wide = 10 ** rs.uniform(-30, 30, 300)
    w[71000:71300] = wide
    w[71500], w[71501] = -1.0, np.nan                                 # never listed in "main"
    lists = []
    for n in BIN_SUM_COUNTS:
        lists.append(rs.permutation(71000)[:n])
    lists.append(np.arange(100, 400))                                 # two bins sharing events 250 .. 399
    lists.append(np.arange(250, 700))
    lists.append(rs.permutation(np.arange(71000, 71300)))             # the wide bin
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    main = dict(name="main", weights=w, index=np.concatenate(lists).astype(np.int64), offsets=off, status=0)
    out = [main]
    for name, ev in (("listed_negative", 71500), ("listed_nan", 71501)):
        ls = [np.arange(10, 300), np.array([5, ev, 6])]
        out.append(dict(name=name, weights=w, index=np.concatenate(ls).astype(np.int64),
                        offsets=np.array([0, 290, 293], dtype=np.int64), status=ERR_NEGATIVE))
    return out


def bin_sums_digest(c):
    """SHA-256 of a bin-sums call's inputs (the golden keeps this, not the 72000 weights)"""
    import hashlib

    return hashlib.sha256(b"".join(c[col].tobytes() for col in ("weights", "index", "offsets"))).digest()


# ------------------------------------------------------------------------------------------- the gate
_EXACT = None


def exact():
    """{(family, call index): dict(hi, lo, m, flag, err, branch)} from the committed golden, whose inputs must be
    this module's; also "params" and "bin_sums/<call>" entries"""
    global _EXACT
    if _EXACT is None:
        z = np.load(EXACT_FILE, allow_pickle=False)
        out = {}
        for f, calls in families().items():
            for i, c in enumerate(calls):
                for col in INPUT_COLUMNS:
                    assert z["%s/%d/%s" % (f, i, col)].tobytes() == np.asarray(c[col]).tobytes(), (f, i, col)
                out[(f, i)] = {col: z["%s/%d/%s" % (f, i, col)] for col in ("hi", "lo", "m", "flag", "err", "branch")}
        pf = params_family()[0]
        for col in ("sw", "sw2", "n", "adj"):
            assert z["params/" + col].tobytes() == pf[col].tobytes(), col
        out["params"] = {col: z["params/" + col] for col in ("alpha_hi", "alpha_lo", "beta_hi", "beta_lo")}
        for c in bin_sums_family():
            assert z["bin_sums/%s/digest" % c["name"]].tobytes() == bin_sums_digest(c), c["name"]
            out["bin_sums/" + c["name"]] = {col: z["bin_sums/%s/%s" % (c["name"], col)]
                                            for col in ("sw_hi", "sw_lo", "sw2_hi", "sw2_lo", "abs1", "abs2")}
        _EXACT = out
    return _EXACT


def ratios(got, ref, restated=None):
    """|got - exact| / (eps m) per bin: 0 on flagged bins (compared with == by `check`); on F_RESTATED bins against
    `restated`, the restatement's values"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.abs((got - ref["hi"]) - ref["lo"]) / (EPS * ref["m"])
        if restated is not None:
            r = np.where(ref["flag"] == F_RESTATED, np.abs(got - restated) / (EPS * ref["m"]), r)
    return np.where((ref["flag"] == F_VALUE) | (ref["flag"] == F_RESTATED), r, 0.0)


def check(got, status, ref, restated, what="", g=None):
    """what every value test asserts of one call: the status is the call's error code, flagged bins equal their rule
    value, every other bin is finite and inside the gate -> {branch: worst ratio}"""
    got = np.asarray(got, dtype=np.float64)
    codes = set(ref["err"][ref["err"] != 0].tolist())
    assert len(codes) <= 1, "a call raises one error code"
    assert status == (codes.pop() if codes else 0), (what, status)
    for flag, value in RULE_VALUE.items():
        sel = ref["flag"] == flag
        assert np.array_equal(got[sel], np.full(int(sel.sum()), value)), (what, flag, got[sel])
    live = (ref["flag"] == F_VALUE) | (ref["flag"] == F_RESTATED)
    assert np.all(np.isfinite(got[live])), (what, got[live])
    r = ratios(got, ref, restated)
    worst = {}
    for name, br in (("mixture", BRANCH_MIXTURE), ("poisson", BRANCH_POISSON)):
        sel = live & (ref["branch"] == br)
        worst[name] = float(r[sel].max()) if sel.any() else 0.0
        limit = g_of(name) if g is None else g
        i = int(np.argmax(np.where(sel, r, -1.0)))
        assert worst[name] <= limit, "%s: bin %d (%s): got %.17g exact %.17g m %.4g: %.3g eps m > %.3g" % (
            what, i, name, got[i], ref["hi"][i], ref["m"][i], worst[name], limit)
    return worst


def total_gate(ref):
    """(exact total or +inf or None where a bin is F_RESTATED, the magnitude sum m_b + sum |rule value|)"""
    import math

    if np.any(ref["flag"] == F_INF):
        return float("inf"), 0.0
    if np.any(ref["flag"] == F_RESTATED):
        return None, 0.0
    value = ref["flag"] == F_VALUE
    m = float(ref["m"][value].sum() + np.abs(ref["hi"][~value]).sum())
    return math.fsum(ref["hi"].tolist() + ref["lo"][value].tolist()), m
