"""Shared pieces of the tests of the nine map metrics (`metric_bin` of csrc/metric_device.hpp, shared by `metric_kernel`
and the fused tails of hist_tail.hip, and `metric_bin_wide` of csrc/metric_flux.hip): the seeded case families, the gate
and a host replica of the kernels' reduction trees.  A plain helper module (no fixtures);
`tests/test_host_metric_cases.py` pins everything here without a GPU, `tests/test_gpu_metric_exact.py` runs the kernels.

The exact values (oracle/exact_metric.py: the reference's per-bin formulae in mpmath at 80 digits) are committed as
tests/golden/metric_exact_ref.npz (`python oracle/gen_metric_exact.py`), the reference's own fp64 values on the same
inputs as tests/golden/stats_edge_ref.npz (`python oracle/gen_golden.py stats_edge`).

The gate, per bin and kind:

    |got - exact| <= G_kind * eps * (m + 1)

m is the sum of the absolute values of the terms the fp64 formula adds and subtracts (oracle/exact_metric.py lists it
per kind); the `+ 1` is an absolute floor of one ulp of 1.0 per bin, far below anything a fit can see, which keeps
lgamma near its zeros from being held to a relative accuracy the formula does not need.  NaN and -inf outcomes are
compared as patterns, not through the gate.  G_kind = KERNEL_FACTOR * max(1, G_REF_kind): the device's log is within a
couple of ulp, its lgamma has no stated bound, and where a compiler contracts into fma a term is rounded once instead of
twice.  G_REF_kind is not chosen by looking at the kernels: it is the worst ratio |value - exact| / (eps (m + 1)) of
  - the reference's own values: stats_edge_ref.npz (every seeded family below), stats_ref.npz and stats_wide_ref.npz
    (their inputs are two more families, `stats_ref` and `stats_wide_ref`), and
  - the oracle: `oracle.metric` (C, glibc) and `stages_oracle.metric_wide` (numpy / scipy) on every family.

Measured figures (`tests/test_host_metric_cases.py` measures them again and holds them against G_REF):

    kind                    reference   oracle    G_REF   G_kind
    llh                     0.652       0.652     0.66    4
    poisson_llh             0.902       0.727     0.91    4
    chi2                    0.843       0.843     0.85    4
    mod_chi2                0.859       0.859     0.86    4
    correct_chi2            0.876       0.876     0.88    4
    signed_sqrt_mod_chi2    0.841       0.841     0.85    4
    mcllh_mean              0.913       0.913     0.92    4
    mcllh_eff               0.902       0.902     0.91    4
    conv_llh                1.481       1.481     1.49    5.96

conv_llh alone exceeds 1: where a likelihood underflows the value is ln(SMALL_POS) = -23.03, whose own half ulp is
1.2 eps (m + 1) with m, the terms of the convolutions, about 5 (counts 0 at expectations below 1).

The device's own worst ratios are recorded in tests/test_gpu_metric_exact.py.

What the families leave out, and why (no bin is dropped from a family in any kernel test; each omission is a whole
(family, kind) pair, and one set of bins in the comparison with the reference's values, `reference_is_masked_division`):
  - conv_llh runs on `conv`, `clip` and `lgamma_zeros` only.  Its exact value costs 404 extended-precision steps per
    case, and the other families vary what conv_llh does not read differently from those three (counts beyond 1e4
    put every Poisson term of the convolution below fp64's range: the value is log(SMALL_POS) - log(SMALL_POS)).
  - the eight other kinds run on every family but `conv`, whose point is the width of the convolution.
  - chi2's rule "all |delta| < 5 eps -> a map of zeros" (stats.py:160-161) belongs to a whole map, not to a bin; no
    family is a map of equal pairs, so it is never taken here (tests/test_gpu_kernels.py holds it).
"""
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
SMALL_POS = 1e-10
KERNEL_FACTOR = 4.0

KINDS = ("llh", "poisson_llh", "chi2", "mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2", "mcllh_mean", "mcllh_eff",
         "conv_llh")
PLAIN_KINDS = KINDS[:-1]
SIGMA_KINDS = ("mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2", "mcllh_mean", "mcllh_eff")     # + conv_llh
FUSED_KINDS = ("llh", "poisson_llh", "chi2", "mod_chi2")

# worst ratio of the reference's and the oracle's fp64 values (module docstring)
G_REF = {"llh": 0.66, "poisson_llh": 0.91, "chi2": 0.85, "mod_chi2": 0.86, "correct_chi2": 0.88,
         "signed_sqrt_mod_chi2": 0.85, "mcllh_mean": 0.92, "mcllh_eff": 0.91, "conv_llh": 1.49}
G_HOST = 2.0            # what the exact restatement and the reference's values are held to on the CPU

FLAG_VALUE, FLAG_NAN, FLAG_NEG_INF = 0, 1, 2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT_FILE = os.path.join(GOLDEN, "metric_exact_ref.npz")
EDGE_FILE = os.path.join(GOLDEN, "stats_edge_ref.npz")


def g_kind(kind):
    return KERNEL_FACTOR * max(1.0, G_REF[kind])


# ------------------------------------------------------------------------------------- case families
DELTAS = (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 0.1, -0.1)
LGAMMA_K = (0.0, 5e-324, 1e-300, 1e-17, 1e-12, 1e-3, 0.4616321449683623, 1 - 2.0 ** -52, 1 + 2.0 ** -52, 1 - 1e-9,
            1 + 1e-9, 1.5, 2 - 1e-9, 2 + 1e-9)
CLIP_LAM = (0.0, 1e-300, 1e-11, float(np.nextafter(1e-10, 0.0)), 1e-10, float(np.nextafter(1e-10, 1.0)))
SIGMA_WIDTHS = (0.0, 1e-160, 1e-8, 1e-3, 0.1, 1.0, 10.0, 1e3)
CONV_K = (0.0, 1.0, 2.5, 40.0, 1450.0, 1e4)
CONV_RATIOS = (0.5, 1.0, 1.3)
CONV_WIDTHS = (0.0, 1e-6, 1e-3, 0.01, 0.03, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0)


def _family(k, lam, sigma=None):
    k, lam = np.asarray(k, dtype=np.float64).ravel(), np.asarray(lam, dtype=np.float64).ravel()
    sigma = np.zeros_like(k) if sigma is None else np.asarray(sigma, dtype=np.float64).ravel()
    assert k.shape == lam.shape == sigma.shape
    return dict(k=k, lam=lam, sigma=sigma, s2=sigma * sigma)        # sigma ** 2 as stats.py forms it


def _make_families():
    fam = {}
    # asimov: non-integer counts, k ln(lam) - lam against k ln(k) - k (or lgamma) with full cancellation
    rs = np.random.RandomState(201)
    lam = 10 ** (-3 + 10 * rs.rand(40))
    lam[:2] = [1e-3, 1e7]
    fam["asimov"] = _family(np.concatenate([lam * (1 + d) for d in DELTAS]), np.tile(lam, len(DELTAS)))
    # lgamma_zeros: both zeros of lgamma(k + 1) (k = 0, 1), its minimum (k = 0.46163...), the smallest counts
    k, lam = [], []
    for kk in LGAMMA_K:
        for ll in (kk, 1e-3, 1.0, 50.0):
            k.append(kk)
            lam.append(ll)
    fam["lgamma_zeros"] = _family(k, lam)
    # integers: every count to 200 (170! is the last factorial fp64 holds), powers of two to 2^30
    k = np.concatenate([np.arange(201.0), 2.0 ** np.arange(8, 31)])
    fam["integers"] = _family(np.tile(k, 3), np.concatenate([k * 0.5, k, k * 2.0]))
    # large: to 1e9, integers and half-integers, lam / k around 1
    rs = np.random.RandomState(202)
    k = np.concatenate([10.0 ** np.arange(3, 10), np.rint(10 ** (3 + 6 * rs.rand(20)))])
    k = np.concatenate([k, k + 0.5])
    ratios = (1 - 1e-6, 1.0, 1 + 1e-6, 2.0)
    fam["large"] = _family(np.tile(k, len(ratios)), np.concatenate([k * r for r in ratios]))
    # clip: the expectation at, around and far below SMALL_POS
    k, lam = np.meshgrid([0.0, 1.0, 3.0], CLIP_LAM)
    fam["clip"] = _family(k, lam)
    # sigma: widths from none to 1e3 sqrt(lam); 1e-160 squares to a subnormal and the mixture's shape overflows
    lam = 10 ** np.linspace(np.log10(0.3), 6, 12)
    ks, ls, ss = [], [], []
    for w in SIGMA_WIDTHS:
        for kk in (np.zeros_like(lam), np.rint(lam), lam * 1.1):
            ks.append(kk)
            ls.append(lam)
            ss.append(w * np.sqrt(lam))
    fam["sigma"] = _family(np.concatenate(ks), np.concatenate(ls), np.concatenate(ss))
    # conv: widths in units of sqrt(lam) (of 1 where lam = 0), cut to 24 bits so that sigma^2 is exact and
    # sqrt(sigma^2), which the kernel forms, is the sigma the reference reads
    ks, ls, ss = [], [], []
    for kk in CONV_K:
        for r in CONV_RATIOS:
            ll = (kk if kk > 0 else 1.0) * r if (kk > 0 or r != 1.0) else 0.0      # k = 0: lam = 0.5, 0, 1.3
            for w in CONV_WIDTHS:
                ks.append(kk)
                ls.append(ll)
                ss.append(float(np.float32(w * (np.sqrt(ll) if ll > 0 else 1.0))))
    fam["conv"] = _family(ks, ls, ss)
    return fam


SEEDED = ("asimov", "lgamma_zeros", "integers", "large", "clip", "sigma", "conv")
# the inputs of the two older stats goldens, as two more families: the reference's values are the goldens' own
GOLDEN_INPUTS = {"stats_ref": ("stats_ref.npz", ("llh", "poisson_llh", "chi2", "mod_chi2")),
                 "stats_wide_ref": ("stats_wide_ref.npz", ("mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2",
                                                           "mcllh_mean", "mcllh_eff", "conv_llh"))}
FAMILY_ORDER = SEEDED + tuple(GOLDEN_INPUTS)
CONV_FAMILIES = ("conv", "clip", "lgamma_zeros")
_FAMILIES = None


def families():
    """{name: dict(k, lam, sigma, s2)}: seeded, built once and shared -- the arrays are read-only"""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _make_families()
        for name, (fname, _) in GOLDEN_INPUTS.items():
            g = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
            _FAMILIES[name] = _family(g["actual"], g["expected"], g["sigma"] if "sigma" in g.files else None)
        assert tuple(_FAMILIES) == FAMILY_ORDER
        for f in _FAMILIES.values():
            for v in f.values():
                v.setflags(write=False)
    return _FAMILIES


def kinds_of(family):
    """the kinds a family is evaluated with (module docstring: what is left out and why)"""
    if family in GOLDEN_INPUTS:
        return GOLDEN_INPUTS[family][1]
    if family == "conv":
        return ("conv_llh",)
    return PLAIN_KINDS + (("conv_llh",) if family in CONV_FAMILIES else ())


def pairs():
    return [(f, kind) for f in FAMILY_ORDER for kind in kinds_of(f)]


# ------------------------------------------------------------------------------------------- the gate
def flags_of(values):
    """NaN / -inf pattern of fp64 values, in the golden's encoding"""
    v = np.asarray(values, dtype=np.float64)
    return np.where(np.isnan(v), FLAG_NAN, np.where(v == -np.inf, FLAG_NEG_INF, FLAG_VALUE)).astype(np.int8)


def gate_ratio(got, hi, lo, m, flag):
    """|got - (hi + lo)| / (eps (m + 1)) per bin; 0 where the golden flags a NaN or -inf outcome (compared as a
    pattern by `check`).  got - hi is exact whenever the two are within a factor of two of each other."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.abs((got - hi) - lo) / (EPS * (m + 1.0))
    return np.where(flag == FLAG_VALUE, r, 0.0)


def check(got, ref, g, what=""):
    """the assertions every value test makes of fp64 per-bin values `got` against one (family, kind) entry `ref`
    = dict(hi, lo, m, flag) of the golden: patterns equal, every live bin finite and inside the gate with G = `g`.
    -> the worst ratio"""
    got = np.asarray(got, dtype=np.float64)
    pattern = flags_of(got)
    bad = np.nonzero(pattern != ref["flag"])[0]
    assert bad.size == 0, "%s: NaN / -inf pattern differs at %s: got %s, flags %s" % (
        what, bad[:5], got[bad[:5]], ref["flag"][bad[:5]])
    live = ref["flag"] == FLAG_VALUE
    assert np.all(np.isfinite(got[live])), what + ": non-finite value where the exact one is finite"
    r = gate_ratio(got, ref["hi"], ref["lo"], ref["m"], ref["flag"])
    worst = float(r.max()) if r.size else 0.0
    i = int(np.argmax(r)) if r.size else 0
    assert worst <= g, "%s: bin %d: got %.17g exact %.17g m %.3g: %.3g eps (m + 1) > %.3g" % (
        what, i, got[i], ref["hi"][i], ref["m"][i], worst, g)
    return worst


_EXACT = None


def exact():
    """{(family, kind): dict(hi, lo, m, flag)} from the committed golden, whose inputs must be this module's"""
    global _EXACT
    if _EXACT is None:
        z = np.load(EXACT_FILE, allow_pickle=False)
        fams = families()
        out = {}
        for f in FAMILY_ORDER:
            for c in ("k", "lam", "sigma", "s2"):
                assert z["%s/%s" % (f, c)].tobytes() == fams[f][c].tobytes(), (f, c)
            for kind in kinds_of(f):
                out[(f, kind)] = {c: z["%s/%s/%s" % (f, kind, c)] for c in ("hi", "lo", "m", "flag")}
        _EXACT = out
    return _EXACT


# ----------------------------------------------------------------------- the kernels' reduction trees
def tree256(s):
    """s[t] += s[t + off] for off = 128 .. 1 on 256 fp64 values -> s[0]"""
    s = np.array(s, dtype=np.float64)
    assert s.shape == (256,)
    off = 128
    while off > 0:
        s[:off] = s[:off] + s[off:2 * off]
        off >>= 1
    return float(s[0])


def strided_sums(values):
    """thread t adds values[t], values[t + 256], ... in that order, NaN dropped (np.nansum) -> 256 partial sums"""
    v = np.asarray(values, dtype=np.float64)
    v = np.where(np.isnan(v), 0.0, v)          # acc += 0.0 changes no bit of acc but the sign of a -0.0 start, and acc starts at +0.0
    n = v.size
    pad = np.zeros(((n + 255) // 256) * 256)
    pad[:n] = v
    acc = np.zeros(256)
    for row in pad.reshape(-1, 256):
        acc = acc + row
    return acc


def tree_total(per_bin):
    """the total `pisa_hip_metric` forms from its own per-bin values: one workgroup up to 4096 bins (strided sums,
    then the 256-wide tree), above that one bin per thread and the tree per workgroup, then the same strided pass
    and tree over the workgroups' sums"""
    v = np.asarray(per_bin, dtype=np.float64)
    if v.size <= 4096:
        return tree256(strided_sums(v))
    v = np.where(np.isnan(v), 0.0, v)
    pad = np.zeros(((v.size + 255) // 256) * 256)
    pad[:v.size] = v
    partial = [tree256(row) for row in pad.reshape(-1, 256)]
    return tree256(strided_sums(partial))


def join_parts(p):
    """the caller's join of a split tail's partial sums (4 or 16 of them): the tree's last levels"""
    p = [float(v) for v in p]
    w = len(p) // 2
    while w >= 1:
        for i in range(w):
            p[i] = p[i] + p[i + w]
        w //= 2
    return p[0]


# ------------------------------------------------------------------ reference / oracle on the families
# Where numpy.ma answers instead of the formula.  The reference divides masked arrays, and numpy.ma's division masks
# a quotient whose divisor is below 2.2e-308 times the dividend and passes the DIVIDEND on as its data: at the width
# 1e-160 sqrt(lam) the mixture's alpha = lam^2 / sigma2 and beta = lam / sigma2 become lam^2 and lam, and the values
# the reference returns there are finite numbers of no meaning.  The formula itself, in IEEE arithmetic, overflows
# to inf - inf = NaN: that is what the exact restatement flags, what the oracle gives and what the kernels must give.
# These bins (36 of the 288 of `sigma`, both mixture kinds) are left out of the comparison with the REFERENCE'S values
# only; no kernel test leaves them out.
def reference_is_masked_division(family, kind):
    """boolean per bin: the reference's value is numpy.ma's dividend, not the formula's"""
    f = families()[family]
    if kind not in ("mcllh_mean", "mcllh_eff"):
        return np.zeros(f["k"].size, dtype=bool)
    lam = np.maximum(f["lam"], SMALL_POS)
    with np.errstate(all="ignore"):
        return (f["s2"] > 0) & (lam * lam * float(np.finfo(np.float64).tiny) >= f["s2"])


_EDGE = None


def reference_values(family, kind):
    """the reference's own per-bin values: stats_edge_ref.npz for the seeded families, the older goldens for theirs"""
    global _EDGE
    if family in GOLDEN_INPUTS:
        return np.load(os.path.join(GOLDEN, GOLDEN_INPUTS[family][0]), allow_pickle=False)[kind]
    if _EDGE is None:
        _EDGE = np.load(EDGE_FILE, allow_pickle=False)
    return _EDGE["%s/%s" % (family, kind)]


def oracle_values(orc, so, kind, f):
    """the fp64 oracle's per-bin values of one family: `oracle.metric` for the four kinds of the C oracle (mod_chi2
    with the family's sigma^2), `stages_oracle.metric_wide` for the others"""
    with np.errstate(all="ignore"):
        if kind in FUSED_KINDS:
            return orc.metric(kind, f["k"], f["lam"], f["s2"] if kind == "mod_chi2" else None)[0]
        return np.asarray(so.metric_wide(kind, f["k"], f["lam"], f["sigma"]), dtype=np.float64)
