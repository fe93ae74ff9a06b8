"""Shared pieces of the tests of the exact accumulator: the 192-bit fixed-point
number with LSB 2^-116 that every histogram sum is kept in, as six 32-bit digits in int64 limbs.

Everything here is Python-integer arithmetic: the reference of `tests/test_gpu_exact_accumulator.py`
(what the fused kernels must deposit, digit for digit), the accumulators the decoder tests feed to
`limbs_to_double`, and a port of the kernel's two shift forms that pins the rule without a GPU
(`tests/test_host_limbs.py`)."""
import math

import numpy as np

LSB = 116                 # value = sum limb_j 2^(32 j - 116)
NL = 6
TOP = 2.0 ** 76           # |x| >= TOP is refused
M_ONES = (1 << 53) - 1
M_ALT_A = 0x15555555555555          # 1 0101 ... 01  (53 bits)
M_ALT_B = 0x1AAAAAAAAAAAAA          # 1 1010 ... 10  (53 bits)


def canonical(limbs):
    """carry-normalised digits of every accumulator: limbs [..., 6] int64 (un-normalised sums of signed
    digits) -> the unique representation with digits 0 .. 2^32 - 1 below a signed top digit.  Two limb
    sets describe the same exact sums iff these agree (every kernel form cuts a weight into digits with
    `deposit_units`, but each adds them up in an order and a grouping of its own)."""
    out = limbs.clone()
    for j in range(out.shape[-1] - 1):
        carry = out[..., j] >> 32          # arithmetic shift: floor division
        out[..., j] -= carry << 32
        out[..., j + 1] += carry
    return out


# ------------------------------------------------------------------ the rule, in Python integers
def accepted(x):
    """a weight is refused iff it is not finite or |x| >= 2^76"""
    x = float(x)
    return math.isfinite(x) and abs(x) < TOP


def units(x):
    """sign(x) floor(|x| 2^116) of an accepted double, exactly (`engine.float_to_limbs` states the same
    rule through rationals; this form is fast enough for every event of a test)"""
    n, d = float(x).as_integer_ratio()
    u = (abs(n) << LSB) // d
    return -u if n < 0 else u


def digits_of(total):
    """carry-normalised digits of an exact sum of units: five digits 0 .. 2^32 - 1 and a signed top one"""
    out = []
    for _ in range(NL - 1):
        out.append(total & 0xFFFFFFFF)
        total >>= 32
    out.append(total)
    return out


def value_of(total):
    """the correctly rounded fp64 value of an exact sum of units (int / int is correctly rounded)"""
    return total / (1 << LSB)


def limbs_total(limbs):
    return sum(int(v) << (32 * j) for j, v in enumerate(limbs))


# ------------------------------------------------------------------ the kernel's two shift forms
def _fields(x):
    bits = int(np.float64(x).view(np.uint64))
    return bits >> 32, bits & 0xFFFFFFFF        # hi, lo words


def kernel_general(x):
    """`deposit_units_general` (csrc/hist_device.hpp) on Python integers with the kernel's word sizes: the list
    of (digit index, signed count) it hands to `add`, or None where it refuses"""
    hi, lo = _fields(x)
    ex = (hi >> 20) & 0x7FF
    if ex == 0x7FF:
        return None
    t = ex - 1023 + LSB
    if t < 0:
        return []
    j = t >> 5
    if j >= NL:
        return None
    sh = t & 31
    m = (((hi & 0xFFFFF) | 0x100000) << 32) | lo
    low = (m << (sh + 12)) & 0xFFFFFFFFFFFFFFFF
    d0, d1, d2 = m >> (52 - sh), low >> 32, low & 0xFFFFFFFF
    if hi & 0x80000000:
        d0, d1, d2 = -d0, -d1, -d2
    out = [(j, d0)]
    if j >= 1 and d1 != 0:
        out.append((j - 1, d1))
    if j >= 2 and d2 != 0:
        out.append((j - 2, d2))
    return out


def kernel_is_fast(x):
    """the wave-uniform test of `deposit_units`: positive, leading bit in digit 2 or above, in range"""
    hi, _ = _fields(x)
    t = ((hi >> 20) - (1023 - LSB)) & 0xFFFFFFFF
    return ((t - 64) & 0xFFFFFFFF) < NL * 32 - 64


def kernel_fast(x):
    """the branch-free form of `deposit_units` (valid where `kernel_is_fast`)"""
    hi, lo = _fields(x)
    t = ((hi >> 20) - (1023 - LSB)) & 0xFFFFFFFF
    sh = t & 31
    m = (((hi & 0xFFFFF) | 0x100000) << 32) | lo
    low = (m << (sh + 12)) & 0xFFFFFFFFFFFFFFFF
    j = t >> 5
    return [(j, m >> (52 - sh)), (j - 1, low >> 32), (j - 2, low & 0xFFFFFFFF)]


def kernel_units(x):
    """what the kernel deposits for x, as one integer of units (None: refused)"""
    d = kernel_fast(x) if kernel_is_fast(x) else kernel_general(x)
    return None if d is None else sum(v << (32 * j) for j, v in d)


# ------------------------------------------------------------------ weight families
def mant(m, e):
    """m (53 bits, leading bit set) placed with its leading bit at 2^e"""
    return math.ldexp(float(m), e - 52)


POW2_EXPONENTS = (-120, -117, -116, -115, -85, -84, -83, -53, -52, -51, -21, -20, -19, 11, 12, 13, 37)


def weight_families(seed=4, n_random=3000):
    """name -> fp64 weights, every one accepted and with an accepted square (|w| < 2^38).  Each family is
    meant for (container, bin) cells of its own, so that a failure names its cause.  Dealt round-robin over five
    bins, every sum stays inside the range except the sums of SQUARES of the two "cancel_carry" families (several
    hundred times 2^74): their limbs are exact like all others, their map is refused by the decoder."""
    rs = np.random.RandomState(seed)
    fam = {}
    fam["pow2"] = [s * 2.0 ** e for e in POW2_EXPONENTS for s in (1.0, -1.0)]
    # full mantissas with the leading bit at each of the 32 positions of digits 1, 2 and 3
    fam["mantissa"] = [s * mant(m, t - LSB) for t in range(32, 128) for m in (M_ONES, M_ALT_A, M_ALT_B) for s in (1.0, -1.0)]
    nothing = [5e-324, 2.0 ** -1022, 2.0 ** -117, np.nextafter(2.0 ** -116, 0.0)]
    fam["bottom"] = ([s * v for v in nothing for s in (1.0, -1.0)]
                     + [2.0 ** -116, 1.5 * 2.0 ** -116, -1.5 * 2.0 ** -116, 0.0, -0.0])
    pairs = fam["pow2"][::2] + fam["mantissa"][::2] + [mant(M_ONES, 35), 2.0 ** -60 * 3, 1.5 * 2.0 ** -116]
    fam["cancel_pairs"] = [s * v for v in pairs for s in (1.0, -1.0)] + [2.0 ** -116]
    big = mant((1 << 52) | 1, 37)          # 2^37 (1 + 2^-52)
    fam["cancel_carry_neg"] = [big] * 300 + [-big] * 300 + [-(2.0 ** -116)]       # total -1 unit: borrows to the top
    fam["cancel_carry_pos"] = [big] * 301 + [-big] * 300 + [-(2.0 ** -116)]       # one copy less one unit: carries

    def rnd(n, e_lo, e_hi, signs):
        m = (rs.randint(0, 1 << 26, size=n).astype(np.int64) << 26) | rs.randint(0, 1 << 26, size=n) | (1 << 52)
        e = rs.randint(e_lo, e_hi + 1, size=n)
        s = rs.choice(signs, size=n)
        return [float(si) * mant(int(mi), int(ei)) for si, mi, ei in zip(s, m, e)]

    # Exponents above 33 only for a handful of events per family: a bin's sum of squares must itself stay below 2^76
    # for its map to exist (the top of the range has families of its own: "pow2", "top", "cancel_carry_*").
    def spread(n, e_lo, signs):
        return rnd(n - 5, e_lo, 33, signs) + rnd(5, 34, 36, signs)     # (the last five fall into five different bins)

    fam["random"] = spread(n_random, -125, (1.0, -1.0))
    fam["fast_only"] = spread(1025, -26, (1.0,))       # w and w w at or above 2^-52: no wavefront leaves the fast path
    fam["general_only"] = rnd(324, -125, -53, (1.0,)) + spread(700, -125, (-1.0,))
    fam["mixed"] = rnd(1024, -52, 33, (1.0,)) + spread(1023, -125, (1.0, -1.0))
    fam["single"] = [-mant(M_ALT_B, -60)]
    top = float(np.nextafter(2.0 ** 38, 0.0))                                     # the largest weight with an accepted square
    fam["top"] = [top, -top, 2.0 ** 37, -mant(M_ONES, 37)]
    out = {k: np.array(v, dtype=np.float64) for k, v in fam.items()}
    for k, v in out.items():
        assert all(accepted(x) and accepted(np.float64(x) * np.float64(x)) for x in v), k
    return out


FAMILY_ORDER = ("pow2", "mantissa", "bottom", "cancel_pairs", "cancel_carry_neg", "cancel_carry_pos", "random",
                "fast_only", "general_only", "mixed", "single", "top")
ONE_BIN = ("cancel_pairs", "cancel_carry_neg", "cancel_carry_pos", "single")    # families whose point is one sum


def exact_sums(weights, bins, n_bins, second="square"):
    """exact sums of one container: (H [n_bins], S [n_bins]) Python integers of units from the weights the
    kernel sees and their bins (-1: no deposit).  second = "square": units(fl(w w)), numpy's product."""
    H, S = [0] * n_bins, [0] * n_bins
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(all="ignore"):
        w2 = w * w
    for x, x2, b in zip(w.tolist(), w2.tolist(), np.asarray(bins).tolist()):
        if b < 0:
            continue
        H[b] += units(x)
        S[b] += units(x2) if second == "square" else 1 << LSB
    return H, S


def sums_to_limbs(sums):
    """[(H, S)] per container -> canonical limbs int64 [n_cont, n_bins, 2, 6]"""
    n_cont, n_bins = len(sums), len(sums[0][0])
    out = np.zeros((n_cont, n_bins, 2, NL), dtype=np.int64)
    for c, (H, S) in enumerate(sums):
        for q, tot in enumerate((H, S)):
            for b in range(n_bins):
                if tot[b]:
                    out[c, b, q] = digits_of(tot[b])
    return out


def sums_out_of_range(sums):
    """[(H, S)] per container -> boolean (hist, sumw2) [n_cont, n_bins]: the exact sum does not fit the format"""
    lim = 1 << (76 + LSB)
    return (np.array([[abs(v) >= lim for v in H] for H, _ in sums]), np.array([[abs(v) >= lim for v in S] for _, S in sums]))


def sums_to_maps(sums):
    """[(H, S)] per container -> (hist, sumw2) fp64 [n_cont, n_bins], correctly rounded"""
    hist = np.array([[value_of(v) for v in H] for H, _ in sums], dtype=np.float64)
    sumw2 = np.array([[value_of(v) for v in S] for _, S in sums], dtype=np.float64)
    return hist, sumw2


# ------------------------------------------------------------------ accumulators for the decoder
def adversarial_accumulators(seed=9):
    """six-limb accumulators built to hurt `limbs_to_double`: negative and mixed-sign limbs, carries that
    ripple through every limb, values exactly halfway between two doubles (ties to even, both directions,
    with and without a sticky bit far below), single bits at either end of the range, zero, and random
    fills of every magnitude"""
    rs = np.random.RandomState(seed)
    cases = []
    cases.append([0] * 6)
    cases.append([1, 0, 0, 0, 0, 0])                     # 2^-116
    cases.append([-1, 0, 0, 0, 0, 0])
    cases.append([0, 0, 0, 0, 0, 1 << 30])               # near the top of the range
    cases.append([0, 0, 0, 0, 0, -(1 << 30)])
    cases.append([0xFFFFFFFF] * 5 + [0])                 # carries everywhere
    cases.append([-0xFFFFFFFF] * 5 + [1])                # borrows everywhere
    cases.append([(1 << 62) - 1] * 6)                    # heavily un-normalised sums
    cases.append([-(1 << 62)] * 5 + [1 << 20])
    # ties: a 54-bit pattern whose lowest bit is exactly half an ulp, placed at several offsets
    for shift in (0, 5, 31, 32, 40, 63, 64, 77, 100):
        for mant_ in ((1 << 53) | 1, (1 << 53) | 3, (1 << 54) - 1, (1 << 53) + 2 + 1):
            for sticky in (0, 1):
                for sign in (1, -1):
                    total = sign * ((mant_ << (shift + 1)) + (sticky if shift > 0 else 0))
                    limbs, t = [], total
                    for _ in range(5):
                        limbs.append(t & 0xFFFFFFFF)
                        t >>= 32
                    limbs.append(t)
                    if abs(limbs[5]) < (1 << 62):
                        cases.append(limbs)
    for _ in range(3000):
        bits = rs.randint(1, 63, size=6)
        vals = [int(rs.randint(0, 2 ** 31)) << 31 | int(rs.randint(0, 2 ** 31)) for _ in range(6)]
        limbs = [(v & ((1 << int(b)) - 1)) * (1 if rs.rand() < 0.6 else -1) for v, b in zip(vals, bits)]
        if rs.rand() < 0.3:
            for k in rs.choice(6, size=rs.randint(1, 5), replace=False):
                limbs[k] = 0
        cases.append(limbs)
    return cases
