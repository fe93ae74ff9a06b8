"""The nine per-bin map metrics of pisa/utils/stats.py restated in mpmath (80 digits): what the formulae give on the
real numbers for fp64 inputs (k, lam, sigma2), with every rule of the reference kept:

  - the expectation is clipped to SMALL_POS (stats.py:154-155, 243-244, 318-319, 375-376, 687-688, 721-722, 779-780);
  - llh at k = 0 is NaN (0 * ln 0), so that np.nansum drops the bin;
  - the mixture (likelihood_functions.py:22-63) is Poisson at sigma2 == 0, -inf (0 where k == 0) at lam <= 0 or
    sigma2 < 0, and NaN where its shape alpha = lam^2 / sigma2 + a or rate beta = lam / sigma2 leave fp64's range:
    there the reference adds and subtracts infinities, and that NaN is the expected result;
  - conv_llh (stats.py:479-596): the three clips of conv_poisson, 2 * 51 - 1 = 101 steps over +-3 sigma shifted by
    half a step, the sum started at the first positive f_x, nan_to_num of the Poisson term, the normalisation
    exp(log_poisson(l, l)) / conv_poisson(l, l, s) with its NaN at l = 0, and max(SMALL_POS, .) under both logs
    (Python's max: a NaN argument gives SMALL_POS).

`per_bin(kind, k, lam, s2)` -> (value as mpf or None, m, flag): m is the sum of the absolute values of the terms the
fp64 formula adds and subtracts, the scale of the gate of tests/metric_cases.py:

    llh                    |k ln lam| + lam + |k ln k| + k
    poisson_llh            |k ln lam| + lam + |lgamma(k + 1)|
    mcllh_mean, mcllh_eff  |alpha ln beta| + |lgamma(k + alpha)| + |lgamma(k + 1)| + |(k + alpha) ln(1 + beta)|
                           + |lgamma(alpha)|   (Poisson's three terms at sigma2 == 0)
    chi2, mod_chi2, signed_sqrt_mod_chi2   |value|
    correct_chi2           the quotient + |ln(sigma2 + lam)|
    conv_llh               the largest, over the steps of its four convolutions, of
                           |k ln f_x| + f_x + |lgamma(k + 1)| + |c_y|

chi2's whole-map rule (all |delta| < 5 eps -> zeros, stats.py:160-161) is not a per-bin rule and is not applied.
Needs mpmath; nothing else of this repository.
"""
import math

import mpmath as mp

mp.mp.dps = 80

FLAG_VALUE, FLAG_NAN, FLAG_NEG_INF = 0, 1, 2
SMALL_POS = mp.mpf(1e-10)                 # the fp64 constant, exactly
_TWO_PI = mp.mpf(2 * math.pi)             # 2 * np.pi as fp64 forms it
KINDS = ("llh", "poisson_llh", "chi2", "mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2", "mcllh_mean", "mcllh_eff",
         "conv_llh")


def _f(x):
    return mp.mpf(float(x))


def _poisson(k, lam):
    a, b, c = k * mp.log(lam) if k != 0 else mp.mpf(0), lam, mp.loggamma(k + 1)
    return a - b - c, abs(a) + b + abs(c)


def _mixture(k, lam, s2, a):
    if lam <= 0 or s2 < 0:
        return (mp.mpf(0), mp.mpf(0), FLAG_VALUE) if k == 0 else (None, mp.mpf(0), FLAG_NEG_INF)
    if s2 == 0:
        return _poisson(k, lam) + (FLAG_VALUE,)
    with_fp64 = float(lam) * float(lam)
    alpha64 = with_fp64 / float(s2) + a if math.isfinite(with_fp64) else math.inf
    beta64 = float(lam) / float(s2)
    if not (math.isfinite(alpha64) and math.isfinite(beta64)):
        return None, mp.mpf(0), FLAG_NAN
    alpha = lam * lam / s2 + a
    beta = lam / s2
    t = (alpha * mp.log(beta), mp.loggamma(k + alpha), -mp.loggamma(k + 1), -(k + alpha) * mp.log(1 + beta),
         -mp.loggamma(alpha))
    return mp.fsum(t), mp.fsum(abs(x) for x in t), FLAG_VALUE


def _conv_poisson(k, l, s):
    """stats.py:479-527 -> (value, m)"""
    l, k, s = max(SMALL_POS, l), max(SMALL_POS, k), max(SMALL_POS, s)
    st = 2 * (50 + 1)
    lg = mp.loggamma(k + 1)
    log_s, half = mp.log(s), mp.log(_TWO_PI) / 2
    conv, norm, m = mp.mpf(0), mp.mpf(0), mp.mpf(0)
    opened = False
    for j in range(st - 1):
        x = -3 * s + j * (6 * s / (st - 1)) + 3 * s / (st - 1)
        cy = -log_s - half - x * x / (2 * s * s)
        norm += mp.exp(cy)
        fx = x + l
        opened = opened or fx > 0
        if opened:
            a = k * mp.log(fx)
            conv += mp.exp(cy + (a - fx - lg))
            m = max(m, abs(a) + fx + abs(lg) + abs(cy))
    return conv / norm, m


def _norm_conv_poisson(k, l, s):
    """stats.py:529-556 -> (value or None for NaN, m)"""
    cp, m1 = _conv_poisson(k, l, s)
    n2, m2 = _conv_poisson(l, l, s)
    if l == 0:
        return None, max(m1, m2)           # exp(log_poisson(0, 0)): 0 * ln 0
    n1 = mp.exp(l * mp.log(l) - l - mp.loggamma(l + 1))
    return cp * n1 / n2, max(m1, m2)


def per_bin(kind, k, lam, s2):
    """-> (value mpf or None, m mpf, flag) of one bin; k, lam, s2 fp64 numbers, finite and non-negative"""
    k, lam, s2 = _f(k), _f(lam), _f(s2)
    if kind == "conv_llh":
        s = mp.sqrt(s2)
        a, ma = _norm_conv_poisson(k, lam, s)
        b, mb = _norm_conv_poisson(k, k, s)
        a = SMALL_POS if a is None or not a > SMALL_POS else a
        b = SMALL_POS if b is None or not b > SMALL_POS else b
        return mp.log(a) - mp.log(b), max(ma, mb), FLAG_VALUE
    if lam < SMALL_POS:
        lam = SMALL_POS
    if kind == "llh":
        if k == 0:
            return None, lam, FLAG_NAN
        a, c = k * mp.log(lam), k * mp.log(k)
        return (a - lam) - (c - k), abs(a) + lam + abs(c) + k, FLAG_VALUE
    if kind == "poisson_llh":
        return _poisson(k, lam) + (FLAG_VALUE,)
    if kind == "chi2":
        v = (k - lam) ** 2 / lam
        return v, abs(v), FLAG_VALUE
    if kind == "mod_chi2":
        v = (k - lam) ** 2 / (s2 + lam)
        return v, abs(v), FLAG_VALUE
    if kind == "correct_chi2":
        q, lg = (k - lam) ** 2 / (s2 + lam), mp.log(s2 + lam)
        return q + lg, q + abs(lg), FLAG_VALUE
    if kind == "signed_sqrt_mod_chi2":
        v = (k - lam) / mp.sqrt(s2 + lam)
        return v, abs(v), FLAG_VALUE
    if kind in ("mcllh_mean", "mcllh_eff"):
        return _mixture(k, lam, s2, 1 if kind == "mcllh_eff" else 0)
    raise ValueError(kind)


def hi_lo(v):
    """an mpf as a pair of doubles: hi the nearest fp64, lo the nearest fp64 of the rest"""
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def evaluate(kind, k, lam, s2):
    """arrays -> (hi, lo, m, flag) lists of Python numbers; hi = NaN / -inf and lo = m = 0 where flagged"""
    hi, lo, m, flag = [], [], [], []
    for kk, ll, ss in zip(k, lam, s2):
        v, mm, fl = per_bin(kind, kk, ll, ss)
        if fl == FLAG_VALUE:
            h, r = hi_lo(v)
            hi.append(h), lo.append(r), m.append(float(mm))
        else:
            hi.append(math.nan if fl == FLAG_NAN else -math.inf), lo.append(0.0), m.append(0.0)
        flag.append(fl)
    return hi, lo, m, flag
