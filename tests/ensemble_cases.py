"""Shared pieces of the tests of the trial-ensemble kernels (csrc/ensemble.hip: `pisa_hip_metric_matrix`,
`pisa_hip_metric_matrix_best`) and of pisa_amd/analysis/ensemble.py: the seeded case families, exact values, numpy
restatements of both kernel forms and of the batch evaluator, and the gate.  A plain helper module (no fixtures);
`tests/test_host_ensemble.py` pins everything here without a GPU, `tests/test_gpu_ensemble.py` runs the kernels.

M[t, k] = nansum_b metric_bin(kind, D[t, b], E[k, b], S2[k, b]) for the four fused kinds, chi2 with its whole-map rule
(stats.py:160-163) per (t, k) pair.

The gate, per entry:

    |got - exact| <= G * eps * sum_b (m_b + 1)        over the bins the sum keeps (an llh bin without data is dropped)

with m_b what oracle/exact_metric.py defines per kind (the sum of the absolute values of the terms the fp64 formula adds
and subtracts), and G = metric_cases.KERNEL_FACTOR * max(1, G_REF[form, kind]).  G_REF is the worst ratio
|value - exact| / (eps sum_b (m_b + 1)) of the numpy fp64 restatement of the form (`direct_form`, `product_form`) over
every family and shape below; `tests/test_host_ensemble.py` measures it again and holds it against these figures.  It is
never taken from the device.  Measured (numpy 2.2, scipy 1.15):

    form      llh      poisson_llh   chi2     mod_chi2      ->  G
    direct    1.11     1.53          1.99     1.99              4.44  6.12  7.96  7.96
    product   1.95     1.58          -        -                 7.8   6.32

Both forms carry every sum over bins as ONE chain in ascending order with the rounding error of each addition kept
(`two_sum`), because a plain chain does not meet G_HOST = 2: over these families its worst ratios are 5.7 / 10.5 / 12.1 /
10.2 (direct) and 11.8 / 9.4 (product), growing like the square root of the number of bins.  What is left is the per-bin
formula's own error (chi2: up to 2 eps of the value, from (d - mu)^2 / mu with d - mu rounded), lgamma's, and in the
product form the matrix core's plain accumulator over the 16 bins between two joins.

Exact values.  Every family draws its data and its expectations from two small palettes (at most 2 10^4 distinct
(d, mu, sigma2) triples per family), so one table per (family, kind) of `oracle.exact_metric.evaluate` (mpmath, 80
digits), computed at test time and shared by all shapes, gives every bin of every shape; an entry is the sum of its
bins' (hi, lo) pairs in np.longdouble (pairwise: 130 bins add about 0.002 eps sum m to the exact value's own error).
The `poisson` family (Poisson draws around the templates, the only one with more distinct pairs than a table can hold)
is integer data and takes `exact_longdouble`: the four formulae in np.longdouble (eps 1.1e-19), lgamma(d + 1) from a
running longdouble sum of ln i.

Families (index palettes; `family(name, T, K, B)` -> dict(D, E, S2, iD, iE)):
    edges    expectations 0, 1e-300, 1e-11, 5e-11, just below / at / above SMALL_POS, 2^30; data 0 in whole rows and whole
             columns, counts 1, 2, 170, 171, 2^30; the first template row carries the clipped expectations in order
    asimov   non-integer data: a template row times (1 +- 1e-9 ... 1e-1)
    large    counts to 1e9, expectations within 1e-6 of them and a factor 2 away
    sigma    sigma2 from 0 to 1e6 mu (read by mod_chi2 alone)
    equal    integer data, but ONE data row identical to one template row: chi2's whole-map rule fires for that pair only
    poisson  Poisson draws around the template rows (expectations 1e-2 ... 1e3, the clipped ones in the first row)
"""
import zlib

import numpy as np
from scipy.special import gammaln

from tests import metric_cases as mc

EPS = mc.EPS
SMALL_POS = mc.SMALL_POS
KINDS = mc.FUSED_KINDS
LLH_KINDS = ("llh", "poisson_llh")
FORMS = ("direct", "product")
G_HOST = mc.G_HOST

# worst ratio of the numpy restatements against the exact values (module docstring)
G_REF = {("direct", "llh"): 1.11, ("direct", "poisson_llh"): 1.53, ("direct", "chi2"): 1.99,
         ("direct", "mod_chi2"): 1.99, ("product", "llh"): 1.95, ("product", "poisson_llh"): 1.58}

PALETTE_FAMILIES = ("edges", "asimov", "large", "sigma", "equal")
FAMILIES = PALETTE_FAMILIES + ("poisson",)

SIZES = (1, 15, 16, 17, 33)
BINS = (1, 3, 4, 5, 127, 128, 130)
BIG_SHAPE = (70, 33, 130)
STRIP_SHAPE = (1000, 40, 8)        # more strips of trials than one pass of the grid's workgroups
TILE_SHAPE = (64, 300, 12)         # many template tiles per strip (the reduced output)
SHAPES = tuple((t, k, b) for t in SIZES for k in SIZES for b in BINS) + (BIG_SHAPE, STRIP_SHAPE, TILE_SHAPE)


def forms_of(kind):
    return FORMS if kind in LLH_KINDS else FORMS[:1]


def g_of(form, kind):
    return mc.KERNEL_FACTOR * max(1.0, G_REF[(form, kind)])


# ------------------------------------------------------------------------------------- case families
DELTAS = (1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3, 0.1, -0.1)
_BELOW, _ABOVE = float(np.nextafter(1e-10, 0.0)), float(np.nextafter(1e-10, 1.0))
CLIPPED = (0.0, 1e-300, 1e-11, 1e-10, 5e-11, _BELOW, _ABOVE)


def _rs(*key):
    return np.random.RandomState(zlib.crc32("/".join(str(k) for k in key).encode()) & 0x7FFFFFFF)


def _palettes(name):
    """-> (PD, PE, PS2): the data palette and the (expectation, sigma2) palette of a family"""
    if name == "edges":
        pe = np.array(CLIPPED + (0.5, 1.0, 2.5, 170.0, 171.5, 2.0 ** 30, 1.5 * 2.0 ** 30))
        pd = np.array([0.0, 1.0, 2.0, 170.0, 171.0, 2.0 ** 30, 3.0, 50.0])
        return pd, pe, np.zeros_like(pe)
    if name == "asimov":
        pe = 10 ** np.linspace(-2, 3, 24) * (1 + 0.01 * np.sin(np.arange(24.0)))
        pd = np.concatenate([pe * (1 + d) for d in DELTAS])          # value (delta i, expectation j) at 24 i + j
        return pd, pe, np.zeros_like(pe)
    if name == "large":
        pd = np.rint(10 ** np.linspace(3, 9, 24))
        pe = np.concatenate([pd * r for r in (1 - 1e-6, 1.0, 1 + 1e-6, 2.0)])   # (ratio i, count j) at 24 i + j
        return pd, pe, np.zeros_like(pe)
    if name == "sigma":
        lam = 10 ** np.linspace(np.log10(0.3), 6, 8)
        widths = (0.0, 1e-6, 1e-2, 1.0, 1e3, 1e6)
        pe = np.tile(lam, len(widths))                               # (width i, expectation j) at 8 i + j
        ps2 = np.concatenate([w * lam for w in widths])
        pd = np.concatenate([np.zeros_like(lam), np.rint(lam), lam * 1.1])
        return pd, pe, ps2
    if name == "equal":
        pe = 10 ** np.linspace(-0.5, 2.7, 30) * (1 + 0.02 * np.cos(np.arange(30.0)))
        counts = np.unique(np.rint(np.concatenate([pe * 0.8, pe, pe * 1.3])))
        return np.concatenate([counts, pe]), pe, np.zeros_like(pe)   # the expectations themselves from len(counts) on
    raise KeyError(name)


_PAL = {}


def palettes(name):
    if name not in _PAL:
        _PAL[name] = _palettes(name)
        for a in _PAL[name]:
            a.setflags(write=False)
    return _PAL[name]


def _indices(name, T, K, B):
    """index arrays iD [T, B] into PD and iE [K, B] into (PE, PS2)"""
    rs = _rs(name, T, K, B)
    pd, pe, _ = palettes(name)
    if name == "edges":
        i_d = rs.randint(0, pd.size, (T, B))
        i_d[1::5] = 0                            # whole rows without data
        i_d[:, 2::4] = 0                         # whole columns without data
        i_e = rs.randint(0, pe.size, (K, B))
        i_e[0] = np.arange(B) % len(CLIPPED)     # the first template: the clipped expectations in order
        return i_d, i_e
    if name == "asimov":
        i_e = rs.randint(0, 24, (K, B))
        t = np.arange(T)
        i_d = 24 * ((t // K + t) % len(DELTAS))[:, None] + i_e[t % K]
        return i_d, i_e
    if name in ("large", "sigma"):
        n = 24 if name == "large" else 8
        n_var = 4 if name == "large" else 6
        col = rs.randint(0, n, B)                # most pairs of a column are near each other, some are far apart
        j_d = np.where(rs.rand(T, B) < 0.7, col[None, :], rs.randint(0, n, (T, B)))
        j_e = np.where(rs.rand(K, B) < 0.7, col[None, :], rs.randint(0, n, (K, B)))
        if name == "large":
            return j_d, n * rs.randint(0, n_var, (K, B)) + j_e
        return n * rs.randint(0, 3, (T, B)) + j_d, n * rs.randint(0, n_var, (K, B)) + j_e
    if name == "equal":
        n_counts = pd.size - pe.size
        i_e = rs.randint(0, pe.size, (K, B))
        i_d = rs.randint(0, n_counts, (T, B))
        i_d[T // 2] = n_counts + i_e[K // 3]     # ONE data row is a template row
        return i_d, i_e
    raise KeyError(name)


_FAM = {}


def family(name, T, K, B):
    """dict(D [T, B], E [K, B], S2 [K, B], iD, iE (None for `poisson`)): seeded, built once, read-only"""
    key = (name, T, K, B)
    if key not in _FAM:
        if name == "poisson":
            rs = _rs(name, T, K, B)
            e = 10 ** (-2 + 5 * rs.rand(K, B))
            e[0, :min(B, len(CLIPPED))] = CLIPPED[:min(B, len(CLIPPED))]
            d = rs.poisson(e[np.arange(T) % K]).astype(np.float64)
            f = dict(D=d, E=e, S2=np.abs(e * rs.randn(K, B)), iD=None, iE=None)
        else:
            pd, pe, ps2 = palettes(name)
            i_d, i_e = _indices(name, T, K, B)
            f = dict(D=pd[i_d], E=pe[i_e], S2=ps2[i_e], iD=i_d, iE=i_e)
        for v in f.values():
            if v is not None:
                v.setflags(write=False)
        _FAM[key] = f
    return _FAM[key]


# ------------------------------------------------------------------------------------------ exact values
def chi2_rule(D, E):
    """[T, K] bool: stats.py:160-161, all |d - max(mu, SMALL_POS)| < 5 eps, in fp64 as the reference forms it"""
    lc = np.maximum(E, SMALL_POS)
    return np.all(np.abs(D[:, None, :] - lc[None, :, :]) < 5 * EPS, axis=2)


_TABLE = {}
_XM = None


def _exact_metric():
    """oracle/exact_metric.py, loaded under a private name and with mpmath's global precision put back: the module sets
    the precision where it is first imported, and tests that run later in a session (tests/test_host_metric_cases.py
    after the hypersurface generator has set its own) rely on THEIR import doing so.  Every call here runs under
    `workdps(80)` instead."""
    global _XM
    if _XM is None:
        import importlib.util
        import os

        import mpmath as mp

        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "exact_metric.py")
        spec = importlib.util.spec_from_file_location("_ensemble_exact_metric", path)
        mod = importlib.util.module_from_spec(spec)
        dps = mp.mp.dps
        try:
            spec.loader.exec_module(mod)
        finally:
            mp.mp.dps = dps
        _XM = mod
    return _XM


def exact_table(name, kind):
    """the (hi, lo, m, live) tables [|PD|, |PE|] of a palette family: oracle.exact_metric on every pair, once"""
    if (name, kind) not in _TABLE:
        import mpmath as mp

        xm = _exact_metric()
        pd, pe, ps2 = palettes(name)
        assert pd.size * pe.size <= 20000
        k = np.repeat(pd, pe.size)
        with mp.workdps(80):
            hi, lo, m, flag = xm.evaluate(kind, k, np.tile(pe, pd.size), np.tile(ps2, pd.size))
        live = (np.array(flag) == xm.FLAG_VALUE).reshape(pd.size, pe.size)
        assert kind == "llh" or live.all()
        assert np.array_equal(~live, np.repeat(pd == 0, pe.size).reshape(live.shape)) or kind != "llh"
        shape = (pd.size, pe.size)
        _TABLE[(name, kind)] = (np.where(live, np.array(hi).reshape(shape), 0.0), np.array(lo).reshape(shape),
                                np.array(m).reshape(shape), live)
    return _TABLE[(name, kind)]


def exact_longdouble(kind, D, E, S2):
    """the four formulae in np.longdouble for INTEGER data -> (value [T, K] longdouble, scale [T, K] float):
    lgamma(d + 1) from a running longdouble sum of ln i"""
    ld = np.longdouble
    assert np.array_equal(D, np.rint(D)) and D.min() >= 0 and D.max() < 1e7
    d = D.astype(ld)[:, None, :]
    lam = np.maximum(E, SMALL_POS).astype(ld)[None, :, :]
    live = np.ones(np.broadcast_shapes(d.shape, lam.shape), dtype=bool)
    if kind in LLH_KINDS:
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(d > 0, d * np.log(lam), ld(0))
            if kind == "llh":
                c = np.where(d > 0, d * np.log(np.where(d > 0, d, ld(1))), ld(0))
                v, m = (a - lam) - (c - d), np.abs(a) + lam + np.abs(c) + d
                live = np.broadcast_to(d > 0, live.shape)
            else:
                lg = np.concatenate([[ld(0)], np.cumsum(np.log(np.arange(1, int(D.max()) + 1, dtype=ld)))])
                c = lg[D.astype(np.int64)][:, None, :]
                v, m = (a - lam) - c, np.abs(a) + lam + np.abs(c)
    else:
        s2 = S2.astype(ld)[None, :, :] if kind == "mod_chi2" else ld(0)
        v = (d - lam) ** 2 / (s2 + lam)
        m = np.abs(v)
    value = np.where(live, v, ld(0)).sum(axis=2)
    scale = np.where(live, m + 1, ld(0)).sum(axis=2).astype(np.float64)
    if kind == "chi2":
        value = np.where(chi2_rule(D, E), ld(0), value)
    return value, scale


_EXACT = {}


def exact(name, kind, T, K, B):
    """(value [T, K] np.longdouble, scale [T, K] = sum over the kept bins of (m_b + 1)): computed once, shared"""
    key = (name, kind, T, K, B)
    if key not in _EXACT:
        f = family(name, T, K, B)
        if name == "poisson":
            value, scale = exact_longdouble(kind, f["D"], f["E"], f["S2"])
        else:
            hi, lo, m, live = exact_table(name, kind)
            idx = (f["iD"][:, None, :], f["iE"][None, :, :])
            lv = live[idx]
            value = hi[idx].astype(np.longdouble).sum(axis=2) + lo[idx].astype(np.longdouble).sum(axis=2)
            scale = np.where(lv, m[idx] + 1.0, 0.0).sum(axis=2)
            if kind == "chi2":
                value = np.where(chi2_rule(f["D"], f["E"]), np.longdouble(0), value)
        value.setflags(write=False), scale.setflags(write=False)
        _EXACT[key] = (value, scale)
    return _EXACT[key]


# ------------------------------------------------------------------------------------------- the gate
def gate_ratio(got, value, scale):
    """|got - exact| / (eps scale) per entry; an entry without a kept bin (scale 0) must be exactly 0"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got.astype(np.longdouble) - value).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, err / (EPS * np.where(scale > 0, scale, 1.0)), np.where(err == 0, 0.0, np.inf))


def check(got, value, scale, g, what=""):
    """every entry finite and inside the gate with G = `g` -> the worst ratio"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == value.shape, (what, got.shape, value.shape)
    assert np.all(np.isfinite(got)), what + ": non-finite entry"
    r = gate_ratio(got, value, scale)
    worst = float(r.max())
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    assert worst <= g, "%s: entry %s: got %.17g exact %.17g scale %.3g: %.3g eps scale > %.3g" % (
        what, i, got[i], float(value[i]), scale[i], worst, g)
    return worst


# ------------------------------------------------------------------------- numpy restatements of the forms
def lgamma1(d):
    """lgamma(d + 1) in fp64, elementwise (scipy's gammaln: within 1.5 eps absolute between 1 and 3, where glibc's
    lgamma is off by up to 7 eps)"""
    u, inv = np.unique(np.asarray(d, dtype=np.float64) + 1.0, return_inverse=True)
    return gammaln(u)[inv].reshape(np.shape(d))


def metric_bin(kind, d, lam, s2, lg=None):
    """csrc/metric_device.hpp in numpy: the same operations in the same order, unfused"""
    lam = np.where(lam < SMALL_POS, SMALL_POS, lam)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "llh":
            v = d * np.log(lam) - lam
            return v - (d * np.log(d) - d)          # d == 0 -> NaN, dropped by nansum
        if kind == "poisson_llh":
            return (d * np.log(lam) - lam) - (lgamma1(d) if lg is None else lg)
        delta = d - lam
        return (delta * delta) / lam if kind == "chi2" else (delta * delta) / (s2 + lam)


def two_sum(s, c, x):
    """`ens_two_sum` of csrc/ensemble.hip: (s, c) += x with the addition's rounding error kept in c"""
    t = s + x
    bb = t - s
    return t, c + ((s - (t - bb)) + (x - bb))


def direct_form(kind, D, E, S2=None):
    """the direct kernel: per (t, k) ONE compensated chain over the bins in ascending order, NaN bins dropped,
    chi2's rule"""
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    lg = lgamma1(D) if kind == "poisson_llh" else None
    s = np.zeros((D.shape[0], E.shape[0]))
    c = np.zeros_like(s)
    for b in range(D.shape[1]):
        v = metric_bin(kind, D[:, b, None], E[None, :, b], S2[None, :, b], None if lg is None else lg[:, b, None])
        s, c = two_sum(s, c, np.where(np.isnan(v), 0.0, v))
    acc = s + c
    if kind == "chi2":
        acc = np.where(chi2_rule(D, E), 0.0, acc)
    return acc


def _chain(x):
    """the preparation's constants: one compensated chain over the last axis -> the (hi, lo) pair"""
    s = np.zeros(x.shape[:-1])
    c = np.zeros_like(s)
    for b in range(x.shape[-1]):
        s, c = two_sum(s, c, x[..., b])
    hi = s + c
    return hi, (s - hi) + c


FLUSH_BINS = 16         # EP_FLUSH of csrc/ensemble.hip


def product_form(kind, D, E):
    """the product kernel: L = ln mu, s_k = sum_b mu and c_t as (hi, lo) pairs; the accumulator takes the bins in groups
    of 4 in ascending order (for llh the group's four d L, then its four (d > 0) (-mu)), joins the running (sum, comp)
    every 16 bins and restarts from zero; then (sum - s_k) - c_t with every rounding error kept and added last.
    Every product is rounded here; the matrix core may fuse it into the addition."""
    assert kind in LLH_KINDS
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    lam = np.where(E < SMALL_POS, SMALL_POS, E)
    L = np.log(lam)
    ind = (D > 0).astype(np.float64)
    if kind == "poisson_llh":
        c_hi, c_lo = _chain(lgamma1(D))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            c_hi, c_lo = _chain(np.where(D > 0, D * np.log(D) - D, 0.0))
    B = D.shape[1]
    s = np.zeros((D.shape[0], E.shape[0]))
    c = np.zeros_like(s)
    for f0 in range(0, B, FLUSH_BINS):
        acc = np.zeros_like(s)
        for g0 in range(f0, min(f0 + FLUSH_BINS, B), 4):
            for b in range(g0, min(g0 + 4, B)):
                acc = acc + D[:, b, None] * L[None, :, b]
            if kind == "llh":
                for b in range(g0, min(g0 + 4, B)):
                    acc = acc + ind[:, b, None] * (-lam[None, :, b])
        s, c = two_sum(s, c, acc)
    if kind == "poisson_llh":
        s_hi, s_lo = _chain(lam)
        s, c = two_sum(s, c, -s_hi[None, :])
        c = c - s_lo[None, :]
    s, c = two_sum(s, c, -c_hi[:, None])
    c = c - c_lo[:, None]
    return s + c


def form_values(form, kind, D, E, S2=None):
    return direct_form(kind, D, E, S2) if form == "direct" else product_form(kind, D, E)


def reduce_matrix(kind, M, offset=None, k0=0):
    """the reduced output restated on a full matrix: (best, arg: the smallest k attaining it, at)"""
    V = M if offset is None else M + np.asarray(offset, dtype=np.float64)[None, :]
    arg = np.argmax(V, axis=1) if kind in LLH_KINDS else np.argmin(V, axis=1)      # (the first of equal values)
    return V[np.arange(V.shape[0]), arg], arg.astype(np.int32), V[:, k0].copy()


class NumpySolver:
    """the batch evaluator of pisa_amd/analysis/ensemble.py restated in numpy (the direct form): what the host
    tests run everything around the kernels with"""

    def __init__(self, form="direct"):
        self.form = form
        self.calls = []

    def _form(self, kind):
        return self.form if kind in LLH_KINDS else "direct"

    def matrix(self, kind, data, expected, sigma2=None):
        self.calls.append(("matrix", kind, np.shape(data), np.shape(expected)))
        return form_values(self._form(kind), kind, data, expected, sigma2)

    def best(self, kind, data, expected, sigma2=None, offset=None, k0=0):
        self.calls.append(("best", kind, np.shape(data), np.shape(expected)))
        return reduce_matrix(kind, form_values(self._form(kind), kind, data, expected, sigma2), offset, k0)


def scale_fp64(kind, D, E, S2=None):
    """sum_b (m_b + 1) over the kept bins in fp64, [T, K]: the gate's scale where no exact table is at hand"""
    D, E = np.asarray(D, dtype=np.float64)[:, None, :], np.asarray(E, dtype=np.float64)[None, :, :]
    lam = np.maximum(E, SMALL_POS)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(D > 0, np.abs(D * np.log(lam)), 0.0)
        if kind == "llh":
            m = np.where(D > 0, a + lam + np.abs(D * np.log(np.where(D > 0, D, 1.0))) + D + 1.0, 0.0)
        elif kind == "poisson_llh":
            m = a + lam + np.abs(lgamma1(D)) + 1.0
        else:
            s2 = 0.0 if (kind == "chi2" or S2 is None) else np.asarray(S2, dtype=np.float64)[None, :, :]
            m = (D - lam) ** 2 / (s2 + lam) + 1.0
    return m.sum(axis=2)


# ---------------------------------------------------------- the drivers restated as the reference's loops
def toy_grid(metric, n_bins=24, seed=11):
    """a 3 x 3 grid of templates (two shape parameters around ~40 counts per bin) with errors and a priors penalty
    -> (hist [9, B], sumw2 [9, B], points [9, 2], penalty [9])"""
    rs = np.random.RandomState(seed)
    x = np.linspace(0.0, 1.0, n_bins)
    base = 40.0 * (1.0 + 0.5 * np.sin(5.0 * x)) + 5.0 * rs.rand(n_bins)
    a, b = np.meshgrid(np.linspace(0.0, 1.0, 3), np.linspace(0.0, 1.0, 3), indexing="ij")
    points = np.stack([a.ravel(), b.ravel()], axis=1)
    hist = np.stack([base * (1.0 + 0.16 * (p[0] - 0.5) * np.cos(3.0 * x) + 0.12 * (p[1] - 0.5) * x) for p in points])
    sumw2 = 0.3 * hist
    pull = ((points[:, 1] - 0.5) / 0.8) ** 2
    penalty = pull if metric in ("chi2", "mod_chi2") else -0.5 * pull
    return hist, sumw2, points, penalty


def loop_delta(metric_total, maps, templates, penalty, metric, k0):
    """the reference's loop: per data map the metric against every template + penalty, the best, minus / against k0"""
    out = []
    for m in maps:
        vals = np.array([metric_total(m, k) for k in range(len(templates))]) + penalty
        out.append(vals.max() - vals[k0] if metric in LLH_KINDS else vals[k0] - vals.min())
    return np.array(out)


def loop_feldman_cousins(metric_total, template_maps, penalty, metric, n_trials, cl, seed, true_points=None):
    """`feldman_cousins` as a plain loop over `Map.fluctuate` + a metric_total(data_map, k) -> (crit, deltas per point)"""
    crit, deltas = [], []
    for k0 in (range(len(template_maps)) if true_points is None else true_points):
        rs = np.random.RandomState([seed, k0])
        maps = [template_maps[k0].fluctuate("poisson", random_state=rs) for _ in range(n_trials)]
        d = loop_delta(metric_total, maps, template_maps, penalty, metric, k0)
        s = sorted(d)
        crit.append([s[int(np.ceil(c * n_trials)) - 1] for c in cl])
        deltas.append(d)
    return np.array(crit), deltas


def clear_of(values, crit, tol):
    """no value within 10 tol of `crit` but those EQUAL to it, and several equal ones only at 0 (the trial's best
    point is the true point: exactly 0 whoever computes it)"""
    v = np.asarray(values, dtype=np.float64)
    same = v == crit
    return bool(np.all(same | (np.abs(v - crit) > 10 * tol)) and (same.sum() <= 1 or crit == 0.0))
