"""Shared pieces of the tests of the MC-uncertainty metrics in the trial-ensemble matrix (csrc/ensemble_mc.hip:
`pisa_hip_metric_matrix_mc`, `pisa_hip_metric_matrix_mc_best`): the seeded case families, exact values, a numpy
restatement of the kernels' arithmetic (hoisting included) and the gate.  A plain helper module (no fixtures);
`tests/test_host_ensemble_mc.py` pins everything here without a GPU, `tests/test_gpu_ensemble_mc.py` runs the kernels.
It builds on tests/ensemble_cases.py (`_rs`, `two_sum`, `gate_ratio`, `check`, `reduce_matrix`, `_exact_metric`) and
tests/metric_cases.py.

M[t, k] = nansum_b w(kind, D[t, b], E[k, b], S2[k, b]) for correct_chi2, mcllh_mean, mcllh_eff and conv_llh, w the
per-bin formula of `metric_bin_wide` (csrc/metric_flux.hip).

The gate, per entry, is that of tests/ensemble_cases.py:

    |got - exact| <= G * eps * sum_b (m_b + 1)

with m_b what oracle/exact_metric.py defines per kind and G = metric_cases.KERNEL_FACTOR * max(1, G_REF[kind]).  G_REF
is the worst ratio of `direct_form_mc`, the numpy fp64 restatement of what the kernels compute, over the kind's family
and every shape below; `tests/test_host_ensemble_mc.py` measures it again and holds it against these figures.  It is
never taken from the device.  Measured (numpy 2.2, scipy 1.15):

    correct_chi2   mcllh_mean   mcllh_eff   conv_llh      ->  G
    1.96           0.94         1.43        1.04              7.84  4  5.72  4.16

None exceeds G_HOST = 2.  correct_chi2's 1.96 is the formula's own error, as chi2's 1.99 in tests/ensemble_cases.py:
(d - lam)^2 / (s2 + lam) with d - lam and s2 + lam rounded.  Hoisting moves no figure: c0 = alpha ln beta - lgamma(alpha)
is two of the five terms m counts, rounded once more; conv_llh's second term taken as exp(log_poisson(d, d)) drops
the two roundings of the quotient it replaces.

Families (`family(name, T, K, B)` -> dict(D, E, S2, iD, iE)); rows 1::5 of the data are all zeros, the first template
row carries the palette's entries in order, the rest are seeded draws:
    mc_sigma    correct_chi2, mcllh_mean, mcllh_eff.  Expectations lam = 10^linspace(log10 0.3, 6, 8) at the widths
                s2 = w lam, w in (0, 1e-6, 1e-2, 1, 1e3), after the clipped expectations (0, 1e-300, 1e-11, 1e-10,
                5e-11) with s2 (0, 0, 1e-12, 1e-10, 1); data 0, rint(lam), 1.1 lam, 1, 2, 170, 171: 945 triples, every
                one a finite value of the exact oracle.  (The overflowing widths of metric_cases' `sigma` family give
                NaN bins by definition; tests/test_gpu_metric_exact.py holds them.)
    mc_conv     conv_llh.  k in (0, 1, 2.5, 40), lam = k (0.5, 1, 1.3) (k = 0: 0.5, 0, 1.3, as metric_cases), widths
                (0, 1e-3, 0.1, 0.5, 1, 3) sqrt(lam) cut to float32 so that s2 is exact; data (0, 1, 2.5, 3, 40, 52):
                432 triples, about 40 ms each in mpmath -- one table per session, shared by all shapes.
    mc_poisson  Poisson draws around templates of 1e-2 ... 1e3, s2 = |e randn|.  No exact values: the bit-for-bit
                properties only.
"""
import numpy as np
from scipy.special import gammaln

from tests import ensemble_cases as ec
from tests import metric_cases as mc

EPS = mc.EPS
SMALL_POS = mc.SMALL_POS
KINDS = ("correct_chi2", "mcllh_mean", "mcllh_eff", "conv_llh")
CHEAP_KINDS = KINDS[:3]
LLH_KINDS = KINDS[1:]              # maximised
G_HOST = mc.G_HOST

# worst ratio of `direct_form_mc` against the exact values (module docstring)
G_REF = {"correct_chi2": 1.96, "mcllh_mean": 0.94, "mcllh_eff": 1.43, "conv_llh": 1.04}

SIZES = (1, 15, 16, 17, 33)
BINS = (1, 3, 64, 65, 130)
BIG_SHAPE = (70, 33, 130)
STRIP_SHAPE = (1000, 40, 8)
CHEAP_SHAPES = tuple((t, k, b) for t in SIZES for k in SIZES for b in BINS) + (BIG_SHAPE, STRIP_SHAPE)
CONV_SHAPES = ((1, 1, 1), (16, 17, 4), (17, 16, 5), (33, 15, 3), (70, 33, 13))


def family_of(kind):
    return "mc_conv" if kind == "conv_llh" else "mc_sigma"


def shapes_of(kind):
    return CONV_SHAPES if kind == "conv_llh" else CHEAP_SHAPES


def g_of(kind):
    return mc.KERNEL_FACTOR * max(1.0, G_REF[kind])


# ------------------------------------------------------------------------------------- case families
CLIPPED = (0.0, 1e-300, 1e-11, 1e-10, 5e-11)
CLIPPED_S2 = (0.0, 0.0, 1e-12, 1e-10, 1.0)
SIGMA_WIDTHS = (0.0, 1e-6, 1e-2, 1.0, 1e3)
CONV_K = (0.0, 1.0, 2.5, 40.0)
CONV_RATIOS = mc.CONV_RATIOS
CONV_WIDTHS = (0.0, 1e-3, 0.1, 0.5, 1.0, 3.0)
CONV_DATA = (0.0, 1.0, 2.5, 3.0, 40.0, 52.0)


def _palettes(name):
    """-> (PD, PE, PS2): the data palette and the (expectation, sigma2) palette of a family"""
    if name == "mc_sigma":
        lam = 10 ** np.linspace(np.log10(0.3), 6, 8)
        pe = np.concatenate([CLIPPED, np.tile(lam, len(SIGMA_WIDTHS))])
        ps2 = np.concatenate([CLIPPED_S2] + [w * lam for w in SIGMA_WIDTHS])
        pd = np.concatenate([[0.0], np.rint(lam), 1.1 * lam, [1.0, 2.0, 170.0, 171.0]])
        return pd, pe, ps2
    if name == "mc_conv":
        ls, ss = [], []
        for kk in CONV_K:
            for r in CONV_RATIOS:
                ll = (kk if kk > 0 else 1.0) * r if (kk > 0 or r != 1.0) else 0.0      # k = 0: lam = 0.5, 0, 1.3
                for w in CONV_WIDTHS:
                    ls.append(ll)
                    ss.append(float(np.float32(w * (np.sqrt(ll) if ll > 0 else 1.0))))
        sigma = np.array(ss)
        return np.array(CONV_DATA), np.array(ls), sigma * sigma
    raise KeyError(name)


_PAL = {}


def palettes(name):
    if name not in _PAL:
        _PAL[name] = _palettes(name)
        for a in _PAL[name]:
            a.setflags(write=False)
    return _PAL[name]


_FAM = {}


def family(name, T, K, B):
    """dict(D [T, B], E [K, B], S2 [K, B], iD, iE (None for `mc_poisson`)): seeded, built once, read-only"""
    key = (name, T, K, B)
    if key not in _FAM:
        rs = ec._rs(name, T, K, B)
        if name == "mc_poisson":
            e = 10 ** (-2 + 5 * rs.rand(K, B))
            d = rs.poisson(e[np.arange(T) % K]).astype(np.float64)
            f = dict(D=d, E=e, S2=np.abs(e * rs.randn(K, B)), iD=None, iE=None)
        else:
            pd, pe, ps2 = palettes(name)
            i_d = rs.randint(0, pd.size, (T, B))
            i_d[1::5] = 0                            # whole rows without data
            i_e = rs.randint(0, pe.size, (K, B))
            i_e[0] = np.arange(B) % pe.size          # the first template: the palette in order
            f = dict(D=pd[i_d], E=pe[i_e], S2=ps2[i_e], iD=i_d, iE=i_e)
        for v in f.values():
            if v is not None:
                v.setflags(write=False)
        _FAM[key] = f
    return _FAM[key]


# ------------------------------------------------------------------------------------------ exact values
_TABLE = {}


def exact_table(name, kind):
    """the (hi, lo, m, flag) tables [|PD|, |PE|] of a palette family: oracle.exact_metric on every triple, once"""
    if (name, kind) not in _TABLE:
        import mpmath as mp

        xm = ec._exact_metric()
        pd, pe, ps2 = palettes(name)
        with mp.workdps(80):
            hi, lo, m, flag = xm.evaluate(kind, np.repeat(pd, pe.size), np.tile(pe, pd.size), np.tile(ps2, pd.size))
        shape = (pd.size, pe.size)
        t = tuple(np.array(a).reshape(shape) for a in (hi, lo, m, flag))
        for a in t:
            a.setflags(write=False)
        _TABLE[(name, kind)] = t
    return _TABLE[(name, kind)]


_EXACT = {}


def exact(name, kind, T, K, B):
    """(value [T, K] np.longdouble, scale [T, K] = sum_b (m_b + 1)) as `ensemble_cases.exact` builds them: the
    (hi, lo) pairs summed in np.longdouble; computed once, shared"""
    key = (name, kind, T, K, B)
    if key not in _EXACT:
        f = family(name, T, K, B)
        hi, lo, m, flag = exact_table(name, kind)
        assert np.all(flag == mc.FLAG_VALUE)
        idx = (f["iD"][:, None, :], f["iE"][None, :, :])
        value = hi[idx].astype(np.longdouble).sum(axis=2) + lo[idx].astype(np.longdouble).sum(axis=2)
        scale = (m[idx] + 1.0).sum(axis=2)
        value.setflags(write=False), scale.setflags(write=False)
        _EXACT[key] = (value, scale)
    return _EXACT[key]


# ---------------------------------------------------------------- numpy restatement of csrc/ensemble_mc.hip
N_NODES = 101


def _nodes(s, c0):
    """`emc_node` for every j: x [..., 101], c_y [..., 101] from s [...] and c0 = -ln s - ln(2 pi) / 2"""
    s, c0 = np.asarray(s)[..., None], np.asarray(c0)[..., None]
    j = np.arange(N_NODES, dtype=np.float64)
    start, stop = -3 * s, 3 * s
    step = (stop - start) / N_NODES
    shift = 3 * s / float(N_NODES)
    x = (j * step + start) + shift
    return x, c0 - x * x / (2 * (s * s))


def _log_poisson(k, l):
    with np.errstate(all="ignore"):
        return k * np.log(l) - l - gammaln(k + 1)


def prepare(kind, D, E, S2):
    """`emc_prep_kernel`: -> (template planes, data planes), each a tuple of arrays of the rows' shape"""
    with np.errstate(all="ignore"):
        lam = np.where(E < SMALL_POS, SMALL_POS, E)
        if kind == "correct_chi2":
            tv = S2 + lam
            return (lam, tv, np.log(tv)), ()
        if kind in ("mcllh_mean", "mcllh_eff"):
            a = 1.0 if kind == "mcllh_eff" else 0.0
            s2 = np.where(S2 > 0, S2, 1.0)
            alpha = (lam * lam) / s2 + a
            beta = lam / s2 + 0.0
            mix = S2 > 0
            p0 = np.where(mix, alpha, np.where(S2 == 0, -1.0, -2.0))
            p1 = np.where(mix, alpha * np.log(beta) - gammaln(alpha), np.where(S2 == 0, np.log(lam), 0.0))
            p2 = np.where(mix, np.log1p(beta), np.where(S2 == 0, lam, 0.0))
            return (p0, p1, p2), (gammaln(D + 1.0),)
        assert kind == "conv_llh"
        sq = np.sqrt(S2)
        s = np.where(sq > SMALL_POS, sq, SMALL_POS)
        lc = np.where(E > SMALL_POS, E, SMALL_POS)
        c0 = -np.log(s) - 0.5 * np.log(2 * 3.141592653589793)
        x, cy = _nodes(s, c0)
        lg = gammaln(lc + 1)
        norm, conv = np.zeros_like(E), np.zeros_like(E)
        for j in range(N_NODES):                        # both sums in node order, as the kernel adds them
            norm = norm + np.exp(cy[..., j])
            fx = x[..., j] + lc
            fy = lc * np.log(fx) - fx - lg
            conv = conv + np.where(fx > 0, np.exp(cy[..., j] + np.where(np.isnan(fy), 0.0, fy)), 0.0)
        n1 = np.exp(_log_poisson(E, E))
        dc = np.where(D > SMALL_POS, D, SMALL_POS)
        n1d = np.exp(_log_poisson(D, D))
        return (norm, n1, conv / norm, c0, s), (gammaln(dc + 1), np.log(np.where(n1d > SMALL_POS, n1d, SMALL_POS)))


def bin_values(kind, d, g, e, p):
    """the pair part of one bin: d [T], g the data planes [T], e [K], p the template planes [K] -> [T, K]"""
    d = d[:, None]
    with np.errstate(all="ignore"):
        if kind == "correct_chi2":
            dl = d - p[0][None, :]
            return (dl * dl) / p[1][None, :] + p[2][None, :]
        if kind in ("mcllh_mean", "mcllh_eff"):
            a, b1, b2, lg1 = p[0][None, :], p[1][None, :], p[2][None, :], g[0][:, None]
            mix = ((b1 + gammaln(d + np.where(a >= 0, a, 1.0))) - lg1) - (d + a) * b2
            return np.where(a >= 0, mix, np.where(a == -1.0, (d * b1 - b2) - lg1, np.where(d == 0, 0.0, -np.inf)))
        norm, n1, n2, c0, s = p
        lc = np.where(e > SMALL_POS, e, SMALL_POS)
        x, cy = _nodes(s, c0)
        fx = x + lc[:, None]
        opened = fx > 0
        L = np.where(opened, np.log(np.where(opened, fx, 1.0)), 0.0)
        q = np.where(opened, cy - fx, -np.inf)
        dc = np.where(d > SMALL_POS, d, SMALL_POS)
        lg, lb = g[0][:, None], g[1][:, None]
        conv = np.zeros((d.shape[0], e.shape[0]))
        for j in range(N_NODES):
            conv = conv + np.exp((dc * L[None, :, j] + q[None, :, j]) - lg)
        a = (conv / norm[None, :]) * n1[None, :] / n2[None, :]
        return np.log(np.where(a > SMALL_POS, a, SMALL_POS)) - lb


def direct_form_mc(kind, D, E, S2):
    """csrc/ensemble_mc.hip in numpy fp64: the preparation per row, the pair part per bin, and per (t, k) ONE
    compensated chain over the bins in ascending order, NaN bins dropped"""
    D, E, S2 = (np.asarray(a, dtype=np.float64) for a in (D, E, S2))
    P, G = prepare(kind, D, E, S2)
    s = np.zeros((D.shape[0], E.shape[0]))
    c = np.zeros_like(s)
    for b in range(D.shape[1]):
        v = bin_values(kind, D[:, b], tuple(g[:, b] for g in G), E[:, b], tuple(p[:, b] for p in P))
        s, c = ec.two_sum(s, c, np.where(np.isnan(v), 0.0, v))
    return s + c


def reduce_matrix(kind, M, offset=None, k0=0):
    """`ensemble_cases.reduce_matrix` with the llh kinds of this module maximised"""
    return ec.reduce_matrix("llh" if kind in LLH_KINDS else "chi2", M, offset, k0)


def scale_mc(kind, D, E, S2):
    """sum_b (m_b + 1) in fp64, [T, K], m_b as oracle/exact_metric.py lists it per kind: the gate's scale where no
    exact table is at hand"""
    D, E, S2 = (np.asarray(a, dtype=np.float64) for a in (D, E, S2))
    d, e, s2 = D[:, None, :], E[None, :, :], S2[None, :, :]
    lam = np.maximum(e, SMALL_POS)
    with np.errstate(all="ignore"):
        if kind == "correct_chi2":
            m = (d - lam) ** 2 / (s2 + lam) + np.abs(np.log(s2 + lam))
        elif kind in ("mcllh_mean", "mcllh_eff"):
            a = 1.0 if kind == "mcllh_eff" else 0.0
            sp = np.where(s2 > 0, s2, 1.0)
            alpha, beta = lam * lam / sp + a, lam / sp
            mix = (np.abs(alpha * np.log(beta)) + np.abs(gammaln(d + alpha)) + np.abs(gammaln(d + 1))
                   + np.abs((d + alpha) * np.log1p(beta)) + np.abs(gammaln(alpha)))
            poisson = np.where(d > 0, np.abs(d * np.log(lam)), 0.0) + lam + np.abs(gammaln(d + 1))
            m = np.where(s2 > 0, mix, poisson)
        else:
            s = np.maximum(np.sqrt(s2), SMALL_POS)
            x, cy = _nodes(s, -np.log(s) - 0.5 * np.log(2 * np.pi))
            m = np.zeros(np.broadcast_shapes(d.shape, e.shape))
            for k, l in ((d, e), (e, e), (d, d)):
                k, l = np.maximum(k, SMALL_POS)[..., None], np.maximum(l, SMALL_POS)[..., None]
                fx = x + l
                t = np.abs(k * np.log(np.where(fx > 0, fx, 1.0))) + fx + np.abs(gammaln(k + 1)) + np.abs(cy)
                m = np.maximum(m, np.where(fx > 0, t, 0.0).max(axis=-1))
    return (m + 1.0).sum(axis=2)


class NumpySolverMC:
    """the batch evaluator of pisa_amd/analysis/ensemble.py on the restatement: what the host tests run everything
    around the kernels with"""

    def __init__(self):
        self.calls = []

    def matrix(self, kind, data, expected, sigma2=None):
        self.calls.append(("matrix", kind, np.shape(data), np.shape(expected)))
        return direct_form_mc(kind, data, expected, sigma2)

    def best(self, kind, data, expected, sigma2=None, offset=None, k0=0):
        self.calls.append(("best", kind, np.shape(data), np.shape(expected)))
        return reduce_matrix(kind, direct_form_mc(kind, data, expected, sigma2), offset, k0)
