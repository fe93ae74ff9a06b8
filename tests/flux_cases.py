"""Shared pieces of the tests of the flux chain (`pisa_hip_barr_simple[_multi]`, `pisa_hip_barr_factors` +
`pisa_hip_barr_fold_multi`, `pisa_hip_flux_2d`): an extended-precision restatement of the Barr systematics, the
seeded case families the GPU tests run, the gate they apply and the quadrature of the integral-preservation check.
A plain helper module (no fixtures); `tests/test_host_flux_cases.py` pins everything here without a GPU.

The gate.  Every output column is a product of well-conditioned factors and ONE factor that is not,
modRatioNuBar = max(0, d) or max(0, 1 / d) with d = 1 + m, m = 0.5 * Barr_nu_nubar_ratio * ModFlux: a relative
error delta of ModFlux is a relative error delta |m| / |d| of the result.  A fixed relative tolerance is therefore
too loose far from d = 0 and too tight close to it, and the tests ask, per event and column,

    |got - ext| <= G * eps * (1 + |m| / |d|) * |ext|

with `ext` the value of `barr_extended` (64-bit mantissa).  G is not chosen by looking at the kernel: G_REF below is
the worst such ratio of the reference's own fp64 values (tests/golden/barr_ref.npz, barr_wide_ref.npz) and of the C
oracle (glibc's log10, pow, exp) over every family of this module, and the kernels get KERNEL_FACTOR times that: the
device's log10, exp10, exp and log each differ from glibc's by a couple of ulp, and the two substitutions the kernels
make (exp10 for pow(10, .), exp(delta log x) for pow(x, delta)) add about two more.

ONE departure from that formula: at 1e-300 and 1e300 GeV, two of the six energies of the bad-energy family, the right
side carries one more factor |log10 E| / 5 = 60 (`gate_ratio`).  No fp64 evaluation meets the plain gate there: the
exponent t of LogLogParam's 10^t is about 140, a rounding error of t is a relative error ln(10) |t| eps of the result,
and the C oracle itself deviates by 123 eps from the extended value at 1e300 GeV (2.1 with the factor).  The factor is 1
for every other energy, the other four bad ones (0, -1, NaN, inf) included, which are held to the plain gate.

Measured figures (this module's families and the two goldens; `python oracle/measure_flux_refs.py` prints them):
    reference's own values   worst ratio 5.09   (barr_wide_ref.npz; barr_ref.npz: 2.66)   -> G_REF = 5.1
    C oracle                 worst ratio 4.10   (all four families; at 1e-300 / 1e300 GeV with the factor 60 above)
    smallest |d| of any family 1.2e-5, so the sign of d (the clamp) is never in doubt
`tests/test_host_flux_cases.py` measures them again and holds them against G_REF.
The kernels' own worst ratios are recorded in tests/test_gpu_flux.py.
"""
import os

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble

G_REF = 5.1                 # worst ratio of the reference's and the oracle's fp64 values (module docstring)
KERNEL_FACTOR = 4.0
N_FAMILY = 16 * 256 + 3     # 16 full blocks of the launch and 3 events of a 17th

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def extended_available():
    """True where np.longdouble has more mantissa bits than float64 (the rule of oracle/referee.py); where it
    has not, the tests that need `barr_extended` skip instead of comparing fp64 with fp64"""
    return int(np.finfo(np.longdouble).nmant) > 52


NO_EXTENDED = "np.longdouble carries no more than fp64's 53 bits on this host: no extended arithmetic to compare with"


# --------------------------------------------------------------- apply_sys_vectorized in np.longdouble
# barr_parameterization.py:17-113 and barr_simple.py:107-204 as oracle/pisa_oracle.c restates them; the
# constants are the fp64 ones, every operation on them is np.longdouble
def _c(x):
    return LD(float(x))


def _sign(v):
    return np.where(v == 0, LD(0), np.where(v >= 0, LD(1), LD(-1)))


def _loglog(e, y1, y2, x1, x2, cutoff):
    nu_nubar = _sign(y2)
    y1 = _sign(y1) * np.log10(np.abs(y1) + _c(0.0001))
    y2 = np.log10(np.abs(y2 + _c(0.0001)))
    mod = nu_nubar * np.power(LD(10), ((y2 - y1) / (x2 - x1)) * (np.log10(e) - x1) + y1 - LD(2))
    if cutoff is not None:
        mod = mod * np.exp(LD(-1) * e / cutoff)
    return mod


def _norm_fcn(x, a, sigma):
    pi = _c(np.pi)
    return a / np.sqrt(LD(2) * pi * (sigma * sigma)) * np.exp(-(x * x) / (LD(2) * (sigma * sigma)))


_E1MU, _E2MU, _E1E, _E2E = _c(3.0), _c(43), _c(2.5), _c(10)
_X1E, _X2E = _c(0.5), _c(3.0)
_Z1MU, _Z2MU, _Z1E, _Z2E = _c(0.6), _c(5.0), _c(0.3), _c(5.0)
_NUE_CUT, _NUMU_CUT = _c(650.0), _c(1000.0)
_X1Z, _X2Z = _c(0.5), _c(2.0)
_PIVOT = _c(24.0900951261)


def _modflux(flav, e, cz):
    if flav == 1:
        a_ave = _loglog(e, _E1MU, _E2MU, _X1E, _X2E, None)
        a_shape = _c(2.5) * _loglog(e, _Z1MU, _Z2MU, _X1Z, _X2Z, _NUMU_CUT)
        return a_ave - (_norm_fcn(cz, a_shape, _c(0.36)) - _c(0.6) * a_shape)
    a_ave = _loglog(e, _E1MU + _E1E, _E2MU + _E2E, _X1E, _X2E, None)
    a_shape = _loglog(e, _Z1MU + _Z1E, _Z2MU + _Z2E, _X1Z, _X2Z, _NUE_CUT)
    return a_ave - (_c(1.5) * _norm_fcn(cz, a_shape, _c(0.36)) - _c(0.7) * a_shape)


def _ratio_scale(scale, in1, in2):
    ratio = in1 / in2
    new = (in1 + in2) / (LD(1) + scale * ratio)
    both0 = (in1 == 0) & (in2 == 0)
    return np.where(both0, LD(0), scale * ratio * new), np.where(both0, LD(0), new)


def barr_extended(true_energy, true_coszen, nu_flux_nominal, nubar_flux_nominal, nubar, nue_numu_ratio,
                  nu_nubar_ratio, delta_index, Barr_uphor_ratio, Barr_nu_nubar_ratio):
    """`apply_sys_vectorized` in np.longdouble -> (out[n, 2], m[n, 2], d[n, 2]) as np.longdouble, with
    m = 0.5 * Barr_nu_nubar_ratio * ModFlux(flavour) and d = 1 + m per event and flavour column"""
    with np.errstate(all="ignore"):
        e = np.asarray(true_energy, dtype=np.float64).astype(LD)
        cz = np.asarray(true_coszen, dtype=np.float64).astype(LD)
        nu = np.asarray(nu_flux_nominal, dtype=np.float64).astype(LD)
        nub = np.asarray(nubar_flux_nominal, dtype=np.float64).astype(LD)
        r_flav, r_bar, delta = _c(nue_numu_ratio), _c(nu_nubar_ratio), _c(delta_index)
        uphor, sys = _c(Barr_uphor_ratio), _c(Barr_nu_nubar_ratio)
        nu0, nu1 = _ratio_scale(r_flav, nu[:, 0], nu[:, 1])
        nb0, nb1 = _ratio_scale(r_flav, nub[:, 0], nub[:, 1])
        idx_scale = np.power(e / _PIVOT, delta)
        nu0, nu1, nb0, nb1 = nu0 * idx_scale, nu1 * idx_scale, nb0 * idx_scale, nb1 * idx_scale
        e0, e1 = _ratio_scale(r_bar, nu0, nb0)
        m0, m1 = _ratio_scale(r_bar, nu1, nb1)
        o = [e1, m1] if nubar < 0 else [e0, m0]
        m = np.stack([_c(0.5) * (sys * _modflux(0, e, cz)), _c(0.5) * (sys * _modflux(1, e, cz))], axis=1)
        d = LD(1) + m
        for fl in (0, 1):
            # Python's max(0., x) and C's fmax(0., x) both give 0 for a NaN x
            fac = LD(1) / d[:, fl] if nubar < 0 else d[:, fl]
            o[fl] = o[fl] * np.where(fac > 0, fac, LD(0))
        a_shape = np.abs(uphor) * _loglog(e, _Z1E + _Z1MU, _Z2E + _Z2MU, _X1Z, _X2Z, _NUE_CUT)
        o[0] = o[0] * (LD(1) - _c(0.3) * _sign(uphor) * _norm_fcn(cz, a_shape, _c(0.35)))
        return np.stack(o, axis=1), m, d


def clamped(d, nubar):
    """where modRatioNuBar is max(0, .) = 0: d <= 0 for neutrinos, d < 0 for antineutrinos (1 / 0 = inf)"""
    return (d < 0) | ((d == 0) & (nubar > 0))


LOG_E_MAX = 5.0             # the largest |log10 E| of the families G_REF was measured on (0.1 GeV .. 100 TeV)


def gate_ratio(got, ext, m, d, energy):
    """|got - ext| / (eps * cond * |ext|) per element with cond = (1 + |m| / |d|) * max(1, |log10 E| / 5):
    0 where got == ext (zeros, infinities), NaN where either is NaN -- the NaN pattern is compared separately.
    The second factor of cond is 1 for every energy from 1e-5 to 1e5 GeV and wherever log10 E is not finite
    (E = 0, negative, NaN, inf).  It matters at 1e-300 and 1e300 GeV only (the bad-energy family): the exponent t
    of LogLogParam's 10^t grows like |log10 E|, and a rounding error of t is a relative error ln(10) |t| eps of
    the result, 60 times what it is at 100 TeV (module docstring)."""
    with np.errstate(all="ignore"):
        got = np.asarray(got, dtype=np.float64).astype(LD)
        log_e = np.log10(np.asarray(energy, dtype=np.float64))
        far = np.where(np.isfinite(log_e), np.maximum(1.0, np.abs(log_e) / LOG_E_MAX), 1.0)
        cond = (LD(1) + np.abs(m) / np.abs(d)) * far[:, None]
        r = np.abs(got - ext) / (LD(EPS) * cond * np.abs(ext))
        r = np.where(got == ext, LD(0), r)
        return r.astype(np.float64), cond.astype(np.float64)


def check_against_extended(got, ext, m, d, nubar, energy, g, what=""):
    """the assertions every Barr value test makes of a kernel's (or the oracle's) fp64 output `got[n, 2]`;
    -> the worst gate ratio.  NaN pattern and zero pattern equal to the extended value's, exactly 0.0 where the
    extended value is clamped, the conditioning-aware gate with G = `g` elsewhere, and the suite's plain
    rtol = 1e-12 as well wherever cond < 10."""
    got = np.asarray(got, dtype=np.float64)
    ext64 = ext.astype(np.float64)
    nan = np.isnan(ext64)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN pattern"
    assert np.array_equal(got == 0, ext64 == 0), what + ": zero pattern"
    cl = clamped(d, nubar) & ~nan
    assert np.all(got[cl] == 0.0), what + ": clamped events must be exactly 0"
    ratio, cond = gate_ratio(got, ext, m, d, energy)
    live = ~nan & ~cl
    worst = float(ratio[live].max()) if live.any() else 0.0
    assert worst <= g, "%s: worst |got - ext| / (eps cond |ext|) = %.3g > %.3g" % (what, worst, g)
    well = live & (cond < 10) & np.isfinite(ext64)
    np.testing.assert_allclose(got[well], ext64[well], rtol=1e-12, atol=0.0)
    return worst


# ------------------------------------------------------------------------------------- case families
PSETS_WIDE = (
    (1.2, 0.7, 0.3, 2.0, -2.0),       # reaches the clamp above about 5 TeV
    (0.5, 2.0, -0.3, -2.0, 2.0),
    (1.03, 0.9, 0.05, 0.0, -0.4),     # Barr_uphor_ratio = 0
    (0.0, 1.1, -0.1, 0.7, 1.0),       # nue_numu_ratio = 0
    (0.9, 1.0, 0.1, -0.6, -1.3),
    (1.0, 1.0, 0.0, 0.0, 0.0),
)
PSETS_CLAMP = ((1.2, 0.7, 0.3, 2.0, -2.0), (0.9, 1.1, -0.2, -1.0, 2.0), (1.0, 1.0, 0.0, 0.0, -2.0))
FLUX_PATTERNS = (((0, 0), (0, 0)), ((0, 1), (0, 1)), ((1, 0), (0, 0)), ((1, 0), (1, 0)), ((0, 0), (1, 1)))
BAD_ENERGIES = (0.0, -1.0, np.nan, np.inf, 1e-300, 1e300)


def _base(seed, lo, hi):
    rs = np.random.RandomState(seed)
    n = N_FAMILY
    e = 10 ** (np.log10(lo) + rs.rand(n) * (np.log10(hi) - np.log10(lo)))
    cz = rs.rand(n) * 2 - 1
    cz[:3] = [-1.0, 0.0, 1.0]
    return rs, dict(true_energy=e, true_coszen=cz, nu_flux_nominal=rs.rand(n, 2) * 10,
                    nubar_flux_nominal=rs.rand(n, 2) * 10)


def _make_families():
    fam = {}
    _, f = _base(101, 0.1, 1e5)
    fam["wide"] = dict(f, psets=PSETS_WIDE)
    _, f = _base(102, 3e3, 1e5)
    fam["clamp"] = dict(f, psets=PSETS_CLAMP)
    rs, f = _base(103, 0.1, 1e5)
    where = rs.choice(N_FAMILY, 400, replace=False)          # a tenth of the events, every pattern 80 times
    for k, i in enumerate(where):
        f["nu_flux_nominal"][i], f["nubar_flux_nominal"][i] = FLUX_PATTERNS[k % len(FLUX_PATTERNS)]
    fam["patterns"] = dict(f, psets=PSETS_WIDE[:4], pattern_rows=where)
    rs, f = _base(104, 0.1, 1e5)
    where = np.sort(rs.choice(np.arange(1, N_FAMILY - 1), 60, replace=False))
    where[:4] = [0, 255, 256, N_FAMILY - 1]                    # the launch's first and last thread, a block edge
    where = np.unique(where)
    f["true_energy"][where] = np.resize(BAD_ENERGIES, where.size)
    fam["bad_energy"] = dict(f, psets=PSETS_WIDE[:3] + PSETS_WIDE[5:], bad_rows=where)   # delta_index = 0: pow(NaN, 0) = 1
    return fam


_FAMILIES = None


def families():
    """{name: dict(true_energy, true_coszen, nu_flux_nominal, nubar_flux_nominal, psets, ...)}, N_FAMILY events
    each, seeded; built once and shared -- treat the arrays as read-only"""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _make_families()
        for f in _FAMILIES.values():
            for v in f.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
    return _FAMILIES


COLUMNS = ("true_energy", "true_coszen", "nu_flux_nominal", "nubar_flux_nominal")
_EXT = {}


def extended_of(name, ip, nubar):
    """`barr_extended` of family `name`, parameter set `ip`, computed once per process"""
    key = (name, ip, nubar)
    if key not in _EXT:
        f = families()[name]
        _EXT[key] = barr_extended(*(f[c] for c in COLUMNS), nubar, *f["psets"][ip])
    return _EXT[key]


def good_energy_families():
    """the families both kernel forms take: every energy positive and finite"""
    return ("wide", "clamp", "patterns")


# ------------------------------------------------------------- flux_2d: integral preservation
# The interpolation is called integral preserving because the interpolant's integral over every table bin
# (one data interval of log10 E x one coszen band) reproduces the table entry:
#     int int flux E^enpow dlog10E dcz = table * E^enpow * dlogE * dcz.
# flux * E^enpow is, inside a bin, a quadratic in log10 E (derivative of the band splines; a not-a-knot end only
# merges two data intervals into one polynomial) times a quadratic in coszen (derivative of the coszen spline):
# a 3 x 3 Gauss-Legendre rule integrates it exactly, so the quadrature's residual is rounding alone.  This is
# the one check of `flux_2d` that depends neither on scipy's coefficient preparation, nor on the oracle, nor on
# goldens made by the same algorithm.
#
# r_ref: the worst |quadrature - table entry's integral| / (band's total integral) of the fp64 CPU evaluation,
# over 4 primaries x 20 bands x every energy bin, measured with `python oracle/measure_flux_refs.py`:
#     Honda  (oracle/flux_oracle.py, 101 bins per band)                        8.9e-16, written 1.0e-15
#            (the reference's own calculate_2d_flux_weights gives the same 8.9e-16)
#     Bartol (the reference's calculate_2d_flux_weights, 70 bins per band)     1.04e-15
# The reference preserves the Bartol bins as well as the Honda ones, so both tables are tested.
# The kernel gets QUAD_FACTOR = 16 times that for its different summation order over 21 knots and 20 bands.
R_REF_HONDA = 1.0e-15
R_REF_BARTOL = 1.04e-15      # the one written figure no CPU test measures again: it takes the reference's own tree
QUAD_FACTOR = 16.0
HONDA = "flux/honda-2015-spl-solmin-aa.d"
BARTOL = "flux/bartol-2004-sno-solmax-aa.d"
TABLE_COLUMNS = ("numu", "numubar", "nue", "nuebar")       # column order of the table files
N_CZ = 20
_GL3 = np.polynomial.legendre.leggauss(3)


def read_table(path):
    """the raw table text with numpy only -> (energy[n_e], {primary: [20 bands ascending in coszen][n_e]})"""
    rows = []
    with open(path) as fh:
        for line in fh:
            try:
                vals = [float(x) for x in line.split()[:5]]
            except ValueError:
                continue                     # the two header lines of every band
            if len(vals) == 5:
                rows.append(vals)
    t = np.array(rows).reshape(N_CZ, -1, 5)  # file order: the band of coszen 0.95 first
    assert np.all(t[:, :, 0] == t[0, :, 0])
    return t[0, :, 0].copy(), {p: t[::-1, :, 1 + k].copy() for k, p in enumerate(TABLE_COLUMNS)}


def bin_edges(name, energy):
    """edges in log10 E of the table's energy bins (the knots of the band splines)"""
    if name == "honda":
        edges = np.linspace(-1.025, 4.025, 102)
    else:
        edges = np.concatenate([np.linspace(-1, 1, 41), np.linspace(1.1, 4, 30)])
    assert edges.size == energy.size + 1
    assert np.all((np.log10(energy) > edges[:-1]) & (np.log10(energy) < edges[1:]))
    return edges


def gauss_nodes(edges):
    """3 Gauss-Legendre nodes per interval -> (nodes[n_int * 3], weights[n_int * 3]) for the plain integral"""
    x, w = _GL3
    lo, hi = edges[:-1, None], edges[1:, None]
    return (0.5 * (lo + hi) + 0.5 * (hi - lo) * x).ravel(), (0.5 * (hi - lo) * w * np.ones_like(lo)).ravel()


def quadrature_points(name, energy):
    """-> dict(e[n_x], cz[n_c], wx[n_x], wc[n_c]): the kernel is evaluated on the n_x x n_c product grid"""
    x, wx = gauss_nodes(bin_edges(name, energy))
    c, wc = gauss_nodes(np.linspace(-1, 1, N_CZ + 1))
    return dict(e=10 ** x, cz=c, wx=wx, wc=wc)


def preservation_residual(name, energy, bands, pts, flux_grid, enpow=1):
    """flux_grid[n_x, n_c] of one primary at `quadrature_points` -> the worst over bins of
    |quadrature - table * E^enpow * dlogE * dcz| / (that band's total integral)"""
    edges = bin_edges(name, energy)
    integrand = flux_grid * (pts["e"] ** enpow)[:, None] * pts["wx"][:, None] * pts["wc"][None, :]
    quad = integrand.reshape(energy.size, 3, N_CZ, 3).sum(axis=(1, 3))              # [n_e, band]
    want = (bands * energy ** enpow * np.diff(edges)).T * (2.0 / N_CZ)              # [n_e, band]
    return float((np.abs(quad - want) / want.sum(axis=0)).max())


def barr_reference_ratios(oracle):
    """-> ({'oracle' | golden file: worst gate ratio}, smallest |d|): what G_REF is read off"""
    worst = {"oracle": 0.0}
    mind = np.inf
    for name, f in families().items():
        for ip, ps in enumerate(f["psets"]):
            for nubar in (1, -1):
                ext, m, d = extended_of(name, ip, nubar)
                mind = min(mind, float(np.nanmin(np.abs(d))))
                got = oracle.barr_simple(*(f[c] for c in COLUMNS), nubar, *ps)
                ok = ~np.isnan(got) & ~clamped(d, nubar)
                worst["oracle"] = max(worst["oracle"], float(gate_ratio(got, ext, m, d, f["true_energy"])[0][ok].max()))
    for gname in ("barr_ref.npz", "barr_wide_ref.npz"):
        g = np.load(os.path.join(GOLDEN, gname))
        w = 0.0
        for ip, ps in enumerate(g["params"]):
            for nubar, tag in ((1, "nu"), (-1, "nubar")):
                ext, m, d = barr_extended(*(g[c] for c in COLUMNS), nubar, *ps)
                got = g["out%d_%s" % (ip, tag)]
                ok = ~np.isnan(got) & ~clamped(d, nubar)
                w = max(w, float(gate_ratio(got, ext, m, d, g["true_energy"])[0][ok].max()))
        worst[gname] = w
    return worst, mind


def oracle_preservation_residual(path):
    """r_ref of the Honda table: the fp64 CPU oracle's worst residual over the four primaries"""
    from oracle import flux_oracle

    energy, bands = read_table(path)
    pts = quadrature_points("honda", energy)
    splines = flux_oracle.load_2d_honda_table(path)
    return max(preservation_residual("honda", energy, bands[p], pts,
                                     flux_oracle.grid_flux(pts["e"], pts["cz"], splines[p])) for p in TABLE_COLUMNS)
