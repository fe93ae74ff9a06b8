"""Shared pieces of the exact-value tests of the KDE (csrc/kde.hip): the seeded sample families, the exact values in
`np.longdouble`, the gate, and a numpy restatement of the estimator's cell-grid rule.  A plain helper module (no
fixtures); `tests/test_host_kde_cases.py` pins everything here without a GPU (the longdouble values against mpmath at
50 digits, G_REF, the regime each family is meant to reach), `tests/test_gpu_kde_exact.py` runs the kernels.

A density value is a pilot density at a source or a density at a query: a sum of terms a_i = coef_i exp(-e_i),
e_i = s2_i r_i^2 / 2 (r_i the whitened distance).  The gate, per value:

    |got - exact| <= G eps S + c_T tol sum_i coef_i + lambda sum_i a_i + U,        S = sum_i a_i (1 + e_i)

  - G eps S: rounding.  A term's relative error is that of exp (a couple of ulp) plus e_i times the relative error of
    its argument, hence the weight (1 + e_i).  G = metric_cases.KERNEL_FACTOR * max(1, G_REF[family]); G_REF is the
    worst ratio |value - exact| / (eps S) of the fp64 restatement of the same sums on the CPU (`fp64_estimator` below,
    which is oracle/kde_oracle.py's chain over `oracle.kde_eval`), measured by tests/test_host_kde_cases.py and
    written below.  It is never taken from the device.  It is kept PER FAMILY and per stage ("pilot": the whole chain
    from the raw sample; "eval": the sum over given arrays): `narrow` (correlation 0.999, mean 1e3) loses three digits
    in x - mean and two more in the whitening, in any fp64 implementation, and one constant over all families would
    carry that loss (G_REF 211) into the gate of every other family.  No family's gate is wider for it than with the
    single constant.
  - c_T tol sum coef: truncation, from the code's own statements.  c_T = 1 where every pair is summed and cells
    beyond the cut-off are skipped (pair-summed pilot, point evaluation, lattice); 5 = 1 + 4 for the series and
    local-expansion pilots (4 tol of a cell's weight per cell); 0 at tol = 0.  For the pair-summed forms the error is
    one-sided (dropped terms are positive): got <= exact + G eps S + U as well.
  - lambda = 3e-13 for the lattice recurrence, 0 elsewhere: the figure kde.hip states.  Derivation: the middle value's
    exponent reaches (r_cut + 25)^2 / 2 = 545 and is formed with three roundings (1.8e-13 of the value at half an ulp
    each), the ratio's exponent |s2 da xc| <= 52 is raised to the power <= 16 (9e-14), Q_k is a chain of <= 2 k
    products of h (4e-15): 2.8e-13 if all were at their worst at once.  A host replica of the kernel's instruction
    sequence (same fma, rint, ldexp) against long double over 3e6 random strips at the admission limit gave 2.1e-13
    (R = 32), 2.0e-13 (16), 2.1e-13 (8) -- the middle value's exponent dominates, so shorter strips gain little.
  - U = (n + sum coef) 2^-1074: below 2^-1022 an fp64 term is rounded to a multiple of 2^-1074 (or to zero), which no
    relative bound covers.  It matters only for queries hundreds of bandwidths away at tol = 0.

For s2 = lam^2 and coef = wn lam^d / norm (lam = (p / g)^alpha, g the geometric mean of the weighted pilots) the
allowance is the pilot's carried through:  |ds2_i| / s2_i <= 2 alpha (rho_i + rho_g) + G eps, rho_i the pilot's
allowance over p_i, rho_g the mean of rho_i over the weighted sources (exponent d instead of 2 for coef).  The last
term is the format's: the quotient, the power, the square and the products each round once.

G_REF as measured is the table G_REF below (tests/test_host_kde_cases.py measures again and holds every constant
within [1, 2] x its measurement).  The restatement sums d^T inv_cov d from raw coordinates, term by term: 5 to 37
eps S, against the 1 to 2 eps S a whitened sum reaches; `narrow` 211 and, for its pilot (not gated), 256.

Where this departs from the wording of the issue that asked for these tests (each argued above; the device's worst
ratios in tests/test_gpu_kde_exact.py show how much of each is used):  (1) U is added -- without it a query at
tol = 0 whose terms lie below 2^-1022 cannot be met by any fp64 code; it is 1e-320 and used nowhere else.
(2) `+ G eps` in the s2 / coef allowance: at most 3e-14 relative, the device uses < 1 % of the allowance either way.
(3) G_REF per family and stage instead of one worst ratio (211): tighter for every family but `narrow`, equal there.
"""
import numpy as np

from tests import metric_cases as mc

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TINY = 2.0 ** -1074
KERNEL_FACTOR = mc.KERNEL_FACTOR
LATTICE_LAMBDA = 3e-13
TOLS = (1e-10, 1e-12, 1e-13, 1e-14)
Q_CHUNK = 512               # csrc/kde_plan.hpp: queries per workgroup of the pilot
HERMITE_MIN_SERIES = 24     # csrc/kde_plan.hpp: a series evaluated per target pays from this many sources
EXPANSION_MIN_N = 1000      # csrc/kde_plan.hpp, expansion_min_n: no expansion below

# family: (pilot, eval) -- worst |fp64 restatement - exact| / (eps S); `None`: the stage is not gated for the family
G_REF = {
    "cloud999": (6.5, 5.7), "cloud1000": (6.4, 5.9), "cloud1500": (7.4, 7.2), "clumps": (15.0, 9.8),
    "capped_w100": (14.3, 14.5), "capped_w60": (9.5, 7.0), "capped_u200": (15.1, 12.5), "feather": (17.2, 36.9),
    "narrow": (None, 211.0), "dim1": (6.4, 7.2), "dim3": (5.4, 5.4),
    "kernel1": (None, 4.9), "kernel2": (None, 8.8), "kernel3": (None, 4.6),
}


def g_of(family, stage):
    ref = G_REF[family][0 if stage == "pilot" else 1]
    assert ref is not None, (family, stage)
    return KERNEL_FACTOR * max(1.0, ref)


# ------------------------------------------------------------------ families
def _cloud_xy(rs, dim, n):
    """the correlated non-Gaussian cloud of tests/test_gpu_kde.py (_estimator_vs_oracle): a coszen-like uniform
    dimension, a ln E-like skewed one"""
    x = np.empty((dim, n))
    x[0] = rs.rand(n) * 2 - 1
    if dim > 1:
        x[1] = 1.5 + rs.gamma(3.0, 0.6, n) + 0.4 * x[0]
    if dim > 2:
        x[2] = rs.randn(n) * 0.3 + 0.2 * x[1]
    return x


def _cloud(n, seed):
    rs = np.random.RandomState(seed)
    x = _cloud_xy(rs, 2, n)
    w = rs.rand(n) * 2 + 0.1
    return x, w, dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=1e-14)


def _capped(n, sigma, weight, tol, seed):
    """N(0,1)^2 and two points `sigma` away on the axes: they widen the bounding box (with weight 0 not even the
    covariance), the grid no longer fits cells_cap(n) at r_cut / 8 and the cells grow by factors of 1.25"""
    rs = np.random.RandomState(seed)
    x = rs.randn(2, n)
    w = np.ones(n)
    x[:, 0] = (sigma, 0.0)
    x[:, 1] = (0.0, sigma)
    w[:2] = weight
    return x, w, dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=tol)


def _whitening_fp64(x, w, bw):
    e = exact_moments(x, w, bw)
    return np.array(e["U"], dtype=float), np.array(e["mean"], dtype=float)


def _clumps():
    """n = 3000: 700 sources inside one cell (> Q_CHUNK: cut into equal parts), two clumps of 120 over a few cells
    each (some reach HERMITE_MIN_SERIES, some do not), 2060 sources of a thousandth of the weight spread so thin that
    most non-empty cells hold one.  Positions are in units of about two cells; the big clump is moved over a fixed list
    of offsets until it sits inside one cell of the grid of `grid_rule` (tol = 1e-14)."""
    rs = np.random.RandomState(41)
    n_thin = 3000 - 700 - 240
    thin = rs.rand(2, n_thin) * 40.0 - 20.0
    c1 = np.array([[6.0], [2.0]]) + 0.22 * rs.randn(2, 120)
    c2 = np.array([[-3.0], [7.0]]) + 0.22 * rs.randn(2, 120)
    big = (rs.rand(2, 700) - 0.5) * 0.3
    w = np.concatenate([rs.rand(940) + 0.5, 1e-3 * (rs.rand(n_thin) + 0.5)])
    kw = dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=1e-14)
    for oy in range(6):
        for ox in range(6):
            x = np.concatenate([big + np.array([[0.2 * ox], [0.2 * oy]]), c1, c2, thin], axis=1)
            g = grid_rule(x, w, "silverman", 1e-14)
            if np.bincount(g["cell_of"]).max() >= 700:
                return x, w, kw
    raise AssertionError("clumps: no offset puts the big clump inside one cell")


def _feather():
    """n = 1200: four heavy clumps on the corners of a square (they set the covariance: a clump is a twentieth of a
    bandwidth wide) and 40 sources whose weights are 1e-18 ... 1e-6 of the mean weight: 8 inside the first clump and 8
    each at 0.5, 0.9, 0.99 and 1.01 r_cut (tol = 1e-14) from its centre in whitened units, on the side away from the
    other clumps.  In exact arithmetic their pilots are positive: the clump's tail, tol-sized at r_cut, plus their
    own term."""
    rs = np.random.RandomState(43)
    heavy = np.concatenate([np.array([[sx], [sy]]) + 0.02 * rs.randn(2, 290) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)], axis=1)
    wh = rs.rand(1160) + 0.5
    U, _ = _whitening_fp64(np.concatenate([heavy, np.zeros((2, 40))], axis=1), np.concatenate([wh, np.zeros(40)]), "silverman")
    r_cut = np.sqrt(2.0 * np.log(1e14))
    centre = np.array([[-1.0], [-1.0]])
    pts = [centre + 0.02 * rs.randn(2, 8)]
    Uinv = np.linalg.inv(U)
    for f in (0.5, 0.9, 0.99, 1.01):
        ang = np.pi + (np.arange(8) + 0.5) / 8.0 * (np.pi / 2)
        pts.append(centre + Uinv @ (f * r_cut * np.stack([np.cos(ang), np.sin(ang)])))
    wf = wh.mean() * 10.0 ** np.linspace(-18.0, -6.0, 40)[rs.permutation(40)]
    x = np.concatenate([heavy] + pts, axis=1)
    w = np.concatenate([wh, wf])
    return x, w, dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=1e-14)


def _narrow():
    rs = np.random.RandomState(44)
    z = rs.randn(2, 1200)
    rho = 0.999
    x = np.stack([z[0], rho * z[0] + np.sqrt(1 - rho * rho) * z[1]]) + 1e3
    w = rs.rand(1200) + 0.2
    return x, w, dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=1e-14)


def _dims(dim):
    rs = np.random.RandomState(45 + dim)
    n = 800 if dim == 1 else 900
    x = _cloud_xy(rs, dim, n)
    w = rs.rand(n) * 2 + 0.1
    return x, w, dict(bw_method="silverman", adaptive=True, alpha=0.3, tol=1e-14)


def _kernel(dim):
    """the shapes of tests/test_gpu_kde.py::test_kde_kernel_vs_oracle: raw arrays for `kde_eval` (all pairs)"""
    rs = np.random.RandomState(1)
    for d, n, m in ((1, 300, 257), (2, 1500, 1030), (3, 700, 300)):
        src, qry = rs.randn(d, n), rs.randn(d, m) * 1.5
        coef, s2 = rs.rand(n), 0.5 + rs.rand(n)
        a = rs.randn(d, d)
        inv_cov = a @ a.T + np.eye(d)
        if d == dim:
            return src, coef, s2, qry, inv_cov


_BUILDERS = {
    # (seed 26: at n = 1500 a cell reaches HERMITE_MIN_SERIES at each of TOLS, so the series per target has work at every order)
    "cloud999": lambda: _cloud(999, 26), "cloud1000": lambda: _cloud(1000, 26), "cloud1500": lambda: _cloud(1500, 26),
    "clumps": _clumps,
    "capped_w100": lambda: _capped(4000, 100.0, 0.0, 1e-14, 31),      # two WEIGHTLESS points at 100 sigma: cell 3.83
    "capped_w60": lambda: _capped(1500, 60.0, 0.0, 1e-12, 32),        # weightless, 60 sigma, tol 1e-12: cell 2.84
    "capped_u200": lambda: _capped(2000, 200.0, 1.0, 1e-14, 33),      # unit weight, 200 sigma: cell 1.96
    "feather": _feather, "narrow": _narrow, "dim1": lambda: _dims(1), "dim3": lambda: _dims(3),
}
SAMPLE_FAMILIES = tuple(_BUILDERS)
CAPPED = {"capped_w100": 3.83, "capped_w60": 2.84, "capped_u200": 1.96}      # the cells of the issue's table
KERNEL_FAMILIES = ("kernel1", "kernel2", "kernel3")
_FAM = {}


def family(name):
    """(x [d, n], w, kwargs) -- cached, do not modify"""
    if name not in _FAM:
        x, w, kw = _BUILDERS[name]()
        x.setflags(write=False)
        w.setflags(write=False)
        _FAM[name] = (x, w, kw)
    x, w, kw = _FAM[name]
    return x, w, dict(kw)


def kernel_family(name):
    return _kernel(int(name[-1]))


def queries(name, m=700, seed=3):
    """m query points of a sample family: inside the cloud, 30 % outside its bounding box, 16 exactly on sources and 8
    a million spans of the sample away: every kernel value is below fp64's range (`feather`'s widest kernels
    are 3e4 bandwidths wide) and beyond every cut-off, the expected value is 0"""
    x, _, _ = family(name)
    d, n = x.shape
    rs = np.random.RandomState(1000 + seed + m)
    lo, hi = np.percentile(x, 1, axis=1)[:, None], np.percentile(x, 99, axis=1)[:, None]
    q = lo + (hi - lo) * rs.rand(d, m)
    n_out = int(0.3 * m)
    side = rs.randint(0, 2, (d, n_out)) * 2 - 1
    q[:, :n_out] = np.where(side > 0, hi + (hi - lo) * 0.4 * rs.rand(d, n_out), lo - (hi - lo) * 0.4 * rs.rand(d, n_out))
    far = np.zeros(m, dtype=bool)
    if m >= 100:
        q[:, n_out:n_out + 16] = x[:, rs.choice(n, 16, replace=False)]
        span = (x.max(axis=1) - x.min(axis=1))[:, None]
        q[:, n_out + 16:n_out + 24] = x.mean(axis=1)[:, None] + span * 1e6 * (rs.rand(d, 8) + 1.0) * (rs.randint(0, 2, (d, 8)) * 2 - 1)
        far[n_out + 16:n_out + 24] = True
    return q, far


# ------------------------------------------------------------------ exact values (np.longdouble)
def _ld(a):
    return np.asarray(a, dtype=LD)


def _inverse(H):
    """(inverse, determinant) of a symmetric d x d matrix, d <= 3, by cofactors"""
    d = H.shape[0]
    P = np.eye(3, dtype=LD)
    P[:d, :d] = H
    det = (P[0, 0] * (P[1, 1] * P[2, 2] - P[1, 2] * P[2, 1]) - P[0, 1] * (P[1, 0] * P[2, 2] - P[1, 2] * P[2, 0]) +
           P[0, 2] * (P[1, 0] * P[2, 1] - P[1, 1] * P[2, 0]))
    inv = np.empty((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            minor = P[r[0], c[0]] * P[r[1], c[1]] - P[r[0], c[1]] * P[r[1], c[0]]
            inv[i, j] = (-1) ** (i + j) * minor / det
    return inv[:d, :d], det


def whitening(inv_cov):
    """U (upper triangular, longdouble) with |U v|^2 = v^T inv_cov v: inv_cov = L L^T, U = L^T"""
    inv = _ld(inv_cov)
    d = inv.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for i in range(d):
        for j in range(i + 1):
            s = inv[i, j] - np.sum(L[i, :j] * L[j, :j])
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L.T.copy()


def whiten(x, inv_cov, mean):
    return whitening(inv_cov) @ (_ld(x) - _ld(mean)[:, None])


def exact_moments(x, w, bw):
    x = _ld(x)
    d, n = x.shape
    wn = np.full(n, LD(1) / n) if w is None else _ld(w) / np.sum(_ld(w))
    base = LD(n) * (d + 2) / 4 if bw == "silverman" else LD(n)
    factor = base ** (-LD(1) / (d + 4))
    mean = np.sum(x * wn, axis=1)
    xc = x - mean[:, None]
    cov = (xc * wn) @ xc.T / (1 - np.sum(wn * wn)) * factor * factor
    inv_cov, det = _inverse(cov)
    norm = np.sqrt((2 * np.arccos(LD(-1))) ** d * det)
    return dict(wn=wn, factor=factor, mean=mean, cov=cov, inv_cov=inv_cov, norm=norm, U=whitening(inv_cov))


def exact_density(ys, coef, s2, yq, chunk=500):
    """sum_i coef_i exp(-s2_i |yq - ys_i|^2 / 2) over the GIVEN arrays (whitened coordinates), every pair, in
    longdouble; returns (value, S = sum a (1 + e)), each [m]"""
    ys, coef, s2, yq = _ld(ys), _ld(coef), _ld(s2), _ld(yq)
    m = yq.shape[1]
    val, S = np.empty(m, dtype=LD), np.empty(m, dtype=LD)
    for c in range(0, m, chunk):
        diff = yq[:, c:c + chunk, None] - ys[:, None, :]
        e = np.sum(diff * diff, axis=0) * (s2[None, :] / 2)
        a = coef[None, :] * np.exp(-e)
        val[c:c + chunk] = np.sum(a, axis=1)
        S[c:c + chunk] = np.sum(a * (1 + e), axis=1)
    return val, S


def exact_quadratic(src, coef, s2, qry, inv_cov):
    """the same sums from raw coordinates and the inverse bandwidth matrix (`kde_eval`'s arguments)"""
    U = whitening(inv_cov)
    return exact_density(U @ _ld(src), coef, s2, U @ _ld(qry))


def exact_estimator(x, w, bw, adaptive, alpha):
    """every number of the estimator, all pairs, no cut-off: mean, cov, factor, inv_cov, norm, ys (whitened sources),
    pilot, pilot_S, glob (geometric mean of the pilots over w > 0: the choice oracle/kde_oracle.py documents; in exact
    arithmetic every weighted pilot is positive), lam, coef, s2"""
    e = exact_moments(x, w, bw)
    d, n = np.shape(x)
    ys = e["U"] @ (_ld(x) - e["mean"][:, None])
    ones = np.ones(n, dtype=LD)
    e["ys"] = ys
    if adaptive:
        pilot, S = exact_density(ys, e["wn"] / e["norm"], ones, ys)
        pos = e["wn"] > 0
        assert np.all(pilot[pos] > 0)
        glob = np.exp(np.mean(np.log(pilot[pos])))
        lam = np.where(pos, (np.where(pos, pilot, 1) / glob) ** LD(alpha), LD(1))
        e.update(pilot=pilot, pilot_S=S, glob=glob)
    else:
        lam = ones
    e.update(lam=lam, s2=lam * lam, coef=e["wn"] * lam ** d / e["norm"])
    return e


_EXACT = {}
_PILOT_KEYS = ("pilot", "pilot_S", "glob", "lam", "coef", "s2")


def exact_case(name, bw=None, adaptive=None, alpha=None):
    """`exact_estimator` of a family (its own settings unless given), cached.  Where the family's pilot is not gated
    (G_REF pilot None: `narrow`, whose x - mean and whitening lose five digits even in longdouble) the pilot-derived
    numbers are NOT exact to 0.01 eps S and are not handed out."""
    x, w, kw = family(name)
    key = (name, bw or kw["bw_method"], kw["adaptive"] if adaptive is None else adaptive, kw["alpha"] if alpha is None else alpha)
    if key not in _EXACT:
        e = exact_estimator(x, w, key[1], key[2], key[3])
        if G_REF[name][0] is None:
            for k in _PILOT_KEYS:
                e.pop(k, None)
        _EXACT[key] = e
    return _EXACT[key]


# ------------------------------------------------------------------ the fp64 restatement (G_REF's subject)
def fp64_estimator(orc, x, w, bw, adaptive, alpha):
    """oracle/kde_oracle.py `gaussian_kde_eval`, line by line, returning the intermediate numbers as well"""
    d, n = x.shape
    w = np.full(n, 1.0 / n) if w is None else np.asarray(w, dtype=float) / np.sum(w)
    factor = (n * (d + 2) / 4.0) ** (-1.0 / (d + 4)) if bw == "silverman" else n ** (-1.0 / (d + 4))
    mean = (x * w).sum(axis=1, keepdims=True)
    xc = x - mean
    cov = (xc * w) @ xc.T / (1.0 - np.sum(w * w))
    covh = cov * factor ** 2
    inv_cov = np.linalg.inv(covh)
    norm = np.sqrt(np.linalg.det(2 * np.pi * covh))
    ones = np.ones(n)
    out = dict(inv_cov=inv_cov, norm=norm, mean=mean[:, 0])
    if adaptive:
        pilot = orc.kde_eval(x, w / norm, ones, x, inv_cov)
        pos = (w > 0) & (pilot > 0)
        glob = np.exp(np.mean(np.log(pilot[pos])))
        s = np.where(pos, (np.where(pos, pilot, 1.0) / glob) ** alpha, 1.0)
        out["pilot"] = pilot
    else:
        s = ones
    out.update(s2=s * s, coef=w * s ** d / norm)
    return out


# ------------------------------------------------------------------ the gate
def allowance(val, S, sum_coef, n, g, c_t=0.0, tol=0.0, lam=0.0):
    """the gate's right-hand side for the exact values `val` (= sum a) with their S"""
    return g * EPS * _ld(S) + c_t * tol * LD(sum_coef) + lam * _ld(val) + (n + LD(sum_coef)) * TINY


def gate_ratio(got, exact, allow):
    """worst |got - exact| / allowance (0 / 0 counts as 0)"""
    diff = np.abs(_ld(got) - exact)
    assert np.all(np.isfinite(np.asarray(got, dtype=float)))
    return float(np.max(np.where(diff == 0, LD(0), diff / allow)))


def one_sided_ratio(got, exact, S, sum_coef, n, g):
    """(got - exact) / (G eps S + U): at most 1 where only positive terms can have been dropped"""
    return float(np.max((_ld(got) - exact) / (g * EPS * _ld(S) + (n + LD(sum_coef)) * TINY)))


def pilot_allowances(ex, g, c_t, tol, alpha, dim):
    """relative allowances (s2, coef) per source, from the exact estimator `ex` (in ITS source order), and rho"""
    n = ex["pilot"].shape[0]
    allow = allowance(ex["pilot"], ex["pilot_S"], 1 / ex["norm"], n, g, c_t, tol)
    rho = allow / ex["pilot"]
    pos = ex["wn"] > 0
    rho_g = np.mean(rho[pos])
    both = np.where(pos, rho + rho_g, 0)
    return 2 * alpha * both + g * EPS, dim * alpha * both + g * EPS, rho


def match_sources(est_ys, inv_cov, mean, x):
    """index into the input sample of each source of the estimator's cell-sorted arrays, through the whitened
    coordinates: a bijection, every distance below 1e-9"""
    from scipy.spatial import cKDTree

    y = np.array(whiten(x, inv_cov, mean), dtype=float)
    dist, idx = cKDTree(y.T).query(np.asarray(est_ys, dtype=float).T)
    assert dist.max() < 1e-9, dist.max()
    assert np.array_equal(np.sort(idx), np.arange(y.shape[1]))
    return idx


# ------------------------------------------------------------------ the cell grid of pisa_hip_kde_create, restated
# (`cell_grid` and `series_order` of csrc/kde_plan.hpp; tests/test_host_kde_plan.py holds the two together on the CPU)
def series_bound(cell, order):
    """`series_order` (csrc/kde_plan.hpp): 2.3 K^2 (cell / 2)^P / sqrt(P!) of a cell's weight, K = 1.09"""
    bound, fact = 2.3 * 1.09 * 1.09, 1.0
    for i in range(1, order + 1):
        bound *= 0.5 * cell
        fact *= float(i)
    return bound / np.sqrt(fact)


def grid_rule(x, w, bw, tol):
    """cell size, grid shape, series order (0: no order up to 20 meets 4 tol -- no expansion), the order the code
    took before it checked 20's bound (`order_unchecked`), and each source's cell, for a 2-D or 1-D / 3-D sample"""
    x = np.asarray(x, dtype=float)
    d, n = x.shape
    U, mean = _whitening_fp64(x, w, bw)
    lo, hi = np.full(d, np.inf), np.full(d, -np.inf)
    for corner in range(1 << d):
        xc = np.array([(x[k].max() if (corner >> k) & 1 else x[k].min()) - mean[k] for k in range(d)])
        a = np.array([np.sum(U[k, k:] * xc[k:]) for k in range(d)])
        lo, hi = np.minimum(lo, a), np.maximum(hi, a)
    r_cut = np.sqrt(2.0 * np.log(1.0 / tol))
    cell = r_cut / (4.0 if d == 3 else 8.0)
    cap = min(1 << 22, max(4096, 4 * n))
    while True:
        counts = np.floor((hi - lo) / cell) + 1.0
        if np.all(counts < (1 << 16)) and np.prod(counts) <= cap:
            break
        cell *= 1.25
    order = next((p for p in (14, 16, 18, 20) if series_bound(cell, p) <= 4.0 * tol), 0)
    unchecked = next((p for p in (14, 16, 18) if series_bound(cell, p) <= 4.0 * tol), 20)
    y = U @ (x - mean[:, None])
    idx = np.minimum(np.floor((y - lo[:, None]) / cell).astype(np.int64), counts.astype(np.int64)[:, None] - 1)
    flat = idx[0]
    stride = 1
    for k in range(1, d):
        stride *= int(counts[k - 1])
        flat = flat + idx[k] * stride
    return dict(cell=cell, r_cut=r_cut, counts=counts.astype(int), order=order, order_unchecked=unchecked, cell_of=flat,
                bound20=series_bound(cell, 20))


# ------------------------------------------------------------------ the lattice kernel's launch shape, restated
def lattice_strip(da_s, tol):
    """strip length of `lattice_strip` (csrc/kde_plan.hpp) for da_s = da sqrt(max s2): the largest R of 32, 16, 8 with
    R da_s <= 50, else 0 (the points are written out and evaluated one by one)"""
    if not tol > 0:
        return 0
    return next((r for r in (32, 16, 8) if r <= 50.0 / da_s), 0)


def lattice_shape(n, tol, u00, u11, step, count, R):
    """(sw, LG) of `lattice_shape` (csrc/kde_plan.hpp): the lane-group width moves from 8 to 16, 32, 64 while the lattice has
    more than 4096 sub-patches of LG strips"""
    r_cut = np.sqrt(2.0 * np.log(1.0 / tol))
    strips_a = (count[0] + R - 1) // R
    rp, rl = r_cut / abs(u00 * step[0]), r_cut / abs(u11 * step[1])
    n0, n1 = float(count[0]), float(count[1])
    for lg in (8, 16, 32, 64):
        best, best_cost = 1, np.inf
        sw = 1
        while sw <= lg:
            if not (sw > 1 and sw // 2 >= strips_a):
                lpw = lg // sw
                j = np.arange(0, count[1], lpw)
                rows = np.sum(np.minimum(1.0, (2.0 * rl + np.minimum(lpw, count[1] - j)) / (n1 + 2.0 * rl)))
                i = np.arange(0, count[0], sw * R)
                cols = np.sum(np.minimum(1.0, (2.0 * rp + np.minimum(sw * R, count[0] - i)) / (n0 + 2.0 * rp)))
                cost = rows * cols
                if cost < best_cost * (1.0 - 1e-9):
                    best_cost, best = cost, sw
            sw *= 2
        lpw = lg // best
        patches = ((strips_a + best - 1) // best) * ((count[1] + lpw - 1) // lpw)
        cap = min(4096, max(1, (64 << 20) // (n // 64 + 1)))
        if patches <= cap or lg == 64:
            return best, lg, patches
