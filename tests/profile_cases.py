"""Shared pieces of the tests of the profiled trial ensembles (csrc/profile_device.hpp, csrc/profile.hip:
`pisa_hip_profiled_metric_matrix`, `pisa_hip_profiled_metric_matrix_best`) and of the `response=` paths of
pisa_amd/analysis/ensemble.py: the numpy fp64 restatement of the solver and of the reported value, the exact reference,
the seeded case families, the gate and a numpy batch evaluator.  A plain helper module (no fixtures);
`tests/test_host_profiled.py` pins everything here without a GPU, `tests/test_gpu_profiled.py` runs the kernels.

The definition ("Profiled trial ensembles").  For data row t, template row k, eta in R^J:

    mu_b(eta) = E[k,b] + R[k,0,b] eta_0 + ... + R[k,J-1,b] eta_{J-1}                 (ascending j, every product rounded)
    Phi(eta)  = sum_b phi(d_b, mu_b, s2_b) + w sum_j (ips_j (eta_j + c[k,j]))^2

phi = mu - d ln mu, w = 1/2 (llh, poisson_llh); phi = (d - mu)^2 / (s2 + mu), w = 1 (chi2: s2 = 0; mod_chi2).  `solve` is
the device's damped Newton iteration step for step (`pf_bin`, `pf_decide`, `pf_factor`, `pf_solve`), every pair of a
call advanced together under masks: all sums over bins are sequential chains in ascending order (`np.cumsum` along the
last axis is one), Phi's is compensated (`two_sum`).  `value` is the reported entry: the direct form of
tests/ensemble_cases.py on the pair's own template row mu(eta_hat), then the prior terms joined in ascending j through
`two_sum` and the pair rounded once more.

The exact reference (`exact`) is the same Newton iteration in np.longdouble (eps 1.1e-19), accepted steps judged at
longdouble's own rounding floor and run until the squared decrement is <= 1e-30 of the scale of Phi; its value comes
from the four formulae in longdouble as `ensemble_cases.exact_longdouble` forms them, lgamma(d + 1) from a running sum
of ln i for integer data and from mpmath (40 digits) otherwise.  The per-bin (hi, lo) tables of oracle/exact_metric.py
do not apply: mu(eta_hat) is a different number in every bin of every pair.

The gate, per entry:

    |got - exact| <= G eps S,
    S = sum over kept bins of ( m_b + 1 + |phi'(mu_b)| (|E_b| + sum_j |R_jb eta_j|) ) + w sum_j (ips_j (eta_j + c_j))^2

m_b as in tests/ensemble_cases.py (an llh bin without data is dropped); the |phi'| term because mu itself is a rounded
sum of J + 1 terms.  G = metric_cases.KERNEL_FACTOR * max(1, G_REF[kind]); G_REF is the worst ratio of `solve` +
`value` against the exact reference over every gated family and shape below, measured by tests/test_host_profiled.py
and held against these figures, never taken from the device.  Measured (numpy 2.2, scipy 1.15): 0.766 (llh), 0.975
(poisson_llh), 0.966 (chi2), 0.923 (mod_chi2), so G = 4 for every kind; at most 11 Newton steps on any gated pair.

The stopping rule.  Stopping at a squared decrement of eps / 2 * sum_b (|phi_b| + 1) (the first rule tried) left eta
within sqrt(eps) of the minimum.  Phi cannot see that, but the reported llh can: np.nansum drops the -mu of a bin
without data, so the value is not stationary at eta_hat and the error of eta enters it in first order -- ratios up
to 1700 on `poisson` at 3 bins.  And a chi2 step at 1e6 counts was refused for ever, because Phi itself is only
good to |phi'| times the rounding of mu.  The rule as it stands: the floor is eps / 2 * sum_b (|phi_b| + 1 + |phi'_b|
(|E_b| + sum_j |R_jb eta_j|)) + the prior terms; a trial point is accepted if Phi does not rise by more than the
floor, or unseen if the step's squared decrement is below the floor; the iteration stops at a squared decrement of
2^-20 of the floor and still applies the step formed there.

Gated families (`family(name, T, K, B, J)`; pseudo-data drawn at eta_0 ~ N(0, 0.5); every pair has status 0 in the exact
reference, which the host test asserts -- no pair is left out of a gated comparison):
    poisson  levels 5, 50, 5e3 and 1e6 per bin, responses 10 % cosine shapes of E, unit priors (so that J > B is fitted)
    norm     J = 1, R = E, no prior: eta_hat = sum d / sum E - 1 for the llh kinds
    asimov   D = mu(eta_0), no priors: eta_hat = eta_0 on the pair's own template and the value is near 0
    prior    ips alternating 0 / 1 with non-zero c, and the last parameter with R = 0 and a prior: eta_hat = -c
    far      D = 3 E, R = E: a long way from the start
    low      D = E / 4, R = E: the full Newton step of the llh kinds leaves the domain and must be damped
    shared   the [J, B] response shared by all templates
Status families (`status_family(name)`, flags compared with `==` against `solve`): `posdef` (J = 3 > B = 2, no priors),
`boundary` (all-zero data rows under llh with a weak prior: the minimum lies beyond mu = 0), `start` (a responding bin
with E = 1e-11), `maxiter` (`far` with max_iter = 1).
"""
import numpy as np

from tests import ensemble_cases as ec
from tests import metric_cases as mc

EPS = mc.EPS
SMALL_POS = mc.SMALL_POS
KINDS = mc.FUSED_KINDS
LLH_KINDS = ec.LLH_KINDS
G_HOST = mc.G_HOST
MAX_PARAMS = 8
NOT_CONVERGED, BOUNDARY, NOT_POSDEF, START_OUTSIDE = 1, 2, 4, 8
PIVOT_REL = 1e-13
MAX_HALVINGS = 40
STOP_REL = 2.0 ** -20          # PF_STOP_REL: the squared decrement the iteration stops at, as a share of Phi's floor
MAX_ITER = 32

# worst ratio of the fp64 restatement against the exact reference (module docstring; tests/test_host_profiled.py)
G_REF = {"llh": 0.77, "poisson_llh": 0.98, "chi2": 0.97, "mod_chi2": 0.93}

GATED = ("poisson", "norm", "asimov", "prior", "far", "low", "shared")
STATUS_FAMILIES = ("posdef", "boundary", "start", "maxiter")
# (T, K, B, J): every T of {1, 63, 64, 65, 257}, K of {1, 3, 17}, B of {1, 3, 64, 65, 130} and J of {1, 2, 5, 8}
SHAPES = ((1, 1, 1, 1), (65, 1, 3, 1), (63, 17, 65, 1), (63, 3, 3, 2), (1, 17, 130, 2), (257, 3, 64, 2),
          (64, 17, 64, 5), (64, 1, 130, 5), (65, 3, 65, 8), (257, 1, 130, 8))
PRIOR_ONLY_SHAPES = ((63, 3, 1, 5), (64, 3, 3, 8))          # J > B: fitted only where every parameter has a prior
STRIP_SHAPE = (1000, 5, 8, 2)                              # more strips of trials than one pass of the workgroups
TILE_SHAPE = (64, 300, 12, 3)                              # many templates per strip (the reduced output)


def g_of(kind):
    return mc.KERNEL_FACTOR * max(1.0, G_REF[kind])


def w_of(kind):
    return 0.5 if kind in LLH_KINDS else 1.0


def shapes_of(name):
    """the shapes a gated family runs on: J = 1 for the one-parameter families, J <= B without priors on every
    parameter, J >= 2 and at most B parameters without a prior for `prior`"""
    every = SHAPES + (STRIP_SHAPE, TILE_SHAPE)
    if name in ("norm", "far", "low"):
        return tuple(s for s in every if s[3] == 1)
    if name == "asimov":
        # (without any prior the few bins of the two large shapes leave pairs whose minimum lies on the domain's edge)
        return tuple(s for s in SHAPES if s[3] <= s[2])
    if name == "prior":
        return tuple(s for s in every if s[3] >= 2 and (s[3] + 1) // 2 <= s[2])
    return every + PRIOR_ONLY_SHAPES


# ------------------------------------------------------------------------------------- case families
LEVELS = (5.0, 50.0, 5e3, 1e6)
_FAM = {}


def _templates(rs, K, B, levels=LEVELS, integer=False):
    lev = np.array(levels)[np.arange(B) % len(levels)] * (0.8 + 0.4 * rs.rand(B))
    # the templates of a family lie within half a standard deviation per bin of each other: every pair is a fit a
    # trial ensemble would make, and ends inside the domain
    e = lev[None, :] * (1.0 + 0.5 / np.sqrt(lev)[None, :] * np.sin(np.arange(K)[:, None] + 0.1 * np.arange(B)[None, :]))
    return 4.0 * np.rint(e / 4.0 + 0.5) if integer else e


def _cosines(K, J, B):
    b = (np.arange(B) + 0.5) / B
    return np.cos((np.arange(J)[None, :, None] + 1) * np.pi * b[None, None, :] + 0.3 * np.arange(K)[:, None, None])


def _mu(E, R, eta):
    """[T, K, B]: mu(eta) of every pair in the stated order; E [K, B], R [K, J, B] or [J, B], eta [T, K, J]"""
    R = R if R.ndim == 3 else R[None]
    mu = np.broadcast_to(E[None], eta.shape[:2] + E.shape[1:]).astype(eta.dtype)
    for j in range(R.shape[1]):
        mu = mu + R[None, :, j, :].astype(eta.dtype) * eta[:, :, j, None]
    return mu


def family(name, T, K, B, J):
    """dict(D [T, B], E [K, B], S2 [K, B], R [K, J, B] or [J, B], ips [J] or None, c [K, J] or None, eta0 [T, J]):
    seeded, built once, read-only"""
    key = (name, T, K, B, J)
    if key in _FAM:
        return _FAM[key]
    rs = ec._rs("profile", name, T, K, B, J)
    own = np.arange(T) % K                       # the template a data row is drawn from
    eta0 = 0.5 * rs.randn(T, J)
    ips = c = None
    if name in ("poisson", "shared", "asimov", "prior"):
        E = _templates(rs, K, B)
        if name == "shared":
            R = 0.1 * _cosines(1, J, B)[0] * E.mean(axis=0)[None, :]
            ips = np.full(J, 0.5)
        else:
            R = 0.1 * _cosines(K, J, B) * E[:, None, :]
        if name == "poisson":
            ips = np.ones(J)
        if name == "prior":
            ips = (np.arange(J) % 2).astype(np.float64)
            ips[J - 1] = 1.0
            R[:, J - 1, :] = 0.0
            c = 0.3 * np.sin(1.0 + np.arange(K)[:, None] + np.arange(J)[None, :])
        full = R if R.ndim == 3 else np.broadcast_to(R[None], (K,) + R.shape)
        mu0 = E[own] + np.einsum("tjb,tj->tb", full[own], eta0)
        mu0 = np.maximum(mu0, 0.05 * E[own])
        D = mu0 if name == "asimov" else rs.poisson(mu0).astype(np.float64)
    elif name == "norm":
        assert J == 1
        E = _templates(rs, K, B, levels=(50.0, 5e3))
        R = E[:, None, :].copy()
        eta0 = np.maximum(eta0, -0.5)
        D = rs.poisson(E[own] * (1.0 + eta0)).astype(np.float64)
    elif name in ("far", "low"):
        assert J == 1
        E = _templates(rs, K, B, integer=True)    # multiples of 4: 3 E and E / 4 are counts
        R = E[:, None, :].copy()
        D = 3.0 * E[own] if name == "far" else E[own] / 4.0
    else:
        raise KeyError(name)
    f = dict(D=D, E=E, S2=np.abs(0.3 * E * rs.randn(K, B)), R=R, ips=ips, c=c, eta0=eta0)
    for v in f.values():
        if v is not None:
            v.setflags(write=False)
    _FAM[key] = f
    return f


def status_family(name):
    """dict(kind, D, E, S2, R, ips, c, max_iter): small cases whose pairs end flagged (module docstring)"""
    rs = ec._rs("profile-status", name)
    if name == "posdef":
        T, K, B, J = 5, 2, 2, 3
        E = 40.0 + 20.0 * rs.rand(K, B)
        return dict(kind="chi2", D=rs.poisson(E[np.arange(T) % K]).astype(np.float64), E=E, S2=0.1 * E,
                    R=0.1 * E[:, None, :] * (1.0 + rs.rand(K, J, B)), ips=None, c=None, max_iter=MAX_ITER)
    if name == "boundary":
        T, K, B, J = 6, 2, 5, 1
        E = 40.0 + 20.0 * rs.rand(K, B)
        D = rs.poisson(E[np.arange(T) % K]).astype(np.float64)
        D[::2] = 0.0                             # the rows without data: Phi = sum mu + prior
        return dict(kind="llh", D=D, E=E, S2=0.1 * E, R=E[:, None, :].copy(), ips=np.array([0.01]), c=None,
                    max_iter=MAX_ITER)
    if name == "start":
        T, K, B, J = 4, 3, 6, 2
        E = 40.0 + 20.0 * rs.rand(K, B)
        E[1, 2] = 1e-11                          # template 1 starts outside the domain
        R = 0.1 * _cosines(K, J, B) * 50.0
        return dict(kind="poisson_llh", D=rs.poisson(np.maximum(E[np.arange(T) % K], 1.0)).astype(np.float64), E=E,
                    S2=0.1 * E, R=R, ips=np.ones(J), c=None, max_iter=MAX_ITER)
    if name == "maxiter":
        f = family("far", 65, 1, 3, 1)
        return dict(kind="mod_chi2", D=f["D"], E=f["E"], S2=f["S2"], R=f["R"], ips=None, c=None, max_iter=1)
    raise KeyError(name)


# ------------------------------------------------------------------------------- the solver, any precision
def two_sum(s, c, x):
    t = s + x
    bb = t - s
    return t, c + ((s - (t - bb)) + (x - bb))


def _chain(x):
    """sum over the last axis as ONE sequential chain in ascending order, from 0"""
    return np.cumsum(x, axis=-1)[..., -1]


def _sweep(kind, D, E, S2, R, eta_t):
    """`pf_bin` over all bins of all pairs at eta_t [T, K, J] -> inside, phi (s, c), scale, g [T, K, J], H {(i, j)}"""
    dt = eta_t.dtype
    J = R.shape[1]
    live = (np.isfinite(D)[:, None, :] & np.isfinite(E)[None, :, :])
    mu = _mu(E, R, eta_t)
    responds = (R != 0).any(axis=1)[None]
    inside = ~(live & responds & ~(mu >= SMALL_POS)).any(axis=2)
    with np.errstate(all="ignore"):
        m = np.where(mu < SMALL_POS, dt.type(SMALL_POS), mu)
        d = D[:, None, :].astype(dt)
        if kind in LLH_KINDS:
            q = d / m
            phi, p1, p2 = m - d * np.log(m), 1.0 - q, q / m
        else:
            s2 = S2[None].astype(dt) if kind == "mod_chi2" else None
            v = s2 + m if kind == "mod_chi2" else m
            rr = d - m
            a = rr / v
            u = ((d + s2) if kind == "mod_chi2" else d) / v
            phi, p1, p2 = rr * a, -(a * (2.0 + a)), 2.0 * (u * u) / v
        zero = dt.type(0)
        phi, p1, p2 = np.where(live, phi, zero), np.where(live, p1, zero), np.where(live, p2, zero)
        s = np.zeros(mu.shape[:2], dtype=dt)
        c = np.zeros_like(s)
        for b in range(mu.shape[2]):
            s, c = two_sum(s, c, phi[:, :, b])
        reach = np.abs(E)[None].astype(dt)
        for j in range(J):
            reach = reach + np.abs(R[None, :, j, :].astype(dt) * eta_t[:, :, j, None])
        scale = _chain(np.where(live, (np.abs(phi) + 1.0) + np.abs(p1) * reach, zero))
        g = np.empty(mu.shape[:2] + (J,), dtype=dt)
        H = {}
        Rb = R[None].astype(dt)
        for i in range(J):
            g[:, :, i] = _chain(p1 * Rb[:, :, i])
            hi = p2 * Rb[:, :, i]
            for j in range(i + 1):
                H[(i, j)] = _chain(hi * Rb[:, :, j])
    return inside, s, c, scale, g, H


def _factor(H, J):
    """`pf_factor`: H -> L in place -> the pairs whose factorisation fails"""
    fail = np.zeros(H[(0, 0)].shape, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(J):
            diag = H[(k, k)]
            piv = diag
            for m in range(k):
                piv = piv - H[(k, m)] * H[(k, m)]
            fail |= ~(piv > PIVOT_REL * diag) | ~(piv > 0.0) | np.isinf(piv)
            lkk = np.sqrt(piv)
            H[(k, k)] = lkk
            for i in range(k + 1, J):
                v = H[(i, k)]
                for m in range(k):
                    v = v - H[(i, m)] * H[(k, m)]
                H[(i, k)] = v / lkk
    return fail


def _solve(L, g, J):
    """`pf_solve` -> (step [T, K, J], lam2)"""
    z = [None] * J
    lam2 = np.zeros(g.shape[:2], dtype=g.dtype)
    with np.errstate(all="ignore"):
        for i in range(J):
            v = g[:, :, i]
            for m in range(i):
                v = v - L[(i, m)] * z[m]
            z[i] = v / L[(i, i)]
            lam2 = lam2 + z[i] * z[i]
        step = np.empty_like(g)
        for i in range(J - 1, -1, -1):
            v = z[i]
            for m in range(i + 1, J):
                v = v - L[(m, i)] * z[m]
            z[i] = v / L[(i, i)]
            step[:, :, i] = -z[i]
    return step, lam2


def solve(kind, D, E, R, S2=None, ips=None, c=None, max_iter=MAX_ITER, dtype=np.float64, stop=None):
    """The device's iteration for every pair -> dict(eta [T, K, J], n_iter, status [T, K] int32).
    dtype = np.longdouble, stop = 1e-30: the exact reference's (steps accepted at longdouble's rounding floor, stopped
    at a squared decrement <= stop * scale)."""
    dt = np.dtype(dtype)
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    R = R if R.ndim == 3 else np.broadcast_to(R[None], (E.shape[0],) + R.shape)
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    T, K, J = D.shape[0], E.shape[0], R.shape[1]
    ips = (np.zeros(J) if ips is None else np.asarray(ips, dtype=np.float64)).astype(dt)
    c = (np.zeros((K, J)) if c is None else np.asarray(c, dtype=np.float64)).astype(dt)
    w = dt.type(w_of(kind))
    eps = dt.type(np.finfo(dt).eps)
    eta = np.zeros((T, K, J), dtype=dt)
    eta_t, step = eta.copy(), eta.copy()
    Phi, floor_, stop_at, lam2_at = (np.zeros((T, K), dtype=dt) for _ in range(4))
    alpha = np.ones((T, K), dtype=dt)
    n_iter, n_halve, status = (np.zeros((T, K), dtype=np.int32) for _ in range(3))
    cut, boundary, done = (np.zeros((T, K), dtype=bool) for _ in range(3))
    first = True
    while not done.all():
        act = ~done
        inside, ps, pc, scale, g, H = _sweep(kind, D, E, S2, R, eta_t)
        phi_t = ps + pc
        for j in range(J):
            p = ips[j] * (eta_t[:, :, j] + c[None, :, j])
            pp = w * (p * p)
            phi_t = phi_t + pp
            scale = scale + pp
            g[:, :, j] = g[:, :, j] + (2.0 * w) * (ips[j] * p)
            H[(j, j)] = H[(j, j)] + (2.0 * w) * (ips[j] * ips[j])
        if first:
            first = False
            out = act & ~inside
            status[out] |= START_OUTSIDE
            done |= out
            accept = act & inside
        else:
            with np.errstate(invalid="ignore"):
                ok = inside & ((phi_t <= Phi + floor_) | (lam2_at <= floor_))     # (below the floor Phi cannot judge)
            rej = act & ~ok
            cut |= rej & ~inside
            n_halve[rej] += 1
            fail = rej & (n_halve > MAX_HALVINGS)
            status[fail] |= NOT_CONVERGED
            boundary[fail] = cut[fail]
            done |= fail
            halve = rej & ~fail
            alpha[halve] *= 0.5
            eta_t = np.where(halve[:, :, None], eta + alpha[:, :, None] * step, eta_t)
            accept = act & ok
        eta = np.where(accept[:, :, None], eta_t, eta)
        Phi = np.where(accept, phi_t, Phi)
        floor_ = np.where(accept, (0.5 * eps) * scale, floor_)
        stop_at = dt.type(STOP_REL) * floor_ if stop is None else np.where(accept, dt.type(stop) * scale, stop_at)
        boundary = np.where(accept, cut, boundary)
        posfail = accept & _factor(H, J)
        status[posfail] |= NOT_POSDEF
        done |= posfail
        new_step, lam2 = _solve(H, g, J)
        lam2_at = np.where(accept, lam2, lam2_at)
        with np.errstate(invalid="ignore"):
            conv = accept & ~posfail & (lam2 <= stop_at)
        eta = np.where(conv[:, :, None], eta + new_step, eta)      # the last step, applied unchecked
        boundary &= ~conv                                            # (a stationary point inside the domain)
        done |= conv
        maxed = accept & ~posfail & ~conv & (n_iter >= max_iter)
        status[maxed] |= NOT_CONVERGED
        done |= maxed
        go = accept & ~posfail & ~conv & ~maxed
        n_iter[go] += 1
        alpha[go] = 1.0
        n_halve[go] = 0
        cut[go] = False
        step = np.where(go[:, :, None], new_step, step)
        eta_t = np.where(go[:, :, None], eta + alpha[:, :, None] * step, eta_t)
    status[boundary] |= BOUNDARY
    return dict(eta=eta, n_iter=n_iter, status=status)


def value(kind, D, E, R, S2, eta, ips=None, c=None):
    """the reported entry [T, K] at eta [T, K, J]: ens_direct_kernel on the pair's own template row mu(eta) (one
    compensated chain, NaN bins dropped, chi2's whole-map rule per pair), then the prior terms in ascending j through
    `two_sum` (subtracted for the llh kinds) and one last rounding"""
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    R = R if R.ndim == 3 else np.broadcast_to(R[None], (E.shape[0],) + R.shape)
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    K, J = E.shape[0], R.shape[1]
    ips = np.zeros(J) if ips is None else np.asarray(ips, dtype=np.float64)
    c = np.zeros((K, J)) if c is None else np.asarray(c, dtype=np.float64)
    lam = _mu(E, R, eta)
    live = np.isfinite(D)[:, None, :] & np.isfinite(E)[None, :, :] & np.isfinite(lam)
    d = np.broadcast_to(D[:, None, :], lam.shape)
    lg = np.broadcast_to(ec.lgamma1(D)[:, None, :], lam.shape) if kind == "poisson_llh" else None
    v = ec.metric_bin(kind, d, lam, S2[None], lg)
    v = np.where(live & ~np.isnan(v), v, 0.0)
    s = np.zeros(lam.shape[:2])
    comp = np.zeros_like(s)
    for b in range(lam.shape[2]):
        s, comp = two_sum(s, comp, v[:, :, b])
    acc = s + comp
    if kind == "chi2":
        with np.errstate(invalid="ignore"):
            same = np.abs(d - np.maximum(lam, SMALL_POS)) < 5 * EPS
        acc = np.where((same | ~live).all(axis=2), 0.0, acc)
    return join_priors(kind, acc, eta, ips, c)


def join_priors(kind, acc, eta, ips, c):
    """(acc, 0) += -+ w (ips_j (eta_j + c_j))^2 in ascending j through `two_sum`, then acc + comp"""
    w = w_of(kind)
    acc = np.array(acc, dtype=np.float64)
    comp = np.zeros_like(acc)
    for j in range(eta.shape[-1]):
        p = ips[j] * (eta[..., j] + c[None, :, j])
        pp = w * (p * p)
        acc, comp = two_sum(acc, comp, -pp if kind in LLH_KINDS else pp)
    return acc + comp


def restated(kind, D, E, R, S2=None, ips=None, c=None, max_iter=MAX_ITER):
    """`solve` + `value` -> dict(value, eta, n_iter, status): what `kernels.profiled_metric_matrix` returns"""
    out = solve(kind, D, E, R, S2, ips, c, max_iter)
    out["value"] = value(kind, D, E, R, S2, out["eta"], ips, c)
    return out


def reduce_profiled(kind, full, offset=None, k0=0):
    """the reduced output restated on the full one"""
    best, arg, at = ec.reduce_matrix(kind, np.asarray(full["value"]), offset, k0)
    rows = np.arange(arg.size)
    return dict(best=best, arg=arg, at=at, eta_best=full["eta"][rows, arg], eta_at=full["eta"][:, k0],
                status=full["status"][rows, arg] | full["status"][:, k0])


# ------------------------------------------------------------------------------------------ exact values
def _lgamma1_exact(D):
    """lgamma(d + 1) in np.longdouble: a running sum of ln i for counts, mpmath at 40 digits otherwise"""
    ld = np.longdouble
    if np.array_equal(D, np.rint(D)) and D.min() >= 0 and D.max() < 1e7:
        lg = np.concatenate([[ld(0)], np.cumsum(np.log(np.arange(1, int(D.max()) + 1, dtype=ld)))])
        return lg[D.astype(np.int64)]
    import mpmath as mp

    u, inv = np.unique(D, return_inverse=True)
    with mp.workdps(40):
        vals = []
        for x in u:
            r = mp.loggamma(mp.mpf(float(x)) + 1)
            hi = float(r)
            vals.append(ld(hi) + ld(float(r - mp.mpf(hi))))
    return np.array(vals, dtype=ld)[inv].reshape(D.shape)


def exact_value(kind, D, E, R, S2, eta, ips, c):
    """(value [T, K] longdouble, S [T, K] float) at the longdouble eta: the formulae of `ec.exact_longdouble` on the
    pair's own mu(eta), the prior terms, and the gate's scale (module docstring)"""
    ld = np.longdouble
    K, J = E.shape[0], (R.shape[1] if R.ndim == 3 else R.shape[0])
    Rf = R if R.ndim == 3 else np.broadcast_to(R[None], (K,) + R.shape)
    ips = (np.zeros(J) if ips is None else np.asarray(ips)).astype(ld)
    c = (np.zeros((K, J)) if c is None else np.asarray(c)).astype(ld)
    S2 = np.zeros_like(E) if S2 is None else S2
    lam = np.maximum(_mu(E, Rf, eta), ld(SMALL_POS))
    d = np.broadcast_to(D[:, None, :].astype(ld), lam.shape)
    kept = np.ones(lam.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind in LLH_KINDS:
            a = np.where(d > 0, d * np.log(lam), ld(0))
            if kind == "llh":
                cc = np.where(d > 0, d * np.log(np.where(d > 0, d, ld(1))), ld(0))
                v, m = (a - lam) - (cc - d), np.abs(a) + lam + np.abs(cc) + d
                kept = d > 0
            else:
                cc = np.broadcast_to(_lgamma1_exact(D)[:, None, :], lam.shape)
                v, m = (a - lam) - cc, np.abs(a) + lam + np.abs(cc)
            p1 = 1 - d / lam
        else:
            s2 = S2[None].astype(ld) if kind == "mod_chi2" else ld(0)
            vv = s2 + lam
            v = (d - lam) ** 2 / vv
            m = np.abs(v)
            aa = (d - lam) / vv
            p1 = -(aa * (2 + aa))
    reach = np.abs(E)[None].astype(ld)
    for j in range(J):
        reach = reach + np.abs(Rf[None, :, j, :].astype(ld) * eta[:, :, j, None])
    prior = (w_of(kind) * (ips[None, None, :] * (eta + c[None])) ** 2).sum(axis=2)
    val = np.where(kept, v, ld(0)).sum(axis=2)
    val = val - prior if kind in LLH_KINDS else val + prior
    S = np.where(kept, m + 1 + np.abs(p1) * reach, ld(0)).sum(axis=2) + prior
    return val, S.astype(np.float64)


_EXACT_ETA = {}
_EXACT = {}


def exact(name, kind, T, K, B, J):
    """dict(value longdouble, scale, eta longdouble, status) of a gated family: computed once, shared, read-only"""
    key = (name, kind, T, K, B, J)
    if key not in _EXACT:
        f = family(name, T, K, B, J)
        group = "llh" if kind in LLH_KINDS else kind            # the llh kinds minimise the same Phi
        if (name, group, T, K, B, J) not in _EXACT_ETA:
            _EXACT_ETA[(name, group, T, K, B, J)] = solve(group, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"],
                                                          max_iter=200, dtype=np.longdouble, stop=1e-30)
        s = _EXACT_ETA[(name, group, T, K, B, J)]
        val, scale = exact_value(kind, f["D"], f["E"], f["R"], f["S2"], s["eta"], f["ips"], f["c"])
        val.setflags(write=False), scale.setflags(write=False)
        _EXACT[key] = dict(value=val, scale=scale, eta=s["eta"], status=s["status"])
    return _EXACT[key]


def gated_cases():
    return [(name, shape) for name in GATED for shape in shapes_of(name)]


# ------------------------------------------------------------------- the batch evaluator restated in numpy
class NumpyProfileSolver(ec.NumpySolver):
    """`DeviceSolver` with the profiled methods, everything through the restatements"""

    def profiled_matrix(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                        max_iter=MAX_ITER):
        self.calls.append(("profiled_matrix", kind, np.shape(data), np.shape(expected)))
        return restated(kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter)

    def profiled_best(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                      offset=None, k0=0, max_iter=MAX_ITER):
        self.calls.append(("profiled_best", kind, np.shape(data), np.shape(expected)))
        full = restated(kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter)
        return reduce_profiled(kind, full, offset, k0)
