"""Shared pieces of the tests of the LOG-LINEAR response of the profiled trial ensembles (csrc/profile_wide_device.hpp:
`pfw_mu_loglinear`, `pfw_bins_loglinear`; csrc/profile_loglinear.hip: `pisa_hip_profiled_metric_matrix_wide_form`,
`..._best_wide_form`; DESIGN.md §4, "Profiled trial ensembles: the log-linear response") and of the `form=` paths of
pisa_amd/analysis/ensemble.py.  A plain helper module on top of tests/profile_cases.py and
tests/profile_bounded_cases.py; `tests/test_host_profiled_loglinear.py` pins everything here without a GPU,
`tests/test_gpu_profiled_loglinear.py` runs the kernels.

The definition.  For data row t, template row k, eta in R^J:

    s_b  = rho[k,0,b] eta_0 + ... + rho[k,J-1,b] eta_{J-1}          (from 0 in ascending j, every product rounded)
    a_b  = |rho[k,0,b] eta_0| + ...                                   (the same way)
    mu_b = E[k,b] exp(s_b)     where E[k,b] != 0 and some rho[k,j,b] != 0 (the bin responds), else mu_b = E[k,b]
    Phi(eta) = sum_b phi(d_b, mu_b, s2_b) + w sum_j (ips_j (eta_j + c[k,j]))^2

with phi, w, the priors, the domain (a responding bin with mu_b not finite or below SMALL_POS is outside it), the damped
Newton state machine, the box, the stop rule and the flags of tests/profile_cases.py and tests/profile_bounded_cases.py.
The restatement is exactly that: `profile_cases.solve` and `profile_bounded_cases.solve_bounded` run with their sweep
over the bins (`profile_cases._sweep`) replaced by `_sweep` below (`_state_machine`), which hands them the gradient and
Hessian of the exponential model,

    g_j = sum_b (phi' m) rho_jb,    H_ij = sum_b ((phi'' m) m + phi' m) rho_ib rho_jb,    m = max(mu, SMALL_POS),

zeros from a bin that does not respond (it is a constant of Phi), and the bin's term of `scale` with reach_b = m_b (2 +
a_b): mu carries the rounding of s (|s| <= a relative to mu), of exp and of one product.  `value` is the reported entry:
the direct form on mu(eta_hat) formed by the same function, then the priors as `profile_cases.join_priors` joins them.

The exact reference is the same in np.longdouble with max_iter = 200 and stop 1e-30; `exact_value` is
`profile_cases.exact_value` with this mu and this reach.  The gate is the project's: |got - exact| <= G eps S, G =
KERNEL_FACTOR * max(1, recorded worst ratio of the restatement), never taken from the device.  numpy's exp is not
libm's nor the device's, so a kernel's value is compared through the gate and its eta with a tolerance, not with `==`.

Families (`family(name, T, K, B, J)`: those of profile_cases rebuilt for the exponential model; truths eta0 ~ N(0, 0.5),
data drawn at E exp(rho . eta0)):
    poisson  rho = 0.1 x cosines, unit priors (so that J > B is fitted)
    shared   the [J, B] response shared by all templates, priors of weight 0.5
    asimov   data at mu(eta0) exactly, no priors: needs J < B (without priors the fit has a unique minimum only where
             the J shapes are independent on the B bins, and the B-th cosine vanishes on every bin centre)
    prior    ips alternating 0 / 1 with non-zero c, the last parameter with rho = 0 and a prior: eta_hat = -c there;
             needs 2 <= J <= B (the cosines above the B-th alias onto lower ones on B bin centres, and every second
             parameter has no prior to tell them apart; measured: NOT_POSDEF pairs at B = 20, J = 32)
    norm     rho = 1, J = 1, no prior: eta_hat = ln(sum d / sum E) for the llh kinds
    far      D = 3 E, rho = 1: eta_hat = ln 3 on the pair's own template
    low      D = E / 4, rho = 1: eta_hat = -ln 4
Status families (`status_family(name)`, flags compared with `==` against the restatement): `start` (that of
profile_cases: a responding bin with E = 1e-11), `posdef` (J = 3 > B = 2, no priors), `maxiter` (`far` with max_iter =
1), `overflow` (E = (50, 50), rho = (1, -1), data rows (5e5, 50) and (50, 5e5), no prior: the first full Newton step is
about +-5000, exp overflows, the trial point is outside the domain and the damping halves the step: status 0).

Measured on the CPU by tests/test_host_profiled_loglinear.py (numpy 2.2) and held against the constants below:
unbounded 0.503 (llh), 0.739 (poisson_llh), 0.159 (chi2), 0.199 (mod_chi2); bounded 0.595, 0.882, 0.311, 0.287: G = 4
for every kind in both forms; at most 7 Newton steps on any gated pair, 89 % of the bounded pairs with a coordinate
on a bound; `overflow` ends with status 0 after 6 steps (llh kinds) and 12 (chi2 kinds).
"""
import contextlib

import numpy as np

from tests import ensemble_cases as ec
from tests import metric_cases as mc
from tests import profile_bounded_cases as pbc
from tests import profile_cases as pc

EPS = pc.EPS
SMALL_POS = pc.SMALL_POS
KINDS = pc.KINDS
LLH_KINDS = pc.LLH_KINDS
MAX_ITER = pc.MAX_ITER
LINEAR, LOGLINEAR = 0, 1       # PISA_HIP_RESPONSE_*

GATED = ("poisson", "shared", "asimov", "prior", "norm", "far", "low")
ONE_PARAMETER = ("norm", "far", "low")
# (T, K, B, J): J edges of the 4 x 4 tiles (1, 4, 5, 9, 12, 16, 17, 31, 32), B edges of the chunk of 64 (1, 63, 64,
# 65, 130) and J > B (20 bins, 32 parameters); many templates per trial: (2, 300, 12, 12) goes through the split of the
# reduced output over workgroups and the join
SHAPES = ((1, 1, 1, 1), (1, 1, 1, 9), (2, 3, 63, 4), (2, 3, 64, 5), (2, 2, 65, 9), (1, 2, 130, 16), (2, 2, 64, 17),
          (1, 2, 130, 31), (1, 2, 130, 32), (2, 2, 20, 32), (8, 30, 12, 12), (2, 300, 12, 12))
ONE_PARAMETER_SHAPES = ((3, 2, 3, 1), (65, 1, 3, 1), (2, 3, 130, 1))
BOUNDED_SHAPES = ((2, 3, 64, 5), (1, 2, 130, 32), (3, 2, 3, 1))
STATUS_FAMILIES = ("start", "posdef", "maxiter", "overflow")

# worst ratio of the fp64 restatement against the exact reference, unbounded and bounded (module docstring)
G_REF_L = {"llh": 0.51, "poisson_llh": 0.75, "chi2": 0.17, "mod_chi2": 0.21}
G_REF_LB = {"llh": 0.60, "poisson_llh": 0.89, "chi2": 0.32, "mod_chi2": 0.30}
MOST_STEPS_L = 7


def g_of(kind, bounded=False):
    return mc.KERNEL_FACTOR * max(1.0, (G_REF_LB if bounded else G_REF_L)[kind])


def shapes_of(name):
    """the gated shapes a family runs on (module docstring: what each family needs of J and B)"""
    if name in ONE_PARAMETER:
        return ONE_PARAMETER_SHAPES
    if name == "asimov":
        return tuple(s for s in SHAPES if s[3] < s[2])
    if name == "prior":
        return tuple(s for s in SHAPES if 2 <= s[3] <= s[2])
    return SHAPES


def gated_cases():
    return [(name, shape) for name in GATED for shape in shapes_of(name)]


def gated_bounded_cases():
    return [(name, bx, shape) for name in GATED for bx in pbc.BOXES for shape in BOUNDED_SHAPES
            if shape in shapes_of(name)]


# ------------------------------------------------------------------------------------- case families
_FAM = {}


def family(name, T, K, B, J):
    """dict(D [T, B], E [K, B], S2 [K, B], R: rho [K, J, B] or [J, B], ips [J] or None, c [K, J] or None, eta0 [T, J]):
    seeded, built once, read-only"""
    key = (name, T, K, B, J)
    if key in _FAM:
        return _FAM[key]
    rs = ec._rs("profile-loglinear", name, T, K, B, J)
    own = np.arange(T) % K
    eta0 = 0.5 * rs.randn(T, J)
    ips = c = None
    if name in ("poisson", "shared", "asimov", "prior"):
        E = pc._templates(rs, K, B)
        if name == "shared":
            rho = 0.1 * pc._cosines(1, J, B)[0]
            ips = np.full(J, 0.5)
        else:
            rho = 0.1 * pc._cosines(K, J, B)
        if name == "poisson":
            ips = np.ones(J)
        if name == "prior":
            ips = (np.arange(J) % 2).astype(np.float64)
            ips[J - 1] = 1.0
            rho[:, J - 1, :] = 0.0
            c = 0.3 * np.sin(1.0 + np.arange(K)[:, None] + np.arange(J)[None, :])
        mu0 = mu_of(E, rho, np.broadcast_to(eta0[:, None, :], (T, K, J)))[0][np.arange(T), own]
        D = mu0.copy() if name == "asimov" else rs.poisson(mu0).astype(np.float64)
    elif name == "norm":
        assert J == 1
        E = pc._templates(rs, K, B, levels=(50.0, 5e3))
        rho = np.ones((K, 1, B))
        D = rs.poisson(E[own] * np.exp(eta0)).astype(np.float64)
    elif name in ("far", "low"):
        assert J == 1
        E = pc._templates(rs, K, B, integer=True)    # multiples of 4: 3 E and E / 4 are counts
        rho = np.ones((K, 1, B))
        D = 3.0 * E[own] if name == "far" else E[own] / 4.0
    else:
        raise KeyError(name)
    f = dict(D=D, E=E, S2=np.abs(0.3 * E * rs.randn(K, B)), R=rho, ips=ips, c=c, eta0=eta0)
    for v in f.values():
        if v is not None:
            v.setflags(write=False)
    _FAM[key] = f
    return f


def status_family(name):
    """dict(kind, D, E, S2, R: rho, ips, c, max_iter): small cases for the flags (module docstring)"""
    if name == "start":
        f = pc.status_family("start")
        return dict(f, R=f["R"] / 50.0)              # (its responses are 0.1 x cosines x 50)
    if name == "posdef":
        f = pc.status_family("posdef")
        return dict(f, R=f["R"] / f["E"][:, None, :])
    if name == "maxiter":
        f = family("far", 65, 1, 3, 1)
        return dict(kind="mod_chi2", D=f["D"], E=f["E"], S2=f["S2"], R=f["R"], ips=None, c=None, max_iter=1)
    if name == "overflow":
        E = np.array([[50.0, 50.0]])
        return dict(kind="llh", D=np.array([[5e5, 50.0], [50.0, 5e5]]), E=E, S2=0.1 * E,
                    R=np.array([[[1.0, -1.0]]]), ips=None, c=None, max_iter=MAX_ITER)
    raise KeyError(name)


# ------------------------------------------------------------------------------- the sweep, any precision
def _full(R, K):
    R = np.asarray(R, dtype=np.float64)
    return R if R.ndim == 3 else np.broadcast_to(R[None], (K,) + R.shape)


def mu_of(E, rho, eta):
    """(mu [T, K, B], a [T, K, B], responds [K, B]) at eta [T, K, J] in eta's precision: `pfw_mu_loglinear`"""
    dt = eta.dtype
    rho = _full(rho, E.shape[0])
    s = np.zeros(eta.shape[:2] + E.shape[1:], dtype=dt)
    a = np.zeros_like(s)
    for j in range(rho.shape[1]):
        t = rho[None, :, j, :].astype(dt) * eta[:, :, j, None]
        s = s + t
        a = a + np.abs(t)
    responds = (rho != 0).any(axis=1) & (E != 0)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.exp(np.where(responds[None], s, dt.type(0)))
        mu = np.where(responds[None], E[None].astype(dt) * x, E[None].astype(dt))
    return mu, a, responds


def _sweep(kind, D, E, S2, R, eta_t):
    """`pfw_bins_loglinear` + `pfw_chains` over all bins of all pairs at eta_t: what `profile_cases._sweep` returns"""
    dt = eta_t.dtype
    J = R.shape[1]
    live = (np.isfinite(D)[:, None, :] & np.isfinite(E)[None, :, :])
    mu, a, responds = mu_of(E, R, eta_t)
    with np.errstate(all="ignore"):
        inside = ~(live & responds[None] & (~(mu >= SMALL_POS) | np.isinf(mu))).any(axis=2)
        m = np.where(mu < SMALL_POS, dt.type(SMALL_POS), mu)
        d = D[:, None, :].astype(dt)
        if kind in LLH_KINDS:
            q = d / m
            phi, f1, f2 = m - d * np.log(m), 1.0 - q, q / m
        else:
            s2 = S2[None].astype(dt) if kind == "mod_chi2" else None
            v = s2 + m if kind == "mod_chi2" else m
            rr = d - m
            aa = rr / v
            u = ((d + s2) if kind == "mod_chi2" else d) / v
            phi, f1, f2 = rr * aa, -(aa * (2.0 + aa)), 2.0 * (u * u) / v
        zero = dt.type(0)
        p1 = f1 * m
        p2 = (f2 * m) * m + p1
        on = live & responds[None]
        phi, p1, p2 = np.where(live, phi, zero), np.where(on, p1, zero), np.where(on, p2, zero)
        s = np.zeros(mu.shape[:2], dtype=dt)
        c = np.zeros_like(s)
        for b in range(mu.shape[2]):
            s, c = pc.two_sum(s, c, phi[:, :, b])
        scale = pc._chain(np.where(live, (np.abs(phi) + 1.0) + np.abs(f1) * (m * (2.0 + a)), zero))
        g = np.empty(mu.shape[:2] + (J,), dtype=dt)
        H = {}
        Rb = R[None].astype(dt)
        for i in range(J):
            g[:, :, i] = pc._chain(p1 * Rb[:, :, i])
            hi = p2 * Rb[:, :, i]
            for j in range(i + 1):
                H[(i, j)] = pc._chain(hi * Rb[:, :, j])
    return inside, s, c, scale, g, H


@contextlib.contextmanager
def _state_machine():
    """the project's own Newton state machines (`profile_cases.solve`, `profile_bounded_cases.solve_bounded`) with only
    the sweep replaced: both read `profile_cases._sweep` when they run"""
    linear = pc._sweep
    pc._sweep = _sweep
    try:
        yield
    finally:
        pc._sweep = linear


def solve(kind, D, E, rho, S2=None, ips=None, c=None, max_iter=MAX_ITER, lower=None, upper=None, dtype=np.float64,
          stop=None):
    """dict(eta [T, K, J], n_iter, status [T, K]) of the log-linear fit; with lower / upper the bounded one"""
    with _state_machine():
        if lower is None and upper is None:
            return pc.solve(kind, D, E, rho, S2, ips, c, max_iter, dtype, stop)
        return pbc.solve_bounded(kind, D, E, rho, lower, upper, S2, ips, c, max_iter, dtype, stop)


def value(kind, D, E, rho, S2, eta, ips=None, c=None):
    """`profile_cases.value` on the log-linear template mu(eta)"""
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    eta = np.asarray(eta, dtype=np.float64)
    K, J = E.shape[0], eta.shape[-1]
    ips = np.zeros(J) if ips is None else np.asarray(ips, dtype=np.float64)
    c = np.zeros((K, J)) if c is None else np.asarray(c, dtype=np.float64)
    lam = mu_of(E, rho, eta)[0]
    live = np.isfinite(D)[:, None, :] & np.isfinite(E)[None, :, :] & np.isfinite(lam)
    d = np.broadcast_to(D[:, None, :], lam.shape)
    lg = np.broadcast_to(ec.lgamma1(D)[:, None, :], lam.shape) if kind == "poisson_llh" else None
    v = ec.metric_bin(kind, d, lam, S2[None], lg)
    v = np.where(live & ~np.isnan(v), v, 0.0)
    s = np.zeros(lam.shape[:2])
    comp = np.zeros_like(s)
    for b in range(lam.shape[2]):
        s, comp = pc.two_sum(s, comp, v[:, :, b])
    acc = s + comp
    if kind == "chi2":
        with np.errstate(invalid="ignore"):
            same = np.abs(d - np.maximum(lam, SMALL_POS)) < 5 * EPS
        acc = np.where((same | ~live).all(axis=2), 0.0, acc)
    return pc.join_priors(kind, acc, eta, ips, c)


def restated(kind, D, E, rho, S2=None, ips=None, c=None, max_iter=MAX_ITER, lower=None, upper=None):
    """`solve` + `value` -> dict(value, eta, n_iter, status): what `kernels.profiled_metric_matrix_wide(...,
    form="loglinear")` returns"""
    out = solve(kind, D, E, rho, S2, ips, c, max_iter, lower, upper)
    out["value"] = value(kind, D, E, rho, S2, out["eta"], ips, c)
    return out


def exact_value(kind, D, E, rho, S2, eta, ips, c):
    """(value [T, K] longdouble, S [T, K] float) at the longdouble eta: `profile_cases.exact_value` with the log-linear
    mu and reach_b = m_b (2 + a_b)"""
    ld = np.longdouble
    K, J = E.shape[0], eta.shape[-1]
    ips = (np.zeros(J) if ips is None else np.asarray(ips)).astype(ld)
    c = (np.zeros((K, J)) if c is None else np.asarray(c)).astype(ld)
    S2 = np.zeros_like(E) if S2 is None else S2
    mu, a, _ = mu_of(E, rho, np.asarray(eta, dtype=ld))
    lam = np.maximum(mu, ld(SMALL_POS))
    d = np.broadcast_to(D[:, None, :].astype(ld), lam.shape)
    kept = np.ones(lam.shape, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind in LLH_KINDS:
            t = np.where(d > 0, d * np.log(lam), ld(0))
            if kind == "llh":
                cc = np.where(d > 0, d * np.log(np.where(d > 0, d, ld(1))), ld(0))
                v, m = (t - lam) - (cc - d), np.abs(t) + lam + np.abs(cc) + d
                kept = d > 0
            else:
                cc = np.broadcast_to(pc._lgamma1_exact(D)[:, None, :], lam.shape)
                v, m = (t - lam) - cc, np.abs(t) + lam + np.abs(cc)
            p1 = 1 - d / lam
        else:
            s2 = S2[None].astype(ld) if kind == "mod_chi2" else ld(0)
            vv = s2 + lam
            v = (d - lam) ** 2 / vv
            m = np.abs(v)
            aa = (d - lam) / vv
            p1 = -(aa * (2 + aa))
    reach = lam * (2 + a)
    prior = (pc.w_of(kind) * (ips[None, None, :] * (eta + c[None])) ** 2).sum(axis=2)
    val = np.where(kept, v, ld(0)).sum(axis=2)
    val = val - prior if kind in LLH_KINDS else val + prior
    S = np.where(kept, m + 1 + np.abs(p1) * reach, ld(0)).sum(axis=2) + prior
    return val, S.astype(np.float64)


_EXACT_ETA = {}
_EXACT = {}
_RESTATED = {}


def exact(name, kind, shape, bx=None):
    """dict(value longdouble, scale, eta longdouble, status, n_iter) of a gated family (`bx`: None or a box of
    profile_bounded_cases): computed once, shared, read-only"""
    key = (name, kind, shape, bx)
    if key not in _EXACT:
        f = family(name, *shape)
        group = "llh" if kind in LLH_KINDS else kind            # the llh kinds minimise the same Phi
        gk = (name, group, shape, bx)
        if gk not in _EXACT_ETA:
            lower, upper = (None, None) if bx is None else pbc.box(bx, shape[1], shape[3])
            _EXACT_ETA[gk] = solve(group, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], 200, lower, upper,
                                   dtype=np.longdouble, stop=1e-30)
        s = _EXACT_ETA[gk]
        val, scale = exact_value(kind, f["D"], f["E"], f["R"], f["S2"], s["eta"], f["ips"], f["c"])
        val.setflags(write=False), scale.setflags(write=False)
        _EXACT[key] = dict(value=val, scale=scale, eta=s["eta"], status=s["status"], n_iter=s["n_iter"])
    return _EXACT[key]


def restated_case(name, kind, shape, bx=None):
    """the restatement's outputs of a gated case: computed once, shared, read-only"""
    key = (name, kind, shape, bx)
    if key not in _RESTATED:
        f = family(name, *shape)
        lower, upper = (None, None) if bx is None else pbc.box(bx, shape[1], shape[3])
        out = restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"], MAX_ITER, lower, upper)
        for v in out.values():
            v.setflags(write=False)
        _RESTATED[key] = out
    return _RESTATED[key]


# ------------------------------------------------------------------- the batch evaluator restated in numpy
class NumpyFormSolver(pbc.NumpyBoundedProfileSolver):
    """`DeviceSolver` with the profiled methods and their `lower=` / `upper=`, `wide=` and `form=`, everything through
    the restatements (which are generic in J: `wide` changes nothing)"""

    def profiled_matrix(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                        max_iter=MAX_ITER, lower=None, upper=None, wide=False, form="linear"):
        self.calls.append(("form", form, bool(wide)))
        if form == "linear":
            return super().profiled_matrix(kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter,
                                           lower, upper)
        assert form == "loglinear", form
        return restated(kind, np.asarray(data), np.asarray(expected), response, sigma2, inv_prior_sigma, center,
                        max_iter, lower, upper)

    def profiled_best(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                      offset=None, k0=0, max_iter=MAX_ITER, lower=None, upper=None, wide=False, form="linear"):
        self.calls.append(("form", form, bool(wide)))
        if form == "linear":
            return super().profiled_best(kind, data, expected, response, sigma2, inv_prior_sigma, center, offset, k0,
                                         max_iter, lower, upper)
        assert form == "loglinear", form
        full = restated(kind, np.asarray(data), np.asarray(expected), response, sigma2, inv_prior_sigma, center,
                        max_iter, lower, upper)
        return pc.reduce_profiled(kind, full, offset, k0)


# ------------------------------------------------------------------- the toy grid with a log-linear response
def toy(metric, n_j, form="loglinear", bounded=False):
    """The toy grid of tests/ensemble_cases.py with n_j nuisance parameters that are not dimensions of the grid: a
    normalisation with a 10 % Gaussian prior that sits 0.05 above its mean at every point, then cosine modes of falling
    size with a Gaussian prior of width 0.2 on every second one.  form="loglinear": rho holds the modes (the template
    is hist * exp(modes . eta)); form="linear": the response hist * modes, the same to first order (a wide response).
    -> (grid, response, the points' penalty without the response's share)"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    K, B = hist.shape
    x = (np.arange(B) + 0.5) / B
    modes = np.stack([np.ones(B)] + [np.cos(j * np.pi * x) / (1.0 + j) for j in range(1, n_j)])
    R = np.ascontiguousarray(np.broadcast_to(modes[None], (K, n_j, B))) if form == "loglinear" else (
        hist[:, None, :] * modes[None])
    ips = np.array([10.0] + [5.0 if j % 2 else 0.0 for j in range(1, n_j)])
    center = np.zeros((K, n_j))
    center[:, 0] = 0.05
    share = (ips[0] * 0.05) ** 2 * (1.0 if metric in ("chi2", "mod_chi2") else -0.5)
    prior_at_point = np.full(K, share)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty + prior_at_point, metric)
    kw = dict(lower=np.full(n_j, -0.2), upper=np.full(n_j, 0.3)) if bounded else {}
    kw.update(dict(form=form) if form != "linear" else dict(wide=True))
    resp = en.NuisanceResponse(tuple("p%d" % j for j in range(n_j)), R, ips, center, prior_at_point,
                               np.zeros((K, n_j)), **kw)
    return grid, resp, penalty
