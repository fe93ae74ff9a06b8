"""Shared pieces of the tests of the BOUNDED profiled trial ensembles (csrc/profile_device.hpp: `pf_init_bounded`,
`pf_decide_bounded`; csrc/profile_bounded.hip: `pisa_hip_profiled_metric_matrix_bounded`, `..._best_bounded`) and of the
`lower=` / `upper=` paths of pisa_amd/analysis/ensemble.py.  A plain helper module on top of tests/profile_cases.py (the
unbounded solver's restatement, the case families, the exact value and the gate's scale are taken from there);
`tests/test_host_profiled_bounded.py` pins everything here without a GPU, `tests/test_gpu_profiled_bounded.py` runs
the kernels.

The definition ("Profiled trial ensembles: bounds").  With Phi exactly as in tests/profile_cases.py,

    eta_hat = argmin Phi(eta)  over  lo[k, j] <= eta_j <= hi[k, j]   on the domain mu_b >= SMALL_POS (responding bins)

`solve_bounded` is `profile_cases.solve` with a projected step, change for change what `pf_decide_bounded` adds:
  1. clamp(x) = x < lo ? lo : (x > hi ? hi : x): comparisons, so that a NaN passes through and a clamped coordinate
     holds the bound's own double;
  2. the start is clamp(0), START_OUTSIDE is judged there;
  3. after an accepted sweep at eta the bound set A = {j: (eta_j == lo_j and g_j > 0) or (eta_j == hi_j and g_j < 0)
     or eta_j == lo_j == hi_j} (a pinned coordinate is no variable: set free by a gradient of exactly 0, as at an
     exact fit, it would bring back the singular Hessian it was pinned to avoid) leaves the system: g_j = 0, row and
     column j of H those of the unit matrix, before the factorisation.  The pivot rule, NOT_POSDEF and lam2 are those
     of the free block;
  4. trial points are clamp(eta + alpha step), the last step is applied as clamp(eta + step); acceptance, floor,
     halvings, the stopping rule and BOUNDARY (cut by the domain, not by the box) are unchanged;
  5. a template with a bound that does not satisfy lo <= hi (a NaN included) gives pairs with status BAD_BOUNDS = 16
     that take no step: eta = 0, n_iter = 0, the value is the metric at eta = 0.
The exact reference is the same rule in np.longdouble with stop 1e-30 and max_iter 200, `profile_cases.exact_value` at
its eta.  The gate is profile_cases': |got - exact| <= G eps S with G = KERNEL_FACTOR * max(1, G_REF_B[kind]).

Boxes (`box(name, K, J)` -> (lower, upper) as the caller passes them; eta_j in [-h (1 + 0.1 j), +h (1 + 0.2 j)]):
    wide     h = 0.25, given as [J] (shared by all templates)
    narrow   h = 0.05, given as [K, J] (every row the same box)
    lower    lo = -0.25 (1 + 0.1 j), no upper bound: `upper` is None
Every gated family of profile_cases runs under every box on every shape it has there.  The pseudo-data are drawn at
eta_0 ~ N(0, 0.5), so most pairs end with a coordinate on a bound.

G_REF_B: the worst ratio of `restated_bounded` against the exact reference over every box, family and shape, measured
by tests/test_host_profiled_bounded.py and held against the figures below, never taken from the device.  Measured
(numpy 2.2): 0.813 (llh), 0.982 (poisson_llh), 1.609 (chi2), 1.605 (mod_chi2), so G = 4, 4, 6.44, 6.44; every pair with
status 0 and the same coordinates on a bound in both, 78 % of the pairs with a coordinate on a bound, at most 24
Newton steps on any pair (MOST_STEPS; max_iter is 32).
"""
import numpy as np

from tests import ensemble_cases as ec
from tests import metric_cases as mc
from tests import profile_cases as pc

BAD_BOUNDS = 16
BOXES = ("wide", "narrow", "lower")
H_OF = {"wide": 0.25, "narrow": 0.05, "lower": 0.25}

# worst ratio of the fp64 restatement against the exact reference (module docstring)
G_REF_B = {"llh": 0.82, "poisson_llh": 0.99, "chi2": 1.61, "mod_chi2": 1.61}
MOST_STEPS = 24


def g_of(kind):
    return mc.KERNEL_FACTOR * max(1.0, G_REF_B[kind])


def box(name, K, J):
    """(lower, upper) of a box family as the caller passes them: [J], [K, J] or None"""
    h = H_OF[name]
    j = np.arange(J, dtype=np.float64)
    lo, hi = -h * (1.0 + 0.1 * j), h * (1.0 + 0.2 * j)
    if name == "wide":
        return lo, hi
    if name == "narrow":
        return np.tile(lo, (K, 1)), np.tile(hi, (K, 1))
    if name == "lower":
        return lo, None
    raise KeyError(name)


def own_rows_box(K, J):
    """a [K, J] box that differs from template to template (one row pinned, one row open on one side)"""
    k = np.arange(K, dtype=np.float64)[:, None]
    j = np.arange(J, dtype=np.float64)[None, :]
    lo = -0.02 * (1.0 + (k % 5.0)) * (1.0 + 0.1 * j)
    hi = 0.03 * (1.0 + ((k + 2.0) % 4.0)) * (1.0 + 0.2 * j)
    if K > 1:
        lo[1], hi[1] = 0.01, 0.01          # pinned away from 0
    if K > 2:
        hi[2] = np.inf
    return lo, hi


def full_bounds(lower, upper, K, J, dtype=np.float64):
    """([K, J], [K, J]) of whatever the caller passes: None is no bound on that side, [J] is shared"""
    lo = np.full((K, J), -np.inf) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (K, J))
    hi = np.full((K, J), np.inf) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (K, J))
    return lo.astype(dtype), hi.astype(dtype)


def clamp(x, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.where(x < lo, lo, np.where(x > hi, hi, x))


def bound_set(eta, g, lo, hi):
    """[T, K, J] bool: the coordinates on a bound with the gradient pointing out of the box, and the pinned ones"""
    with np.errstate(invalid="ignore"):
        at_lo, at_hi = eta == lo, eta == hi
        return (at_lo & at_hi) | (at_lo & (g > 0)) | (at_hi & (g < 0))


def on_bound(eta, lower, upper):
    """[T, K, J] int8: -1 where eta equals the lower bound, +1 the upper one, 2 both (pinned), else 0"""
    K, J = eta.shape[1:]
    lo, hi = full_bounds(lower, upper, K, J, eta.dtype)
    at_lo, at_hi = eta == lo[None], eta == hi[None]
    return np.where(at_lo & at_hi, 2, np.where(at_lo, -1, np.where(at_hi, 1, 0))).astype(np.int8)


def solve_bounded(kind, D, E, R, lower=None, upper=None, S2=None, ips=None, c=None, max_iter=pc.MAX_ITER,
                  dtype=np.float64, stop=None):
    """`pf_init_bounded` + `pf_decide_bounded` for every pair -> dict(eta [T, K, J], n_iter, status [T, K] int32).
    `profile_cases.solve` line for line, with the five changes of the module docstring."""
    dt = np.dtype(dtype)
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    R = R if R.ndim == 3 else np.broadcast_to(R[None], (E.shape[0],) + R.shape)
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    T, K, J = D.shape[0], E.shape[0], R.shape[1]
    ips = (np.zeros(J) if ips is None else np.asarray(ips, dtype=np.float64)).astype(dt)
    c = (np.zeros((K, J)) if c is None else np.asarray(c, dtype=np.float64)).astype(dt)
    lo, hi = full_bounds(lower, upper, K, J, dt)
    with np.errstate(invalid="ignore"):
        bad = np.broadcast_to(~(lo <= hi).all(axis=1)[None, :], (T, K))
    lo, hi = lo[None], hi[None]
    w = dt.type(pc.w_of(kind))
    eps = dt.type(np.finfo(dt).eps)
    zero = np.zeros((T, K, J), dtype=dt)
    eta = np.where(bad[:, :, None], zero, clamp(zero, lo, hi))
    eta_t, step = eta.copy(), zero.copy()
    Phi, floor_, stop_at, lam2_at = (np.zeros((T, K), dtype=dt) for _ in range(4))
    alpha = np.ones((T, K), dtype=dt)
    n_iter, n_halve, status = (np.zeros((T, K), dtype=np.int32) for _ in range(3))
    cut, boundary = (np.zeros((T, K), dtype=bool) for _ in range(2))
    done = bad.copy()
    status[bad] |= BAD_BOUNDS
    first = True
    while not done.all():
        act = ~done
        inside, ps, pcomp, scale, g, H = pc._sweep(kind, D, E, S2, R, eta_t)
        phi_t = ps + pcomp
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
            status[out] |= pc.START_OUTSIDE
            done |= out
            accept = act & inside
        else:
            with np.errstate(invalid="ignore"):
                ok = inside & ((phi_t <= Phi + floor_) | (lam2_at <= floor_))
            rej = act & ~ok
            cut |= rej & ~inside
            n_halve[rej] += 1
            fail = rej & (n_halve > pc.MAX_HALVINGS)
            status[fail] |= pc.NOT_CONVERGED
            boundary[fail] = cut[fail]
            done |= fail
            halve = rej & ~fail
            alpha[halve] *= 0.5
            eta_t = np.where(halve[:, :, None], clamp(eta + alpha[:, :, None] * step, lo, hi), eta_t)
            accept = act & ok
        eta = np.where(accept[:, :, None], eta_t, eta)
        Phi = np.where(accept, phi_t, Phi)
        floor_ = np.where(accept, (0.5 * eps) * scale, floor_)
        stop_at = dt.type(pc.STOP_REL) * floor_ if stop is None else np.where(accept, dt.type(stop) * scale, stop_at)
        boundary = np.where(accept, cut, boundary)
        # the bound set leaves the system (`pf_bind`)
        A = bound_set(eta, g, lo, hi)
        g = np.where(A, dt.type(0), g)
        for i in range(J):
            for j in range(i + 1):
                H[(i, j)] = np.where(A[:, :, i] | A[:, :, j], dt.type(1.0 if i == j else 0.0), H[(i, j)])
        posfail = accept & pc._factor(H, J)
        status[posfail] |= pc.NOT_POSDEF
        done |= posfail
        new_step, lam2 = pc._solve(H, g, J)
        lam2_at = np.where(accept, lam2, lam2_at)
        with np.errstate(invalid="ignore"):
            conv = accept & ~posfail & (lam2 <= stop_at)
        eta = np.where(conv[:, :, None], clamp(eta + new_step, lo, hi), eta)
        boundary &= ~conv
        done |= conv
        maxed = accept & ~posfail & ~conv & (n_iter >= max_iter)
        status[maxed] |= pc.NOT_CONVERGED
        done |= maxed
        go = accept & ~posfail & ~conv & ~maxed
        n_iter[go] += 1
        alpha[go] = 1.0
        n_halve[go] = 0
        cut[go] = False
        step = np.where(go[:, :, None], new_step, step)
        eta_t = np.where(go[:, :, None], clamp(eta + alpha[:, :, None] * step, lo, hi), eta_t)
    status[boundary] |= pc.BOUNDARY
    return dict(eta=eta, n_iter=n_iter, status=status)


def restated_bounded(kind, D, E, R, lower=None, upper=None, S2=None, ips=None, c=None, max_iter=pc.MAX_ITER):
    """`solve_bounded` + `profile_cases.value`: what `kernels.profiled_metric_matrix(..., lower=, upper=)` returns"""
    out = solve_bounded(kind, D, E, R, lower, upper, S2, ips, c, max_iter)
    out["value"] = pc.value(kind, D, E, R, S2, out["eta"], ips, c)
    return out


# ------------------------------------------------------------------------------------------ exact values
_EXACT_ETA = {}
_EXACT = {}


def exact_bounded(name, bx, kind, T, K, B, J):
    """dict(value longdouble, scale, eta longdouble, status, n_iter) of a gated family under a box: computed once,
    shared, read-only"""
    key = (name, bx, kind, T, K, B, J)
    if key not in _EXACT:
        f = pc.family(name, T, K, B, J)
        group = "llh" if kind in pc.LLH_KINDS else kind
        gk = (name, bx, group, T, K, B, J)
        if gk not in _EXACT_ETA:
            lower, upper = box(bx, K, J)
            _EXACT_ETA[gk] = solve_bounded(group, f["D"], f["E"], f["R"], lower, upper, f["S2"], f["ips"], f["c"],
                                           max_iter=200, dtype=np.longdouble, stop=1e-30)
        s = _EXACT_ETA[gk]
        val, scale = pc.exact_value(kind, f["D"], f["E"], f["R"], f["S2"], s["eta"], f["ips"], f["c"])
        val.setflags(write=False), scale.setflags(write=False)
        _EXACT[key] = dict(value=val, scale=scale, eta=s["eta"], status=s["status"], n_iter=s["n_iter"])
    return _EXACT[key]


def gated_cases():
    return [(name, bx, shape) for name in pc.GATED for bx in BOXES for shape in pc.shapes_of(name)]


def gradient(kind, f, eta):
    """(g [T, K, J], diagonal of H [T, K, J], floor [T, K]) of Phi at eta in np.longdouble, priors included; floor
    is the fp64 rounding floor of Phi that the solver judges a step by"""
    ld = np.longdouble
    eta = np.asarray(eta, dtype=ld)
    E = np.asarray(f["E"], dtype=np.float64)
    R = np.asarray(f["R"], dtype=np.float64)
    R = R if R.ndim == 3 else np.broadcast_to(R[None], (E.shape[0],) + R.shape)
    K, J = E.shape[0], R.shape[1]
    _, _, _, scale, g, H = pc._sweep(kind, np.asarray(f["D"], dtype=np.float64), E, np.asarray(f["S2"]), R, eta)
    ips = (np.zeros(J) if f["ips"] is None else np.asarray(f["ips"])).astype(ld)
    c = (np.zeros((K, J)) if f["c"] is None else np.asarray(f["c"])).astype(ld)
    w = ld(pc.w_of(kind))
    diag = np.empty_like(g)
    for j in range(J):
        p = ips[j] * (eta[:, :, j] + c[None, :, j])
        scale = scale + w * (p * p)
        g[:, :, j] = g[:, :, j] + (2 * w) * (ips[j] * p)
        diag[:, :, j] = H[(j, j)] + (2 * w) * (ips[j] * ips[j])
    return g, diag, (0.5 * pc.EPS) * scale.astype(np.float64)


# ------------------------------------------------------------------- status families under a box
def status_family(name):
    """dict(kind, D, E, S2, R, ips, c, lower, upper, max_iter)
    bad            three templates, the second with lo > hi in one parameter: its pairs carry BAD_BOUNDS alone
    bad_nan        the same with a NaN bound
    start_clamped  a box that excludes 0: the fit starts at the clamped point
    posdef_pinned  `posdef` of profile_cases (J = 3 > B = 2, no priors) with J - B parameters pinned at 0
    posdef         the same case under an infinite box: flagged as before
    maxiter        `maxiter` of profile_cases (`far`, max_iter = 1) under a box the fit does not reach
    start          `start` of profile_cases (a responding bin with E = 1e-11 in template 1) under the wide box"""
    if name in ("bad", "bad_nan", "start_clamped"):
        f = dict(pc.family("poisson", 63, 3, 3, 2), kind="llh", max_iter=pc.MAX_ITER)
        lo, hi = np.tile(np.array([-0.25, -0.3]), (3, 1)), np.tile(np.array([0.25, 0.3]), (3, 1))
        if name == "bad":
            lo[1, 1], hi[1, 1] = 0.2, 0.1
        elif name == "bad_nan":
            hi[1, 0] = np.nan
        else:
            lo[:, 0], hi[:, 0] = 0.05, 0.4
            lo[:, 1], hi[:, 1] = -0.4, -0.02
        return dict(f, lower=lo, upper=hi)
    if name in ("posdef", "posdef_pinned"):
        f = pc.status_family("posdef")
        J = f["R"].shape[1]
        if name == "posdef":
            return dict(f, lower=np.full(J, -np.inf), upper=np.full(J, np.inf))
        lo, hi = np.full(J, -np.inf), np.full(J, np.inf)
        lo[2:] = hi[2:] = 0.0                    # B = 2 parameters stay free
        return dict(f, lower=lo, upper=hi)
    if name == "maxiter":
        f = pc.status_family(name)
        return dict(f, lower=np.array([-10.0]), upper=np.array([10.0]))
    if name == "start":
        f = pc.status_family(name)
        lower, upper = box("wide", f["E"].shape[0], f["R"].shape[-2])
        return dict(f, lower=lower, upper=upper)
    raise KeyError(name)


STATUS_FAMILIES = ("bad", "bad_nan", "start_clamped", "posdef_pinned", "posdef", "maxiter", "start")


# ------------------------------------------------------------------- the batch evaluator restated in numpy
class NumpyBoundedProfileSolver(pc.NumpyProfileSolver):
    """`DeviceSolver` with the profiled methods and their `lower=` / `upper=`, everything through the restatements"""

    def profiled_matrix(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                        max_iter=pc.MAX_ITER, lower=None, upper=None):
        self.calls.append(("profiled_matrix", kind, np.shape(data), np.shape(expected),
                           lower is not None or upper is not None))
        return restated_bounded(kind, data, expected, response, lower, upper, sigma2, inv_prior_sigma, center, max_iter)

    def profiled_best(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                      offset=None, k0=0, max_iter=pc.MAX_ITER, lower=None, upper=None):
        self.calls.append(("profiled_best", kind, np.shape(data), np.shape(expected),
                           lower is not None or upper is not None))
        full = restated_bounded(kind, data, expected, response, lower, upper, sigma2, inv_prior_sigma, center, max_iter)
        return pc.reduce_profiled(kind, full, offset, k0)
