"""Shared by tests/test_host_hsfit.py and tests/test_gpu_hsfit.py: a plain numpy restatement of the
hypersurface fit (pisa/utils/hypersurface/hypersurface.py:699-959) and the seeded inputs of the tests.

    eta_n = c_0 + sum_p f_p(x_pn; c_p),  m_n = exp(eta_n) in log mode, eta_n otherwise
    L(c)  = sum_used ((m_n - y_n) / sigma_n)^2 + sum_i (inv_prior_sigma_i c_i)^2          (:847-852)

The first derivatives are the gradient functions of `HYPERSURFACE_PARAM_FUNCTIONS`; the second derivatives
are restated here (and checked against central differences of the first).  The half-gradient and the EXACT
half-Hessian of L are accumulated in np.longdouble; the covariance HESSE estimates with
errordef = LEAST_SQUARES is the inverse of that half-Hessian.  `lm_fit` is a simple Levenberg-Marquardt
with a Newton polish to a Newton-decrement criterion (the kernel's algorithm step for step), the solver the host tests hand to `Hypersurface.fit`.
"""
import numpy as np

from pisa_amd.utils.hypersurface import HYPERSURFACE_PARAM_FUNCTIONS

LD = np.longdouble


def second_derivatives(func_name, x, *c):
    """[k][l] second derivatives of the functional form wrt its coefficients, at x"""
    x = np.asarray(x)
    zero = np.zeros_like(x * c[0])
    if func_name in ("linear",):
        return [[zero]]
    if func_name == "quadratic":
        return [[zero, zero], [zero, zero]]
    if func_name == "exponential":
        return [[x * x * np.exp(c[0] * x)]]
    if func_name == "exponential_scaled":
        a, b = c
        e = np.exp(b * x)
        return [[zero, x * e], [x * e, (a + 1.0) * x * x * e]]
    if func_name == "logarithmic":
        t = 1 + c[0] * x
        return [[-(x * x) / (t * t)]]
    raise ValueError(func_name)


def layout(forms):
    """first coefficient index of every parameter (0 is the intercept) and the total"""
    first, n = [], 1
    for f in forms:
        first.append(n)
        n += HYPERSURFACE_PARAM_FUNCTIONS[f][0]
    return first, n


def model(forms, x, c, log_mode, dtype=LD):
    """m[n], eta-gradient E[n, C], eta second derivatives D[n, C, C] at coefficients c; x[n_par, n_sets]"""
    x = np.asarray(x, dtype)
    c = np.asarray(c, dtype)
    first, n_coef = layout(forms)
    n_sets = x.shape[1]
    eta = np.full(n_sets, c[0], dtype)
    E = np.zeros((n_sets, n_coef), dtype)
    D = np.zeros((n_sets, n_coef, n_coef), dtype)
    E[:, 0] = 1
    with np.errstate(all="ignore"):
        for p, f in enumerate(forms):
            k, func, grad = HYPERSURFACE_PARAM_FUNCTIONS[f]
            cp = [c[first[p] + i] for i in range(k)]
            eta = eta + func(x[p], *cp)
            E[:, first[p]:first[p] + k] = grad(x[p], *cp)
            d2 = second_derivatives(f, x[p], *cp)
            for a in range(k):
                for b in range(k):
                    D[:, first[p] + a, first[p] + b] = d2[a][b]
        m = np.exp(eta) if log_mode else eta
    return m, E, D


def loss_grad_hess(forms, x, y, sigma, c, log_mode, ips=None, dtype=LD):
    """L, its half-gradient and its exact half-Hessian (J^T J + sum r d2r + prior) over the used sets"""
    y, sigma = np.asarray(y, dtype), np.asarray(sigma, dtype)
    used = sigma != 0
    m, E, D = model(forms, np.asarray(x)[:, used], c, log_mode, dtype)
    c = np.asarray(c, dtype)
    n_coef = c.size
    ips = np.zeros(n_coef, dtype) if ips is None else np.asarray(ips, dtype)
    with np.errstate(all="ignore"):
        r = (m - y[used]) / sigma[used]
        scale = (m if log_mode else np.ones_like(m)) / sigma[used]
        J = scale[:, None] * E
        curv = D + (E[:, :, None] * E[:, None, :] if log_mode else 0)
        loss = np.sum(r * r) + np.sum((ips * c) ** 2)
        g = J.T @ r + ips ** 2 * c
        H = J.T @ J + np.einsum("n,nij->ij", r * scale, curv) + np.diag(ips ** 2)
    return loss, g, H


def loss_only(forms, x, y, sigma, c, log_mode, ips=None):
    return float(loss_grad_hess(forms, x, y, sigma, c, log_mode, ips, np.float64)[0])


def chi2_all(forms, x, y, sigma, c, log_mode):
    """((m - y) / sigma)^2 of EVERY set, plain IEEE division (:982-989)"""
    m = model(forms, x, c, log_mode, np.float64)[0]
    with np.errstate(all="ignore"):
        return ((m - np.asarray(y, np.float64)) / np.asarray(sigma, np.float64)) ** 2


PIVOT_REL, POLISH_MAX, NEWTON_TOL = 1e-13, 8, 1e-14          # HS_PIVOT_REL, HS_POLISH_MAX, HS_NEWTON_TOL


def cholesky(M):
    """lower factor, left-looking as the kernel's; None if a pivot is not positive or is so small a share of its
    diagonal entry (PIVOT_REL) that its sign is rounding's"""
    n = M.shape[0]
    F = np.array(M, np.float64)
    for k in range(n):
        v = F[k:, k] - F[k:, :k] @ F[k, :k]
        if not (v[0] > PIVOT_REL * F[k, k] and v[0] > 0.0 and np.isfinite(v[0])):
            return None
        F[k, k] = np.sqrt(v[0])
        F[k + 1:, k] = v[1:] / F[k, k]
    return np.tril(F)


def lm_fit(forms, x, y, sigma, p0, lo, hi, ips, log_mode, fix_intercept=False, max_iter=200, tol=1e-10):
    """one problem: (coef, cov, loss, n_iter, status); status bits as the library's"""
    from pisa_amd._lib import (HSFIT_NOT_CONVERGED, HSFIT_NOT_FITTED, HSFIT_NOT_POSDEF, HSFIT_UNDERDETERMINED)

    y, sigma = np.asarray(y, np.float64), np.asarray(sigma, np.float64)
    n_coef = len(p0)
    nan_c, nan_cov = np.full(n_coef, np.nan), np.full((n_coef, n_coef), np.nan)
    used = sigma != 0
    if not (np.all(np.isfinite(y[used])) and np.all(np.isfinite(sigma[used]))):
        return nan_c, nan_cov, np.nan, 0, HSFIT_NOT_FITTED
    if used.sum() < n_coef - bool(fix_intercept):
        return nan_c, nan_cov, np.nan, 0, HSFIT_NOT_FITTED | HSFIT_UNDERDETERMINED
    lo, hi, ips = np.asarray(lo, float), np.asarray(hi, float), np.asarray(ips, float)
    c = np.clip(np.asarray(p0, float), lo, hi)

    def lgh(c):
        return tuple(np.asarray(v, np.float64) for v in loss_grad_hess(forms, x, y, sigma, c, log_mode, ips))

    def fixed(c, g):
        f = ((c <= lo) & (g > 0)) | ((c >= hi) & (g < 0))
        f[0] |= bool(fix_intercept)
        return f

    def step(M, g, f, damp=0.0):
        M, b = M.copy(), -g.copy()
        M[f, :] = 0
        M[:, f] = 0
        d = np.diag(M).copy()
        M[np.diag_indices(n_coef)] = np.where(f, 1.0, d + damp * np.maximum(d, 1e-30))
        b[f] = 0
        L = cholesky(M)
        return None if L is None else np.linalg.solve(L.T, np.linalg.solve(L, b))

    L, g, H = lgh(c)
    lam, n_iter, conv = 1e-3, 0, False
    while n_iter < max_iter and not conv:
        n_iter += 1
        f = fixed(c, g)
        d = step(gauss_newton(forms, x, y, sigma, c, log_mode, ips), g, f, lam)
        Lt = np.nan
        if d is not None:
            t = np.where(f, c, np.clip(c + d, lo, hi))
            Lt = loss_only(forms, x, y, sigma, t, log_mode, ips)
        if np.isfinite(Lt) and Lt <= L:
            dec = L - Lt
            c = t
            L, g, H = lgh(c)
            conv = dec <= tol * L and lam <= 1.0      # a tiny step under heavy damping is no stall
            lam = max(lam * 0.1, 1e-12)
        elif np.isfinite(Lt) and Lt - L <= tol * L and lam <= 1.0:
            conv = True
        else:
            lam *= 10.0
            if lam > 1e16:
                break
    polished = False
    if conv:
        for k in range(POLISH_MAX + 1):
            d = step(H, g, fixed(c, g))
            if d is None:
                break
            polished = -(g @ d) <= NEWTON_TOL          # the Newton decrement; d = 0 at the fixed components
            if k == POLISH_MAX:
                break
            t = np.where(fixed(c, g), c, np.clip(c + d, lo, hi))
            Lt = loss_only(forms, x, y, sigma, t, log_mode, ips)
            if not (np.isfinite(Lt) and Lt <= L + 1e-12 * abs(L)):
                break
            c = t
            L, g, H = lgh(c)
            if polished:          # the step the decrement was computed for is the last one
                break
    f = (c <= lo) | (c >= hi)
    f[0] |= bool(fix_intercept)
    M = H.copy()
    M[f, :] = 0
    M[:, f] = 0
    M[f, f] = 1.0
    Lc = cholesky(M)
    # 0: stalled AND stationary by the Newton decrement; a Hessian that is not positive definite has no decrement
    status = 0 if conv and (polished or Lc is None) else HSFIT_NOT_CONVERGED
    if Lc is not None:
        inv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.eye(n_coef)))
        cov = np.where(f[:, None] | f[None, :], 0.0, (inv + inv.T) / 2)
    else:
        cov, status = nan_cov, status | HSFIT_NOT_POSDEF
    return c, cov, L, n_iter, status


def gauss_newton(forms, x, y, sigma, c, log_mode, ips):
    """J^T J + prior: the half-Hessian without the residual-curvature term"""
    y, sigma = np.asarray(y, np.float64), np.asarray(sigma, np.float64)
    used = sigma != 0
    m, E, _ = model(forms, np.asarray(x)[:, used], c, log_mode, np.float64)
    with np.errstate(all="ignore"):
        J = ((m if log_mode else np.ones_like(m)) / sigma[used])[:, None] * E
        return J.T @ J + np.diag(np.asarray(ips, np.float64) ** 2)


def batch_solver(x, forms, y, sigma, p0, lo, hi, inv_prior_sigma, log_mode, fix_intercept, max_iter=200):
    """the restatement in the shape of `pisa_amd.utils.hypersurface.device_batch_solver`: y / sigma
    [n_sets, n_prob] -> dict of numpy arrays coef [n_prob, C], cov [n_prob, C, C], chi2 [n_sets, n_prob],
    loss, n_iter, status [n_prob]"""
    y, sigma = np.asarray(y, np.float64), np.asarray(sigma, np.float64)
    n_sets, n_prob = y.shape
    n_coef = len(p0)
    out = dict(coef=np.empty((n_prob, n_coef)), cov=np.empty((n_prob, n_coef, n_coef)),
               chi2=np.empty((n_sets, n_prob)), loss=np.empty(n_prob), n_iter=np.zeros(n_prob, np.int32),
               status=np.zeros(n_prob, np.int32))
    for k in range(n_prob):
        c, cov, L, it, st = lm_fit(forms, x, y[:, k], sigma[:, k], p0, lo, hi, inv_prior_sigma, log_mode,
                                   fix_intercept, max_iter)
        out["coef"][k], out["cov"][k], out["loss"][k], out["n_iter"][k], out["status"][k] = c, cov, L, it, st
        out["chi2"][:, k] = chi2_all(forms, x, y[:, k], sigma[:, k], c, log_mode)
    return out


# ------------------------------------------------------------------ the two measures
def stationarity(forms, x, y, sigma, c, cov, log_mode, ips=None, free=None):
    """max over the free coefficients of |H^-1 (-g)|_i / sqrt(cov_ii), reference side (longdouble)"""
    _, g, H = loss_grad_hess(forms, x, y, sigma, c, log_mode, ips)
    free = np.ones(len(c), bool) if free is None else np.asarray(free)
    g, H = np.asarray(g[free], np.float64), np.asarray(H[np.ix_(free, free)], np.float64)
    delta = np.linalg.solve(H, -g)
    return float(np.max(np.abs(delta) / np.sqrt(np.diag(np.asarray(cov))[free])))


def cov_reference(forms, x, y, sigma, c, log_mode, ips=None, free=None):
    """inverse of the reference half-Hessian at c (fixed rows / columns zero), from longdouble"""
    _, _, H = loss_grad_hess(forms, x, y, sigma, c, log_mode, ips)
    n = len(c)
    free = np.ones(n, bool) if free is None else np.asarray(free)
    out = np.zeros((n, n))
    out[np.ix_(free, free)] = np.linalg.inv(np.asarray(H[np.ix_(free, free)], np.float64))
    return out


def cov_error(cov, ref, free=None):
    """max |cov - ref| / sqrt(ref_ii ref_jj) over the free block"""
    n = ref.shape[0]
    free = np.ones(n, bool) if free is None else np.asarray(free)
    s = np.sqrt(np.diag(ref)[free])
    return float(np.max(np.abs(np.asarray(cov)[np.ix_(free, free)] - ref[np.ix_(free, free)]) / np.outer(s, s)))


# ------------------------------------------------------------------ seeded inputs
FORMS_A = ("quadratic", "exponential_scaled", "logarithmic")
OFFSETS_A = ([-0.2, -0.1, 0.1, 0.25], [-1.0, -0.5, 0.5, 1.0, 1.5], [-0.6, -0.3, 0.3, 0.6, 0.9, 1.2])


def case_a(n_prob=128, seed=5):
    """log mode, quadratic + exponential_scaled + logarithmic (C = 6), the nominal set at x = 0 and 15
    on-axis sets; sigma = 1 % of y x U(0.5, 2), Gaussian scatter.  Returns x [3, 16], y, sigma [16, n_prob],
    the true coefficients [n_prob, 6]."""
    rs = np.random.RandomState(seed)
    n_sets = 1 + sum(len(o) for o in OFFSETS_A)
    x = np.zeros((3, n_sets))
    k = 1
    for p, offs in enumerate(OFFSETS_A):
        x[p, k:k + len(offs)] = offs
        k += len(offs)
    truth = np.stack([rs.normal(0.0, 0.05, n_prob), rs.normal(0.0, 0.5, n_prob), rs.normal(0.0, 0.5, n_prob),
                      rs.normal(0.0, 0.1, n_prob), rs.normal(0.4, 0.05, n_prob), rs.normal(0.3, 0.1, n_prob)], axis=1)
    y0 = np.stack([model(FORMS_A, x, truth[k], True, np.float64)[0] for k in range(n_prob)], axis=1)
    sigma = 0.01 * y0 * rs.uniform(0.5, 2.0, y0.shape)
    y = y0 + sigma * rs.normal(size=y0.shape)
    return x, y, sigma, truth


FORMS_LIMIT = ("quadratic",) * 7 + ("linear",)


def case_limit(n_prob=5, seed=11, n_sets=70):
    """identity link, seven quadratic and one linear parameter (C = 16), 70 sets: random design"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-1.0, 1.0, (8, n_sets))
    x[:, 0] = 0.0
    truth = np.concatenate([1.0 + rs.normal(0, 0.05, (n_prob, 1)), rs.normal(0, 0.3, (n_prob, 15))], axis=1)
    y0 = np.stack([model(FORMS_LIMIT, x, truth[k], False, np.float64)[0] for k in range(n_prob)], axis=1)
    sigma = 0.02 * rs.uniform(0.5, 2.0, y0.shape)
    y = y0 + sigma * rs.normal(size=y0.shape)
    return x, y, sigma, truth


def free_box(n_coef):
    return np.full(n_coef, -np.inf), np.full(n_coef, np.inf)


# ------------------------------------------------------------------ families
# Each family is a dict: forms, x [n_par, n_sets], y, sigma [n_sets, n_prob], truth [n_prob, C] (or None) and the fit
# arguments p0, lo, hi, ips, log_mode, fix_intercept, max_iter.  `well_posed` says whether tests/test_host_hsfit.py
# holds the restatement to a tenth of the gates on it; the others are the flag families.
import functools
import os

EXACT_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hsfit_exact_ref.npz")
MAX_ITER = 200
ALL_FORMS = tuple(HYPERSURFACE_PARAM_FUNCTIONS)


def family(forms, x, y, sigma, truth, log_mode, p0=None, lo=None, hi=None, ips=None, fix_intercept=False,
           max_iter=MAX_ITER, well_posed=True):
    n_coef = layout(forms)[1]
    box = free_box(n_coef)
    if p0 is None:          # Hypersurface.fit's default start: intercept 0 in log mode, 1 otherwise, the rest 0
        p0 = np.zeros(n_coef)
        p0[0] = 0.0 if log_mode else 1.0
    return dict(forms=tuple(forms), x=np.asarray(x, np.float64), y=np.asarray(y, np.float64),
                sigma=np.asarray(sigma, np.float64), truth=truth, log_mode=bool(log_mode),
                p0=np.asarray(p0, np.float64), lo=box[0] if lo is None else np.asarray(lo, np.float64),
                hi=box[1] if hi is None else np.asarray(hi, np.float64),
                ips=np.zeros(n_coef) if ips is None else np.asarray(ips, np.float64),
                fix_intercept=bool(fix_intercept), max_iter=int(max_iter), well_posed=well_posed)


def solve(fam):
    """the restatement on a family"""
    return batch_solver(fam["x"], fam["forms"], fam["y"], fam["sigma"], fam["p0"], fam["lo"], fam["hi"], fam["ips"],
                        fam["log_mode"], fam["fix_intercept"], fam["max_iter"])


def on_axis(offsets):
    """x [n_par, 1 + sum of len(offsets)]: the nominal set at 0, then every parameter's own sets"""
    x = np.zeros((len(offsets), 1 + sum(len(o) for o in offsets)))
    k = 1
    for p, offs in enumerate(offsets):
        x[p, k:k + len(offs)] = offs
        k += len(offs)
    return x


def scatter(rs, forms, x, truth, log_mode, rel=0.01, floor=1e-4):
    """y, sigma [n_sets, n_prob]: sigma = rel |y0| U(0.5, 2) + floor, Gaussian scatter"""
    y0 = np.stack([model(forms, x, t, log_mode, np.float64)[0] for t in truth], axis=1)
    sigma = rel * np.abs(y0) * rs.uniform(0.5, 2.0, y0.shape) + floor
    return y0 + sigma * rs.normal(size=y0.shape), sigma


OFFSETS_FORMS = ([-1.0, -0.5, 0.5, 1.0], [-0.4, -0.2, 0.2, 0.4])


def _intercepts(rs, n_prob, log_mode):
    return rs.normal(0.0, 0.05, n_prob) + (0.0 if log_mode else 1.0)


def _form_truth(rs, form, n_prob):
    """coefficients of one parameter at which the problem is well posed on x in [-1, 1]"""
    if form == "linear":
        return [rs.normal(0.0, 0.3, n_prob)]
    if form == "quadratic":
        return [rs.normal(0.0, 0.3, n_prob), rs.normal(0.0, 0.3, n_prob)]
    if form == "exponential":
        return [rs.normal(0.0, 0.5, n_prob)]
    if form == "exponential_scaled":        # b away from 0, a away from -1: the valley belongs to f_ill
        return [rs.uniform(-0.4, 0.4, n_prob), rs.choice([-1.0, 1.0], n_prob) * rs.uniform(0.6, 1.2, n_prob)]
    return [np.clip(rs.normal(0.0, 0.3, n_prob), -0.7, 0.7)]          # logarithmic: 1 + m x >= 0.3


@functools.lru_cache(maxsize=None)
def f_forms(form, log_mode, n_prob=64, max_iter=MAX_ITER, p0_all=None):
    """one parameter of `form` and one linear parameter, 9 on-axis sets"""
    rs = np.random.RandomState(100 + 10 * ALL_FORMS.index(form) + int(log_mode))
    forms = (form, "linear")
    x = on_axis(OFFSETS_FORMS)
    truth = np.stack([_intercepts(rs, n_prob, log_mode)] + _form_truth(rs, form, n_prob)
                     + [rs.normal(0.0, 0.3, n_prob)], axis=1)
    y, sigma = scatter(rs, forms, x, truth, log_mode)
    p0 = None if p0_all is None else np.full(truth.shape[1], p0_all)
    return family(forms, x, y, sigma, truth, log_mode, p0=p0, max_iter=max_iter, well_posed=max_iter > 0)


SET_COUNTS = (63, 64, 65, 127, 128)
SETS_VARIANTS = tuple("n%d" % n for n in SET_COUNTS) + ("log65", "unused")
FORMS_SETS_LOG = ("exponential", "quadratic", "linear")


@functools.lru_cache(maxsize=None)
def f_sets(variant, n_prob=8):
    """case_limit's design at the set counts where the lane loops and the chains end; `log65`: log mode with an
    exponential parameter; `unused`: 128 sets, sigma = 0 on sets 63 and 64 of the first half of the problems and on
    the last set of the others (NaN values there: an unused set may hold anything)"""
    if variant == "log65":
        rs = np.random.RandomState(65)
        x = rs.uniform(-1.0, 1.0, (3, 65))
        x[:, 0] = 0.0
        truth = np.stack([rs.normal(0, 0.05, n_prob), rs.normal(0, 0.5, n_prob), rs.normal(0, 0.3, n_prob),
                          rs.normal(0, 0.3, n_prob), rs.normal(0, 0.3, n_prob)], axis=1)
        y, sigma = scatter(rs, FORMS_SETS_LOG, x, truth, True)
        return family(FORMS_SETS_LOG, x, y, sigma, truth, True)
    n_sets = 128 if variant == "unused" else int(variant[1:])
    x, y, sigma, truth = case_limit(n_prob, seed=11 + n_sets, n_sets=n_sets)
    if variant == "unused":
        half = n_prob // 2
        sigma[63:65, :half] = 0.0
        sigma[127, half:] = 0.0
        y[64, :half] = np.nan
        y[127, half:] = np.nan
    return family(FORMS_LIMIT, x, y, sigma, truth, False)


FORMS_MANY = ("linear", "exponential")
MANY_FIRST, MANY_EXTRA, MANY_POOL = 4096, 70, 64
# (index, kind): a workgroup takes problem i and then i + 4096.  Bad first, good second ...
MANY_BAD = tuple((i, k) for i, k in zip(range(0, 24, 2), ("nan", "few", "flat") * 4)) \
    + tuple((i + MANY_FIRST, k) for i, k in zip(range(40, 64, 4), ("nan", "few", "flat") * 2))     # ... and good first


@functools.lru_cache(maxsize=None)
def f_many_pool():
    """the distinct well-posed problems of f_many: log mode, intercept + linear + exponential on 5 sets"""
    rs = np.random.RandomState(4166)
    x = on_axis(([-0.5, 0.5], [-1.0, 1.0]))
    truth = np.stack([rs.normal(0, 0.05, MANY_POOL), rs.normal(0, 0.3, MANY_POOL), rs.normal(0, 0.5, MANY_POOL)],
                     axis=1)
    y, sigma = scatter(rs, FORMS_MANY, x, truth, True)
    return family(FORMS_MANY, x, y, sigma, truth, True)


@functools.lru_cache(maxsize=None)
def f_many():
    """4096 + 70 problems: problem j is problem j % 64 of the pool, except the bad ones of MANY_BAD --
    `nan`: a NaN value in a used set (not fitted); `few`: two used sets for three coefficients (not fitted,
    underdetermined); `flat`: the two sets of the exponential parameter unused, so that its derivative row is zero
    on every used set (fitted; the Hessian is singular: NOT_POSDEF).  Returns the family and `source` [n_prob]:
    the pool index, -1 for the bad ones."""
    pool = f_many_pool()
    n = MANY_FIRST + MANY_EXTRA
    source = np.arange(n) % MANY_POOL
    y, sigma = pool["y"][:, source].copy(), pool["sigma"][:, source].copy()
    for i, kind in MANY_BAD:
        source[i] = -1
        if kind == "nan":
            y[2, i] = np.nan
        elif kind == "few":
            sigma[2:, i] = 0.0
        else:
            sigma[3:, i] = 0.0
    return family(FORMS_MANY, pool["x"], y, sigma, None, True, well_posed=False), source


BOX_VARIANTS = ("lower", "two_sided", "pinned", "outside", "intercept", "leave")


@functools.lru_cache(maxsize=None)
def f_box(variant, n_prob=32):
    """case_a's first problems with a box: `lower` a lower bound that cuts some bins, `two_sided` both sides cut
    some, `pinned` lo == hi, `outside` the start outside the box on two coefficients, `intercept` a bound on the
    intercept, `leave` the start ON a bound the minimum is inside of"""
    x, y, sigma, truth = case_a()
    lo, hi = free_box(6)
    p0 = np.zeros(6)
    if variant == "lower":
        lo[1] = -0.1
    elif variant == "two_sided":
        lo[2], hi[2] = -0.3, 0.3
    elif variant == "pinned":
        lo[3] = hi[3] = 0.05
    elif variant == "outside":
        lo[1], hi[1], p0[1] = -1.0, 0.2, 3.0
        lo[5], hi[5], p0[5] = 0.1, 0.6, -0.5
    elif variant == "intercept":
        hi[0] = 0.0
    else:
        lo[4], p0[4] = 0.25, 0.25
        hi[1], p0[1] = 2.0, 2.0
    return family(FORMS_A, x, y[:, :n_prob].copy(), sigma[:, :n_prob].copy(), truth[:n_prob], True, p0=p0, lo=lo, hi=hi)


FORMS_LIN = ("quadratic", "linear", "linear")
LIN_VARIANTS = ("plain", "prior", "up30", "down30")
LIN_SCALE = dict(plain=1.0, prior=1.0, up30=2.0 ** 30, down30=2.0 ** -30)


@functools.lru_cache(maxsize=None)
def f_lin(variant, n_prob=32):
    """the exact anchor: identity link, linear and quadratic forms only, so a linear weighted least-squares
    problem; 12 sets whose sigma spans three decades; `prior`: prior weights on three coefficients; `up30` /
    `down30`: y and sigma times 2^30 / 2^-30 (the answer scales by the same power of two, exactly)"""
    rs = np.random.RandomState(12)
    x = rs.uniform(-1.0, 1.0, (3, 12))
    x[:, 0] = 0.0
    truth = np.concatenate([1.0 + rs.normal(0, 0.05, (n_prob, 1)), rs.normal(0, 0.3, (n_prob, 4))], axis=1)
    y0 = np.stack([model(FORMS_LIN, x, t, False, np.float64)[0] for t in truth], axis=1)
    sigma = (10.0 ** np.linspace(-4.0, -1.0, 12))[:, None] * rs.uniform(0.8, 1.25, y0.shape)
    y = y0 + sigma * rs.normal(size=y0.shape)
    ips = np.array([0.0, 1 / 0.2, 0.0, 1 / 0.5, 1 / 0.1]) if variant == "prior" else None
    s = LIN_SCALE[variant]
    return family(FORMS_LIN, x, y * s, sigma * s, truth * s, False, ips=ips)


FORMS_EDGE = ("logarithmic", "linear")


@functools.lru_cache(maxsize=None)
def f_log_edge(n_prob=32):
    """the truth next to where the model ends: min over the sets of 1 + m x in [0.03, 0.1]; start at zero"""
    rs = np.random.RandomState(31)
    x = on_axis(OFFSETS_FORMS)
    m = rs.choice([-1.0, 1.0], n_prob) * (1.0 - rs.uniform(0.03, 0.1, n_prob))
    truth = np.stack([rs.normal(0, 0.05, n_prob), m, rs.normal(0, 0.3, n_prob)], axis=1)
    y, sigma = scatter(rs, FORMS_EDGE, x, truth, True)
    return family(FORMS_EDGE, x, y, sigma, truth, True)


FORMS_TWIN = ("linear", "linear")
ILL_NAN = (3, 7, 8)          # the problems of f_ill("nan_start") in which the set the start point has no value at is used
LAMBDA_DECADES = 19          # x10 steps from HS_LAMBDA0 = 1e-3 to HS_LAMBDA_MAX = 1e16


@functools.lru_cache(maxsize=None)
def f_ill(variant, n_prob=16):
    """the flag families.  `twin`: two linear parameters with identical x rows, identity link (singular Hessian,
    the minimum loss unique); `twin_prior`: the same with a prior on both slopes (positive definite again);
    `nan_start`: logarithmic with a start point at which 1 + m x <= 0 on the last set, which is used in the problems
    ILL_NAN only; `valley`: exponential_scaled with the intercept fixed at 0 and flat data at exp(1) on sets
    that all lie at x > 0: the model reaches them only as a step, b -> -inf with a -> -2"""
    rs = np.random.RandomState(900 + len(variant))
    if variant in ("twin", "twin_prior"):
        row = np.array([0.0, -1.0, -0.6, -0.3, 0.3, 0.5, 0.8, 1.0])
        x = np.stack([row, row])
        truth = np.stack([1.0 + rs.normal(0, 0.05, n_prob), rs.normal(0, 0.3, n_prob), rs.normal(0, 0.3, n_prob)], axis=1)
        y, sigma = scatter(rs, FORMS_TWIN, x, truth, False)
        ips = np.array([0.0, 1 / 0.3, 1 / 0.4]) if variant == "twin_prior" else None
        return family(FORMS_TWIN, x, y, sigma, truth, False, ips=ips, well_posed=variant == "twin_prior")
    if variant == "nan_start":
        x = on_axis(([-1.0, -0.5, 0.5, 1.0], [-0.4, -0.2, 0.2, 0.4]))
        x = np.concatenate([x, [[1.5], [0.0]]], axis=1)
        truth = np.stack([rs.normal(0, 0.05, n_prob), rs.uniform(-0.5, -0.3, n_prob), rs.normal(0, 0.3, n_prob)], axis=1)
        y, sigma = scatter(rs, FORMS_EDGE, x, truth, True)
        unused = np.ones(n_prob, bool)
        unused[list(ILL_NAN)] = False
        sigma[-1, unused] = 0.0
        p0 = np.array([0.0, -0.8, 0.0])          # 1 - 0.8 * 1.5 < 0
        return family(FORMS_EDGE, x, y, sigma, truth, True, p0=p0, well_posed=False)
    assert variant == "valley"
    forms = ("exponential_scaled",)
    x = on_axis(([0.25, 0.5, 0.75, 1.0],))[:, 1:]
    truth = np.stack([np.full(n_prob, 1.0), rs.uniform(-0.2, 0.2, n_prob), np.zeros(n_prob)], axis=1)
    y, sigma = scatter(rs, forms, x, truth, True)
    return family(forms, x, y, sigma, truth, True, fix_intercept=True, well_posed=False)


FORMS_SCAN = ("exponential_scaled", "linear")


@functools.lru_cache(maxsize=None)
def scan(log_mode, n_prob=256):
    """exponential_scaled + linear with unconstrained truths: some problems run along the (a + 1) b = const valley"""
    rs = np.random.RandomState(77 + int(log_mode))
    x = on_axis(OFFSETS_FORMS)
    truth = np.stack([_intercepts(rs, n_prob, log_mode), rs.normal(0, 0.5, n_prob), rs.normal(0, 0.5, n_prob),
                      rs.normal(0, 0.3, n_prob)], axis=1)
    y, sigma = scatter(rs, FORMS_SCAN, x, truth, log_mode)
    return family(FORMS_SCAN, x, y, sigma, truth, log_mode, well_posed=False)


MAX_ITER_0 = (("exponential", True), ("logarithmic", False), ("quadratic", True))


def f_no_iter(form, log_mode):
    """f_forms problems with max_iter = 0 from a start point that is not zero: flagged, the start point returned"""
    return f_forms(form, log_mode, 8, 0, 0.1)


def _families():
    out = {}
    for f in ALL_FORMS:
        for lm in (True, False):
            out["forms-%s-%s" % (f, "log" if lm else "identity")] = functools.partial(f_forms, f, lm)
    for v in SETS_VARIANTS:
        out["sets-" + v] = functools.partial(f_sets, v)
    out["many-pool"] = f_many_pool
    for v in BOX_VARIANTS:
        out["box-" + v] = functools.partial(f_box, v)
    for v in LIN_VARIANTS:
        out["lin-" + v] = functools.partial(f_lin, v)
    out["log-edge"] = f_log_edge
    for v in ("twin_prior", "twin", "nan_start", "valley"):
        out["ill-" + v] = functools.partial(f_ill, v)
    for f, lm in MAX_ITER_0:
        out["no-iter-%s-%s" % (f, "log" if lm else "identity")] = functools.partial(f_no_iter, f, lm)
    out["scan-log"] = functools.partial(scan, True)
    out["scan-identity"] = functools.partial(scan, False)
    return out


FAMILIES = _families()
WELL_POSED = tuple(n for n in FAMILIES if n.split("-")[0] in ("forms", "sets", "many", "box", "lin", "log")
                   or n == "ill-twin_prior")


def get(name):
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result on a family, computed once per session"""
    return solve(get(name))


def free_mask(fam, coef):
    """[n_prob, C]: the coefficients that are neither on a bound, nor pinned, nor the fixed intercept"""
    free = (coef > fam["lo"]) & (coef < fam["hi"])
    if fam["fix_intercept"]:
        free[:, 0] = False
    return free


def measures(fam, out, which=None):
    """the worst stationarity and covariance figures of a result over the problems `which` (default: all), on the
    free block of every problem"""
    free = free_mask(fam, out["coef"])
    worst_s = worst_c = 0.0
    for k in (range(fam["y"].shape[1]) if which is None else which):
        args = (fam["forms"], fam["x"], fam["y"][:, k], fam["sigma"][:, k], out["coef"][k])
        worst_s = max(worst_s, stationarity(*args, out["cov"][k], fam["log_mode"], fam["ips"], free[k]))
        ref = cov_reference(*args, fam["log_mode"], fam["ips"], free[k])
        worst_c = max(worst_c, cov_error(out["cov"][k], ref, free[k]))
    return worst_s, worst_c


# the restatement's share of flagged problems (NOT_CONVERGED or NOT_POSDEF) in the scan, measured by
# tests/test_host_hsfit.py: the device may exceed it by two percentage points (paths parting on borderline problems)
SCAN_FLAGGED = {"scan-log": 31 / 256, "scan-identity": 34 / 256}
