"""Shared by tests/test_host_hsfit.py and tests/test_gpu_hsfit.py: a plain numpy restatement of the
hypersurface fit (pisa/utils/hypersurface/hypersurface.py:699-959) and the seeded inputs of the tests.

    eta_n = c_0 + sum_p f_p(x_pn; c_p),  m_n = exp(eta_n) in log mode, eta_n otherwise
    L(c)  = sum_used ((m_n - y_n) / sigma_n)^2 + sum_i (inv_prior_sigma_i c_i)^2          (:847-852)

The first derivatives are the gradient functions of `HYPERSURFACE_PARAM_FUNCTIONS`; the second derivatives
are restated here (and checked against central differences of the first).  The half-gradient and the EXACT
half-Hessian of L are accumulated in np.longdouble; the covariance HESSE estimates with
errordef = LEAST_SQUARES is the inverse of that half-Hessian.  `lm_fit` is a simple Levenberg-Marquardt
with a Newton polish, the solver the host tests hand to `Hypersurface.fit`.
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
        try:
            L = np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return None
        return np.linalg.solve(L.T, np.linalg.solve(L, b))

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
    status = 0 if conv else HSFIT_NOT_CONVERGED
    if conv:
        for _ in range(2):
            d = step(H, g, fixed(c, g))
            if d is None:
                break
            t = np.where(fixed(c, g), c, np.clip(c + d, lo, hi))
            Lt = loss_only(forms, x, y, sigma, t, log_mode, ips)
            if not (np.isfinite(Lt) and Lt <= L + 1e-12 * abs(L)):
                break
            c = t
            L, g, H = lgh(c)
    f = (c <= lo) | (c >= hi)
    f[0] |= bool(fix_intercept)
    M = H.copy()
    M[f, :] = 0
    M[:, f] = 0
    M[f, f] = 1.0
    try:
        Lc = np.linalg.cholesky(M)
        inv = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.eye(n_coef)))
        cov = np.where(f[:, None] | f[None, :], 0.0, (inv + inv.T) / 2)
    except np.linalg.LinAlgError:
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
