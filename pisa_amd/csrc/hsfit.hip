// hsfit.hip -- the per-bin fits of Hypersurface.fit (pisa/utils/hypersurface/hypersurface.py:699-959: one Minuit
// MIGRAD + HESSE per bin on a Python closure) as ONE launch over all bins of all maps.
//   hsfit_kernel   one 64-lane wavefront per problem; a workgroup is one wavefront and takes problems in a
//                  grid-stride loop
// Per problem, in fp64:  eta_n = c_0 + sum_p f_p(x_pn; c_p),  m_n = exp(eta_n) (log mode) or eta_n,
//   L(c) = sum_used ((m_n - y_n) / sigma_n)^2 + sum_i (inv_prior_sigma_i c_i)^2                       (:847-852)
// is minimised by Levenberg-Marquardt on the normal equations (damping on the diagonal, a trial point is taken
// only if its loss is finite and not larger, every trial point projected onto the box of the bounds, the solve
// over the free components only), stopped when the loss has stalled.  Then the EXACT half-Hessian of L
// (J^T J + sum_n r_n d2r_n + prior) is formed at the point and Newton steps are taken with it until the Newton
// decrement -g . d (the loss decrease the quadratic model still promises; its root bounds every |d_i| / sigma_i)
// is at most 1e-14 (that step is still taken), eight steps at the most: status 0 says that this was reached.
// The Cholesky inverse of the Hessian at the final point is the covariance HESSE reports with
// errordef = LEAST_SQUARES.
// Lanes run over the sets for the model, the residuals and the derivative rows; lanes run over the entries of
// the normal matrix / Hessian / gradient, EACH entry one lane's sequential chain over the sets in ascending
// order (as fisher.hip): a result depends on the problem's numbers alone, not on the launch shape or on where
// the problem sits in the batch.  The iteration count varies per problem, i.e. per wavefront: the wavefronts of a
// workgroup could not share a barrier, so a workgroup is ONE wavefront and __syncthreads() is that wavefront's
// own LDS fence.  Every branch around a barrier is taken on values all lanes read from the same LDS word.
#include "common.hpp"

#include <math.h>

namespace pisa {

constexpr int HS_LANES = 64;
constexpr int HS_MAXC = PISA_HIP_HSFIT_MAX_COEFFTS;
constexpr int HS_MAX_BLOCKS = 256 * 16;
constexpr double HS_STALL = 1e-10;       // relative loss decrease below which the fit has stalled
constexpr double HS_LAMBDA0 = 1e-3;
constexpr double HS_LAMBDA_MIN = 1e-12;
constexpr double HS_LAMBDA_MAX = 1e16;
constexpr double HS_LAMBDA_STALL = 1.0;   // a stall counts only if the step was at least half the undamped one
constexpr double HS_DAMP_FLOOR = 1e-30;  // keeps a coefficient whose derivative row is zero at the point in place
constexpr double HS_POLISH_SLACK = 1e-12;
constexpr int HS_POLISH_MAX = 8;          // Newton steps with the exact Hessian
constexpr double HS_NEWTON_TOL = 1e-14;   // Newton decrement -g . d at which a point counts as stationary
constexpr double HS_PIVOT_REL = 1e-13;    // a pivot below this share of its diagonal entry is rounding: singular

struct HsDesign {
    int32_t form[HS_MAXC];    // per parameter
    int32_t first[HS_MAXC];   // per parameter: index of its first coefficient
    int32_t owner[HS_MAXC];   // per coefficient: its parameter, -1 for the intercept
    double p0[HS_MAXC], lo[HS_MAXC], hi[HS_MAXC], ips[HS_MAXC];
};

__host__ __device__ inline int hs_ncoef(int form) {
    return (form == PISA_HIP_HSFIT_QUADRATIC || form == PISA_HIP_HSFIT_EXPONENTIAL_SCALED) ? 2 : 1;
}

// f(x; a, b) and its derivatives d0, d1 wrt the coefficients (hypersurface.py:81-205)
__device__ __forceinline__ double hs_form(int form, double x, double a, double b, double &d0, double &d1) {
    d1 = 0.0;
    switch (form) {
    case PISA_HIP_HSFIT_LINEAR:
        d0 = x;
        return a * x;
    case PISA_HIP_HSFIT_QUADRATIC: {
        const double x2 = x * x;
        d0 = x;
        d1 = x2;
        return a * x + b * x2;
    }
    case PISA_HIP_HSFIT_EXPONENTIAL: {
        const double e = exp(a * x);
        d0 = x * e;
        return e - 1.0;
    }
    case PISA_HIP_HSFIT_EXPONENTIAL_SCALED: {
        const double e = exp(b * x);
        d0 = e - 1.0;
        d1 = (a + 1.0) * x * e;
        return (a + 1.0) * (e - 1.0);
    }
    default: {   // logarithmic: outside 1 + m x > 0 the point is not a point of the model
        const double t = 1.0 + a * x;
        if (!(t > 0.0)) {
            d0 = NAN;
            return NAN;
        }
        d0 = x / t;
        return log(t);
    }
    }
}

// second derivative wrt the coefficients k <= l of one parameter
__device__ __forceinline__ double hs_form_d2(int form, int k, int l, double x, double a, double b) {
    switch (form) {
    case PISA_HIP_HSFIT_EXPONENTIAL:
        return x * x * exp(a * x);
    case PISA_HIP_HSFIT_EXPONENTIAL_SCALED: {
        if (l == 0) return 0.0;
        const double e = exp(b * x);
        return k == 0 ? x * e : (a + 1.0) * x * x * e;
    }
    case PISA_HIP_HSFIT_LOGARITHMIC: {
        const double t = 1.0 + a * x;
        return -(x * x) / (t * t);
    }
    default:
        return 0.0;
    }
}

struct HsLds {
    double *x, *y, *sig, *m, *r, *u, *E;   // [n_par][n_sets], 5 x [n_sets], [n_coef][n_sets]
    double *A, *F, *B;                     // [n_coef][n_coef]: normal matrix / Hessian, its factor, the inverse
    double *g, *c, *t, *d, *s;             // [n_coef] x 4, scalars
    int32_t *fix;                          // [n_coef]
};

// model, scaled residual r, derivative scale u and eta's derivative rows E at coefficients cv (in LDS);
// returns the loss (one lane's chain over the sets in ascending order)
__device__ double hs_eval(const HsDesign &ds, const HsLds &s, const double *cv, int n_par, int n_sets, int n_coef,
                          int log_mode) {
    const int lane = threadIdx.x;
    for (int n = lane; n < n_sets; n += HS_LANES) {
        // an unused set (sigma = 0) takes no part: zero residual, zero scale and a ZERO derivative row, so that a
        // NaN or inf its model value may have at a point the used sets accept never meets a 0 * in a chain
        const double sg = s.sig[n];
        const bool used = sg != 0.0;
        double eta = cv[0];
        s.E[n] = used ? 1.0 : 0.0;
        for (int p = 0; p < n_par; p++) {
            const int f = ds.first[p], form = ds.form[p];
            const double a = cv[f], b = hs_ncoef(form) == 2 ? cv[f + 1] : 0.0;
            double d0, d1;
            eta += hs_form(form, s.x[p * n_sets + n], a, b, d0, d1);
            s.E[f * n_sets + n] = used ? d0 : 0.0;
            if (hs_ncoef(form) == 2) s.E[(f + 1) * n_sets + n] = used ? d1 : 0.0;
        }
        const double m = log_mode ? exp(eta) : eta;
        s.m[n] = m;
        s.r[n] = used ? (m - s.y[n]) / sg : 0.0;
        s.u[n] = used ? (log_mode ? m : 1.0) / sg : 0.0;
    }
    __syncthreads();
    if (lane == 0) {
        double L = 0.0;
        for (int n = 0; n < n_sets; n++) L += s.r[n] * s.r[n];
        for (int i = 0; i < n_coef; i++) {
            const double t = ds.ips[i] * cv[i];
            L += t * t;
        }
        s.s[0] = L;
    }
    __syncthreads();
    return s.s[0];
}

// A = J^T J (+ the residual-curvature term if `exact`) + prior, g = J^T r + prior c, at the point of the last hs_eval
__device__ void hs_normal(const HsDesign &ds, const HsLds &s, const double *cv, int n_sets, int n_coef, int log_mode,
                          bool exact) {
    const int n_pairs = n_coef * (n_coef + 1) / 2;
    for (int q = threadIdx.x; q < n_pairs + n_coef; q += HS_LANES) {
        double a = 0.0;
        if (q < n_pairs) {
            int i = 0, rem = q;
            while (rem >= n_coef - i) {
                rem -= n_coef - i;
                i++;
            }
            const int j = i + rem;
            const double *Ei = s.E + i * n_sets, *Ej = s.E + j * n_sets;
            const int p = ds.owner[i];
            const bool curved = exact && p >= 0 && p == ds.owner[j] && ds.form[p] != PISA_HIP_HSFIT_LINEAR &&
                                ds.form[p] != PISA_HIP_HSFIT_QUADRATIC;
            const int f = p >= 0 ? ds.first[p] : 0;
            for (int n = 0; n < n_sets; n++) {
                const double un = s.u[n];
                a += (un * Ei[n]) * (un * Ej[n]);
                if (exact && un != 0.0) {   // un = 0: an unused set (or a model value of 0, whose terms are 0)
                    const double k = s.r[n] * un;
                    if (log_mode) a += k * (Ei[n] * Ej[n]);
                    if (curved) {
                        const double cb = hs_ncoef(ds.form[p]) == 2 ? cv[f + 1] : 0.0;
                        a += k * hs_form_d2(ds.form[p], i - f, j - f, s.x[p * n_sets + n], cv[f], cb);
                    }
                }
            }
            if (i == j) a += ds.ips[i] * ds.ips[i];
            s.A[i * n_coef + j] = a;
            s.A[j * n_coef + i] = a;
        } else {
            const int i = q - n_pairs;
            const double *Ei = s.E + i * n_sets;
            for (int n = 0; n < n_sets; n++) a += (s.u[n] * Ei[n]) * s.r[n];
            a += (ds.ips[i] * ds.ips[i]) * cv[i];
            s.g[i] = a;
        }
    }
    __syncthreads();
}

// F = A with the rows and columns of the fixed components replaced by the identity and `lambda` times the
// diagonal added; d = -g (0 at the fixed components).  Then F = its lower Cholesky factor (left-looking, lanes
// over the rows of a column).  False if a pivot is not positive, or so small a share of the diagonal entry it
// is what is left of (HS_PIVOT_REL) that its sign is rounding's: the matrix of two identical derivative rows
// would otherwise pass as positive definite in one problem out of a few.
__device__ bool hs_factor(const HsLds &s, int n_coef, double lambda) {
    const int lane = threadIdx.x;
    for (int q = lane; q < n_coef * n_coef; q += HS_LANES) {
        const int i = q / n_coef, j = q % n_coef;
        double v = s.A[q];
        if (s.fix[i] || s.fix[j]) v = i == j ? 1.0 : 0.0;
        else if (i == j) v += lambda * fmax(v, HS_DAMP_FLOOR);
        s.F[q] = v;
    }
    if (lane < n_coef) s.d[lane] = s.fix[lane] ? 0.0 : -s.g[lane];
    __syncthreads();
    for (int k = 0; k < n_coef; k++) {
        double v = 0.0;
        const bool mine = lane >= k && lane < n_coef;
        if (mine) {
            v = s.F[lane * n_coef + k];
            for (int m = 0; m < k; m++) v -= s.F[lane * n_coef + m] * s.F[k * n_coef + m];
        }
        const double piv = __shfl(v, k), diag = __shfl(mine ? s.F[lane * n_coef + k] : 0.0, k);
        if (!(piv > HS_PIVOT_REL * diag) || !(piv > 0.0) || !isfinite(piv)) return false;   // every lane has the same piv
        const double lkk = sqrt(piv);
        if (mine) s.F[lane * n_coef + k] = lane == k ? lkk : v / lkk;
        __syncthreads();
    }
    return true;
}

// solves F F^T z = b in place for `n_cols` right-hand sides b[i * stride + col]: one lane per column
__device__ void hs_solve(const HsLds &s, double *b, int stride, int n_cols, int n_coef) {
    const int col = threadIdx.x;
    if (col < n_cols) {
        for (int i = 0; i < n_coef; i++) {
            double v = b[i * stride + col];
            for (int m = 0; m < i; m++) v -= s.F[i * n_coef + m] * b[m * stride + col];
            b[i * stride + col] = v / s.F[i * n_coef + i];
        }
        for (int i = n_coef - 1; i >= 0; i--) {
            double v = b[i * stride + col];
            for (int m = i + 1; m < n_coef; m++) v -= s.F[m * n_coef + i] * b[m * stride + col];
            b[i * stride + col] = v / s.F[i * n_coef + i];
        }
    }
    __syncthreads();
}

// fixed components of a step: the fixed intercept, and a coefficient on a bound whose descent direction leaves the box
__device__ void hs_active(const HsDesign &ds, const HsLds &s, int n_coef, int fix_intercept) {
    const int i = threadIdx.x;
    if (i < n_coef) {
        const double c = s.c[i], g = s.g[i];
        s.fix[i] = (i == 0 && fix_intercept) || (c <= ds.lo[i] && g > 0.0) || (c >= ds.hi[i] && g < 0.0);
    }
    __syncthreads();
}

// t = the projection of c + d onto the box
__device__ void hs_trial(const HsDesign &ds, const HsLds &s, int n_coef) {
    const int i = threadIdx.x;
    if (i < n_coef) s.t[i] = s.fix[i] ? s.c[i] : fmin(fmax(s.c[i] + s.d[i], ds.lo[i]), ds.hi[i]);
    __syncthreads();
}

__device__ void hs_take(const HsLds &s, int n_coef) {
    if ((int)threadIdx.x < n_coef) s.c[threadIdx.x] = s.t[threadIdx.x];
    __syncthreads();
}

__global__ void __launch_bounds__(HS_LANES)
hsfit_kernel(HsDesign ds, const double *__restrict__ x, const double *__restrict__ y,
             const double *__restrict__ sigma, int n_par, int n_sets, int n_coef, int64_t n_prob, int log_mode,
             int fix_intercept, int max_iter, double *__restrict__ coef, double *__restrict__ cov,
             double *__restrict__ chi2, double *__restrict__ loss, int32_t *__restrict__ n_iter,
             int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    HsLds s;
    s.x = s_lds;
    s.y = s.x + n_par * n_sets;
    s.sig = s.y + n_sets;
    s.m = s.sig + n_sets;
    s.r = s.m + n_sets;
    s.u = s.r + n_sets;
    s.E = s.u + n_sets;
    s.A = s.E + n_coef * n_sets;
    s.F = s.A + n_coef * n_coef;
    s.B = s.F + n_coef * n_coef;
    s.g = s.B + n_coef * n_coef;
    s.c = s.g + n_coef;
    s.t = s.c + n_coef;
    s.d = s.t + n_coef;
    s.s = s.d + n_coef;
    s.fix = (int32_t *)(s.s + 2);
    const int lane = threadIdx.x;
    const int cc = n_coef * n_coef;
    for (int q = lane; q < n_par * n_sets; q += HS_LANES) s.x[q] = x[q];

    for (int64_t prob = blockIdx.x; prob < n_prob; prob += gridDim.x) {
        __syncthreads();
        for (int n = lane; n < n_sets; n += HS_LANES) {
            s.y[n] = y[(int64_t)n * n_prob + prob];
            s.sig[n] = sigma[(int64_t)n * n_prob + prob];
        }
        if (lane < n_coef) s.c[lane] = fmin(fmax(ds.p0[lane], ds.lo[lane]), ds.hi[lane]);
        __syncthreads();
        // every lane counts the same words: the branches below are uniform
        int n_used = 0, bad = 0;
        for (int n = 0; n < n_sets; n++) {
            if (s.sig[n] != 0.0) {
                n_used++;
                if (!isfinite(s.y[n]) || !isfinite(s.sig[n])) bad = 1;
            }
        }
        int st = 0;
        if (bad) st = PISA_HIP_HSFIT_NOT_FITTED;
        else if (n_used < n_coef - (fix_intercept ? 1 : 0)) st = PISA_HIP_HSFIT_NOT_FITTED | PISA_HIP_HSFIT_UNDERDETERMINED;
        if (st) {
            for (int q = lane; q < n_coef; q += HS_LANES) coef[prob * n_coef + q] = NAN;
            for (int q = lane; q < cc; q += HS_LANES) cov[prob * cc + q] = NAN;
            for (int n = lane; n < n_sets; n += HS_LANES) chi2[(int64_t)n * n_prob + prob] = NAN;
            if (lane == 0) {
                loss[prob] = NAN;
                n_iter[prob] = 0;
                status[prob] = st;
            }
            continue;
        }

        double L = hs_eval(ds, s, s.c, n_par, n_sets, n_coef, log_mode);
        hs_normal(ds, s, s.c, n_sets, n_coef, log_mode, false);
        double lambda = HS_LAMBDA0;
        int it = 0;
        bool conv = false;
        while (it < max_iter && !conv) {
            it++;
            hs_active(ds, s, n_coef, fix_intercept);
            double Lt = NAN;
            if (hs_factor(s, n_coef, lambda)) {
                hs_solve(s, s.d, 1, 1, n_coef);
                hs_trial(ds, s, n_coef);
                Lt = hs_eval(ds, s, s.t, n_par, n_sets, n_coef, log_mode);
            } else {
                __syncthreads();
            }
            if (isfinite(Lt) && Lt <= L) {
                const double dec = L - Lt;
                hs_take(s, n_coef);
                L = Lt;
                hs_normal(ds, s, s.c, n_sets, n_coef, log_mode, false);
                // a small decrease after a run of refusals (lambda large, the step tiny) is no stall: go on
                conv = dec <= HS_STALL * L && lambda <= HS_LAMBDA_STALL;
                lambda = fmax(lambda * 0.1, HS_LAMBDA_MIN);
            } else if (isfinite(Lt) && Lt - L <= HS_STALL * L && lambda <= HS_LAMBDA_STALL) {
                conv = true;   // the trial point is no better, and no worse than the stall bound either
            } else {
                lambda *= 10.0;
                if (lambda > HS_LAMBDA_MAX) break;
            }
        }

        // the exact half-Hessian at the point; Newton steps with it until the Newton decrement says the point is
        // stationary (`polished`), then the Hessian once more at the final point
        L = hs_eval(ds, s, s.c, n_par, n_sets, n_coef, log_mode);
        hs_normal(ds, s, s.c, n_sets, n_coef, log_mode, true);
        bool polished = false;
        for (int k = 0; k <= HS_POLISH_MAX && conv; k++) {
            hs_active(ds, s, n_coef, fix_intercept);
            if (!hs_factor(s, n_coef, 0.0)) {
                __syncthreads();
                break;
            }
            hs_solve(s, s.d, 1, 1, n_coef);
            if (lane == 0) {
                double nu2 = 0.0;
                for (int i = 0; i < n_coef; i++) nu2 -= s.g[i] * s.d[i];   // d = 0 at the fixed components
                s.s[1] = nu2;
            }
            __syncthreads();
            polished = s.s[1] <= HS_NEWTON_TOL;
            if (k == HS_POLISH_MAX) break;
            hs_trial(ds, s, n_coef);
            const double Lt = hs_eval(ds, s, s.t, n_par, n_sets, n_coef, log_mode);
            const bool ok = isfinite(Lt) && Lt <= L + HS_POLISH_SLACK * fabs(L);
            if (ok) {
                hs_take(s, n_coef);
                L = Lt;
            } else {
                L = hs_eval(ds, s, s.c, n_par, n_sets, n_coef, log_mode);   // E, r, u back at c
            }
            hs_normal(ds, s, s.c, n_sets, n_coef, log_mode, true);
            if (!ok || polished) break;   // the step the decrement was computed for is the last one
        }
        // covariance: the fixed intercept and every coefficient that ended on a bound have zero rows and columns
        if (lane < n_coef)
            s.fix[lane] = (lane == 0 && fix_intercept) || s.c[lane] <= ds.lo[lane] || s.c[lane] >= ds.hi[lane];
        __syncthreads();
        const bool pd = hs_factor(s, n_coef, 0.0);
        if (pd) {
            for (int q = lane; q < cc; q += HS_LANES) s.B[q] = (q / n_coef == q % n_coef) ? 1.0 : 0.0;
            __syncthreads();
            hs_solve(s, s.B, n_coef, n_coef, n_coef);
        } else {
            __syncthreads();
        }
        // 0: stalled AND stationary by the Newton decrement.  A Hessian that is not positive definite has no
        // decrement: the flag for it stands alone if the descent had stalled
        st = conv && (polished || !pd) ? 0 : PISA_HIP_HSFIT_NOT_CONVERGED;
        if (!pd) st |= PISA_HIP_HSFIT_NOT_POSDEF;
        for (int q = lane; q < cc; q += HS_LANES) {
            const int i = q / n_coef, j = q % n_coef;
            double v = NAN;
            if (pd) v = (s.fix[i] || s.fix[j]) ? 0.0 : s.B[i <= j ? q : j * n_coef + i];   // exactly symmetric
            cov[prob * cc + q] = v;
        }
        for (int q = lane; q < n_coef; q += HS_LANES) coef[prob * n_coef + q] = s.c[q];
        // chi2 of EVERY set, plain IEEE division (:982-989)
        for (int n = lane; n < n_sets; n += HS_LANES) {
            const double q = (s.m[n] - s.y[n]) / s.sig[n];
            chi2[(int64_t)n * n_prob + prob] = q * q;
        }
        if (lane == 0) {
            loss[prob] = L;
            n_iter[prob] = it;
            status[prob] = st;
        }
    }
}

inline size_t hs_lds_bytes(int n_par, int n_sets, int n_coef) {
    const size_t doubles = (size_t)n_par * n_sets + 5 * (size_t)n_sets + (size_t)n_coef * n_sets +
                           3 * (size_t)n_coef * n_coef + 4 * (size_t)n_coef + 2;
    return doubles * 8 + (size_t)n_coef * 4;
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_hypersurface_fit(const double *h_x, const int32_t *h_form, int32_t n_par, int32_t n_sets,
                                       int64_t n_prob, const double *d_y, const double *d_sigma,
                                       const double *h_p0, const double *h_lo, const double *h_hi,
                                       const double *h_inv_prior_sigma, int32_t n_coef, int32_t log_mode,
                                       int32_t fix_intercept, int32_t max_iter, double *d_x, double *d_coef,
                                       double *d_cov, double *d_chi2, double *d_loss, int32_t *d_n_iter,
                                       int32_t *d_status, void *stream) {
    if (!h_x || !h_form || !d_y || !d_sigma || !h_p0 || !h_lo || !h_hi || !h_inv_prior_sigma || !d_x || !d_coef ||
        !d_cov || !d_chi2 || !d_loss || !d_n_iter || !d_status)
        return PISA_HIP_ERR_INVALID;
    if (n_par < 1 || n_par > PISA_HIP_HSFIT_MAX_COEFFTS - 1) return PISA_HIP_ERR_INVALID;
    if (n_sets < 1 || n_sets > PISA_HIP_HSFIT_MAX_SETS) return PISA_HIP_ERR_INVALID;
    if (n_prob < 1 || n_prob > 0x7FFFFFFF || max_iter < 0) return PISA_HIP_ERR_INVALID;
    HsDesign ds;
    for (int i = 0; i < HS_MAXC; i++) {
        ds.form[i] = ds.first[i] = 0;
        ds.owner[i] = -1;
        ds.p0[i] = ds.lo[i] = ds.hi[i] = ds.ips[i] = 0.0;
    }
    int n = 1;
    for (int p = 0; p < n_par; p++) {
        if (h_form[p] < PISA_HIP_HSFIT_LINEAR || h_form[p] > PISA_HIP_HSFIT_LOGARITHMIC) return PISA_HIP_ERR_INVALID;
        ds.form[p] = h_form[p];
        ds.first[p] = n;
        for (int k = 0; k < hs_ncoef(h_form[p]); k++, n++) {
            if (n >= PISA_HIP_HSFIT_MAX_COEFFTS) return PISA_HIP_ERR_INVALID;
            ds.owner[n] = p;
        }
    }
    if (n != n_coef) return PISA_HIP_ERR_INVALID;
    for (int i = 0; i < n_coef; i++) {
        // -inf / +inf: no bound; a NaN anywhere, lo > hi, a start point or a prior weight that is not finite: refused
        if (!isfinite(h_p0[i]) || !isfinite(h_inv_prior_sigma[i]) || h_inv_prior_sigma[i] < 0.0) return PISA_HIP_ERR_INVALID;
        if (!(h_lo[i] <= h_hi[i]) || h_lo[i] == INFINITY || h_hi[i] == -INFINITY) return PISA_HIP_ERR_INVALID;
        ds.p0[i] = h_p0[i];
        ds.lo[i] = h_lo[i];
        ds.hi[i] = h_hi[i];
        ds.ips[i] = h_inv_prior_sigma[i];
    }
    for (int q = 0; q < n_par * n_sets; q++)
        if (!isfinite(h_x[q])) return PISA_HIP_ERR_INVALID;
    // the largest index, n_sets * n_prob <= 2^7 * 2^31 and n_prob * n_coef^2 <= 2^31 * 2^8, is far inside int64
    hipStream_t s = as_stream(stream);
    PISA_TRY_HIP(hipMemcpyAsync(d_x, h_x, (size_t)n_par * n_sets * sizeof(double), hipMemcpyHostToDevice, s));
    const unsigned blocks = (unsigned)(n_prob < HS_MAX_BLOCKS ? n_prob : HS_MAX_BLOCKS);
    hipLaunchKernelGGL(hsfit_kernel, dim3(blocks), dim3(HS_LANES), hs_lds_bytes(n_par, n_sets, n_coef), s, ds, d_x,
                       d_y, d_sigma, (int)n_par, (int)n_sets, (int)n_coef, n_prob, (int)log_mode, (int)fix_intercept,
                       (int)max_iter, d_coef, d_cov, d_chi2, d_loss, d_n_iter, d_status);
    PISA_CHECK_LAUNCH("hsfit_kernel");
    return PISA_HIP_OK;
}
