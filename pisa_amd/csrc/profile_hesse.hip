// profile_hesse.hip -- the covariance of the fitted nuisance displacements of a profiled trial ensemble: for trial t,
// its template k_t and a point eta[t] (normally what pisa_hip_profiled_metric_matrix_best returned at that template),
// ONE sweep of `pf_bin` over the bins in ascending order forms gradient and Hessian of Phi exactly as the solver of
// profile.hip does, the prior terms join, the bound set of the bounded form leaves the system, and the free block is
// inverted: cov = c H^-1 (`pf_hesse_begin`, `pf_hesse_end`, `pf_inverse` of profile_device.hpp; DESIGN.md §4,
// "Profiled trial ensembles: covariance and pulls"; restated in tests/hesse_cases.py).  With it an analysis forms the
// pulls (eta_hat - eta_true) / sigma_hat of an ensemble, the closure check of a profiled fit.
// One lane per trial, a workgroup is one wavefront, as in profile_kernel.hpp -- but the template differs from lane to
// lane (k_t is the fit's `arg`, or one k0 for all), so nothing is staged through LDS: a lane reads its own data row,
// its template's row and responses straight from memory.  That is one sweep against the fit's five or so times K
// templates: the simple form is the right one here.  The bits of row t depend on row t of D, row k_t of E / S2 / R /
// center / bounds and eta[t] alone.  The entry point's checks are `pf_check` of profile_kernel.hpp, the fit's own.
#include "profile_kernel.hpp"   // (the checks of the launch layer: `pf_check`)

namespace pisa {

static_assert(PF_MAX_PARAMS == PISA_HIP_PROFILE_MAX_PARAMS && PF_HELD == PISA_HIP_PROFILE_HELD &&
                  PF_NOT_POSDEF == PISA_HIP_PROFILE_NOT_POSDEF && PF_START_OUTSIDE == PISA_HIP_PROFILE_START_OUTSIDE &&
                  PF_BAD_BOUNDS == PISA_HIP_PROFILE_BAD_BOUNDS,
              "profile_device.hpp and pisa_hip.h disagree");

constexpr int PH_LANES = 64;
constexpr int64_t PH_MAX_BLOCKS = (int64_t)1 << 26;

struct PhArgs {
    const double *D, *E, *S2, *R, *ips, *center, *lower, *upper, *eta;
    const int32_t *k_of_trial;   // null: every trial takes k0
    int64_t r_stride_k, b_stride_k, B;
    int T, K, k0;
    double *cov;                 // [T][J][J]
    int32_t *trial_status, *status;
};

template <int KIND, int J>
__global__ void __launch_bounds__(PH_LANES)
hesse_kernel(const PhArgs a) {
    const int64_t t = (int64_t)blockIdx.x * PH_LANES + threadIdx.x;
    if (t >= a.T) return;
    double *const out = a.cov + t * (J * J);
    const int64_t k = a.k_of_trial ? (int64_t)a.k_of_trial[t] : (int64_t)a.k0;
    int32_t status = 0;
    double cov[J * (J + 1) / 2];
    if (k < 0 || k >= a.K) {   // (no row to read: the call is refused, the row is NaN)
        a.status[0] = PISA_HIP_ERR_INVALID;
        status = -1;
    } else {
        PfState<J> st;
        bool ok;
        {
            double eta[J], lo[J], hi[J];
            const bool boxed = a.lower || a.upper;
#pragma unroll
            for (int j = 0; j < J; j++) {
                eta[j] = a.eta[t * J + j];
                lo[j] = a.lower ? a.lower[k * a.b_stride_k + j] : -INFINITY;
                hi[j] = a.upper ? a.upper[k * a.b_stride_k + j] : INFINITY;
            }
            ok = pf_hesse_begin<J>(st, eta, lo, hi, boxed);
        }
        if (!ok) {
            status = PF_BAD_BOUNDS;
        } else {
            const double *const D = a.D + t * a.B, *const E = a.E + k * a.B, *const R = a.R + k * a.r_stride_k;
            const double *const S2 = KIND == PF_MOD_CHI2 ? a.S2 + k * a.B : nullptr;
            bool negative = false;
#pragma clang loop unroll(disable)
            for (int64_t b = 0; b < a.B; b++) {
                double r[J];
#pragma unroll
                for (int j = 0; j < J; j++) r[j] = R[j * a.B + b];
                const double d = D[b], e = E[b];
                if (d < 0.0 || e < 0.0) negative = true;   // (a NaN compares false; an infinite one takes no part)
                pf_bin<KIND, J>(st, d, e, KIND == PF_MOD_CHI2 ? S2[b] : 0.0, r);
            }
            if (negative) a.status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
            double ips[J], c[J];
#pragma unroll
            for (int j = 0; j < J; j++) {
                ips[j] = a.ips ? a.ips[j] : 0.0;
                c[j] = a.center ? a.center[k * J + j] : 0.0;
            }
            status = pf_hesse_end<KIND, J>(st, ips, c, cov);
        }
    }
    const bool none = status & ~PF_HELD;   // a flag other than HELD: no covariance
#pragma unroll
    for (int i = 0; i < J; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const double v = none ? NAN : cov[pf_at(i, j)];
            out[i * J + j] = v;
            out[j * J + i] = v;   // (one double for both: symmetric bit for bit)
        }
    }
    a.trial_status[t] = status;
}

template <int KIND, int J>
static int hesse_launch(const PhArgs &a, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL((hesse_kernel<KIND, J>), dim3(blocks), dim3(PH_LANES), 0, stream, a);
    PISA_CHECK_LAUNCH("hesse_kernel");
    return PISA_HIP_OK;
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_profiled_hesse(int32_t kind, const double *d_data, const double *d_expected,
                                     const double *d_sigma2, const double *d_response, int64_t response_stride_k,
                                     const double *d_inv_prior_sigma, const double *d_center, const double *d_lower,
                                     const double *d_upper, int64_t bound_stride_k, int32_t n_params,
                                     int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                     const int32_t *d_k_of_trial, int32_t k0, const double *d_eta, double *d_cov,
                                     int32_t *d_trial_status, int32_t *d_status, void *stream) {
    if (!pf_check(kind, n_params, PISA_HIP_PROFILE_MAX_PARAMS, n_trials, n_templates, n_bins, d_data, d_expected,
                  d_sigma2, d_response, d_status, response_stride_k, d_lower || d_upper, bound_stride_k))
        return PISA_HIP_ERR_INVALID;
    if (!d_eta || !d_cov || !d_trial_status) return PISA_HIP_ERR_INVALID;
    if (!d_k_of_trial && (k0 < 0 || k0 >= n_templates)) return PISA_HIP_ERR_INVALID;
    const int64_t blocks = (n_trials + PH_LANES - 1) / PH_LANES;
    if (blocks > PH_MAX_BLOCKS) return PISA_HIP_ERR_INVALID;
    PhArgs a{};
    a.D = d_data;
    a.E = d_expected;
    a.S2 = d_sigma2;
    a.R = d_response;
    a.ips = d_inv_prior_sigma;
    a.center = d_center;
    a.lower = d_lower;
    a.upper = d_upper;
    a.eta = d_eta;
    a.k_of_trial = d_k_of_trial;
    a.r_stride_k = response_stride_k;
    a.b_stride_k = bound_stride_k;
    a.B = n_bins;
    a.T = (int)n_trials;
    a.K = (int)n_templates;
    a.k0 = k0;
    a.cov = d_cov;
    a.trial_status = d_trial_status;
    a.status = d_status;
    hipStream_t st = as_stream(stream);
    return dispatch_int<PF_LLH, PF_POISSON_LLH, PF_CHI2, PF_MOD_CHI2>(kind, [&](auto c) {
        return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(n_params, [&](auto j) {
            return hesse_launch<decltype(c)::value, decltype(j)::value>(a, (unsigned)blocks, st);
        });
    });
}
