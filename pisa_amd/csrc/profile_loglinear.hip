// profile_loglinear.hip -- the profiled trial ensembles with a log-linear (multiplicative) nuisance response (DESIGN.md
// §4, "Profiled trial ensembles: the log-linear response"):
//
//     mu_b(eta) = E_b exp( rho_0b eta_0 + ... + rho_(J-1)b eta_(J-1) )
//
// for 1 to 32 displacements per (trial, template) pair.  The solver is the wide one (profile_wide.hip,
// profile_wide_device.hpp): one wavefront per pair, the state in LDS sized by J, the same chains, factor,
// substitutions, bound set, damping, stop rule and statuses.  What differs is what a lane that owns a bin hands to the
// chains (`pfw_bins_loglinear`: p1 = phi' mu, p2 = phi'' mu^2 + phi' mu) and the template the reported metric is taken
// at (`pfw_mu_loglinear`), so the kernels here are `pfw_kernel_body` of profile_wide_kernel.hpp with the form
// PFW_LOGLINEAR: four kinds x full / reduced output.  The reduced form with few trials splits the templates over
// workgroups and joins them with profile_join_kernel through this file's own buffer.
//
// The two entry points take the form as an argument; with the form linear they are the calls of profile_wide.hip's.
#include "profile_wide_kernel.hpp"

using namespace pisa;

namespace pisa {

template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(PFW_LANES)
profile_loglinear_kernel(const PfArgs a, const int J, const int bounded) {
    pfw_kernel_body<KIND, REDUCE, PFW_LOGLINEAR>(a, J, bounded);
}

template <bool REDUCE>
static int pfw_run_loglinear(int32_t kind, int32_t n_params, int32_t max_iter, int64_t T, int64_t K, int64_t B,
                             const PfArgs &a, void *stream) {
    return pfw_run<REDUCE>(kind, n_params, max_iter, T, K, B, a, stream,
                           [](auto c, const PfArgs &aa, dim3 grid, dim3 block, size_t lds, hipStream_t st, int J,
                              int bounded) {
        hipLaunchKernelGGL((profile_loglinear_kernel<decltype(c)::value, REDUCE>), grid, block, lds, st, aa, J,
                           bounded);
        PISA_CHECK_LAUNCH("profile_loglinear_kernel");
        return PISA_HIP_OK;
    });
}

}  // namespace pisa

PISA_API int pisa_hip_profiled_metric_matrix_wide_form(int32_t kind, int32_t form, const double *d_data,
                                                       const double *d_expected, const double *d_sigma2,
                                                       const double *d_response, int64_t response_stride_k,
                                                       const double *d_inv_prior_sigma, const double *d_center,
                                                       const double *d_lower, const double *d_upper,
                                                       int64_t bound_stride_k, int32_t n_params, int32_t max_iter,
                                                       int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                                       double *d_value, double *d_eta, int32_t *d_n_iter,
                                                       int32_t *d_pair_status, int32_t *d_status, void *stream) {
    if (form == PISA_HIP_RESPONSE_LINEAR)
        return pisa_hip_profiled_metric_matrix_wide(kind, d_data, d_expected, d_sigma2, d_response, response_stride_k,
                                                    d_inv_prior_sigma, d_center, d_lower, d_upper, bound_stride_k,
                                                    n_params, max_iter, n_trials, n_templates, n_bins, d_value, d_eta,
                                                    d_n_iter, d_pair_status, d_status, stream);
    if (form != PISA_HIP_RESPONSE_LOGLINEAR) return PISA_HIP_ERR_INVALID;
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_full(in, d_value, d_eta, d_n_iter, d_pair_status);
    return pfw_run_loglinear<false>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}

PISA_API int pisa_hip_profiled_metric_matrix_best_wide_form(int32_t kind, int32_t form, const double *d_data,
                                                            const double *d_expected, const double *d_sigma2,
                                                            const double *d_response, int64_t response_stride_k,
                                                            const double *d_inv_prior_sigma, const double *d_center,
                                                            const double *d_lower, const double *d_upper,
                                                            int64_t bound_stride_k, const double *d_offset, int32_t k0,
                                                            int32_t n_params, int32_t max_iter, int64_t n_trials,
                                                            int64_t n_templates, int64_t n_bins, double *d_best,
                                                            int32_t *d_arg, double *d_at, double *d_eta_best,
                                                            double *d_eta_at, int32_t *d_trial_status,
                                                            int32_t *d_status, void *stream) {
    if (form == PISA_HIP_RESPONSE_LINEAR)
        return pisa_hip_profiled_metric_matrix_best_wide(kind, d_data, d_expected, d_sigma2, d_response,
                                                         response_stride_k, d_inv_prior_sigma, d_center, d_lower,
                                                         d_upper, bound_stride_k, d_offset, k0, n_params, max_iter,
                                                         n_trials, n_templates, n_bins, d_best, d_arg, d_at,
                                                         d_eta_best, d_eta_at, d_trial_status, d_status, stream);
    if (form != PISA_HIP_RESPONSE_LOGLINEAR) return PISA_HIP_ERR_INVALID;
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_best(in, d_offset, k0, d_best, d_arg, d_at, d_eta_best, d_eta_at, d_trial_status);
    return pfw_run_loglinear<true>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}
