// profile_bounded.hip -- the profiled trial ensembles of profile.hip with every nuisance displacement fitted inside its
// range: eta_hat = argmin Phi(eta) over lo[k][j] <= eta_j <= hi[k][j] on the domain of profile.hip (DESIGN.md §4,
// "Profiled trial ensembles: bounds").  The solver is the damped Newton iteration of profile_device.hpp with a
// projected step: the start and every trial point are held inside the box by comparisons, and after each accepted
// sweep the coordinates that sit on a bound with the gradient pointing out of the box leave the Newton system
// (`pf_bind`).  Phi is convex, so the constrained minimum is unique wherever the unconstrained one is.  A template
// whose box has a bound with lo > hi or a NaN gives pairs flagged _BAD_BOUNDS that take no step.
//
// The kernel is profile_kernel of profile_kernel.hpp with BOUNDED set: the mapping, the staging, the placement rule,
// the reduced output and its split over workgroups are those of profile.hip.  The 64 bounded instantiations live in
// this file so that the two files compile side by side.
#include "profile_kernel.hpp"

using namespace pisa;

PISA_API int pisa_hip_profiled_metric_matrix_bounded(int32_t kind, const double *d_data, const double *d_expected,
                                                     const double *d_sigma2, const double *d_response,
                                                     int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                     const double *d_center, const double *d_lower,
                                                     const double *d_upper, int64_t bound_stride_k, int32_t n_params,
                                                     int32_t max_iter, int64_t n_trials, int64_t n_templates,
                                                     int64_t n_bins, double *d_value, double *d_eta,
                                                     int32_t *d_n_iter, int32_t *d_pair_status, int32_t *d_status,
                                                     void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_full(in, d_value, d_eta, d_n_iter, d_pair_status);
    return pf_run<false, true>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}

PISA_API int pisa_hip_profiled_metric_matrix_best_bounded(int32_t kind, const double *d_data, const double *d_expected,
                                                          const double *d_sigma2, const double *d_response,
                                                          int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                          const double *d_center, const double *d_lower,
                                                          const double *d_upper, int64_t bound_stride_k,
                                                          const double *d_offset, int32_t k0, int32_t n_params,
                                                          int32_t max_iter, int64_t n_trials, int64_t n_templates,
                                                          int64_t n_bins, double *d_best, int32_t *d_arg, double *d_at,
                                                          double *d_eta_best, double *d_eta_at,
                                                          int32_t *d_trial_status, int32_t *d_status, void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_best(in, d_offset, k0, d_best, d_arg, d_at, d_eta_best, d_eta_at, d_trial_status);
    return pf_run<true, true>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}
