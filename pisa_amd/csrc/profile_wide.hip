// profile_wide.hip -- the wide form of the profiled trial ensembles: the fit of profile.hip / profile_bounded.hip for up
// to 32 nuisance displacements per (trial, template) pair ("Profiled trial ensembles: more than 8
// parameters").  The definition and the arithmetic are those of profile_device.hpp; what is new is the mapping:
//
//   one wavefront = one workgroup = one pair.  Its state (eta, the trial point, the step, g, the packed H) lives in
//   LDS, 5.5 KiB at J = 32.  A sweep takes the bins in chunks of 64.  Per chunk (1) the lanes own bins: the data row,
//   E, S2 and the J response rows of the chunk are staged into LDS, each lane forms mu, phi, phi', phi'' of its bin;
//   (2) the lanes own chains: up to 36 lanes a 4 x 4 tile of H each (every response read feeds four products), 8 lanes
//   four entries of g each, one lane Phi, `scale` and the domain flag, each over the chunk's bins in ascending order
//   (one branch-free loop for all lanes: the LDS reads of four bins are in flight together).
//   Factor, substitutions, bound set and clamp are the cooperative phases of profile_wide_device.hpp, between barriers.
//   No floating-point value is reduced across lanes; at J <= 8 the outputs are the bits of profile_kernel.
//
// J and `bounded` are run-time values (the LDS of the response chunk is sized by J at the launch); the kind and the
// output form are template parameters: 8 kernels.  Full output: grid.x = t K + k.  Reduced output: grid.x = t, the
// workgroup walks its range of templates in ascending order (grid.y ranges where the trials are too few to fill the
// device) and profile_join_kernel of profile_kernel.hpp joins the ranges through this file's own buffer.  The checks,
// the split and the launch with its join are `pf_run_any` of profile_kernel.hpp, with a trial as the row unit.
// The kernel's body and `pfw_run` stand in profile_wide_kernel.hpp, with the form of the response as a parameter:
// this file instantiates the linear form, profile_loglinear.hip the log-linear one.
#include "profile_wide_kernel.hpp"

using namespace pisa;

namespace pisa {

// the linear response: `pfw_kernel_body` of profile_wide_kernel.hpp, which profile_loglinear.hip shares
template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(PFW_LANES)
profile_wide_kernel(const PfArgs a, const int J, const int bounded) {
    pfw_kernel_body<KIND, REDUCE, PFW_LINEAR>(a, J, bounded);
}

template <bool REDUCE>
static int pfw_run_linear(int32_t kind, int32_t n_params, int32_t max_iter, int64_t T, int64_t K, int64_t B,
                          const PfArgs &a, void *stream) {
    return pfw_run<REDUCE>(kind, n_params, max_iter, T, K, B, a, stream,
                           [](auto c, const PfArgs &aa, dim3 grid, dim3 block, size_t lds, hipStream_t st, int J,
                              int bounded) {
        hipLaunchKernelGGL((profile_wide_kernel<decltype(c)::value, REDUCE>), grid, block, lds, st, aa, J, bounded);
        PISA_CHECK_LAUNCH("profile_wide_kernel");
        return PISA_HIP_OK;
    });
}

}  // namespace pisa

PISA_API int pisa_hip_profiled_metric_matrix_wide(int32_t kind, const double *d_data, const double *d_expected,
                                                  const double *d_sigma2, const double *d_response,
                                                  int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                  const double *d_center, const double *d_lower, const double *d_upper,
                                                  int64_t bound_stride_k, int32_t n_params, int32_t max_iter,
                                                  int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                                  double *d_value, double *d_eta, int32_t *d_n_iter,
                                                  int32_t *d_pair_status, int32_t *d_status, void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_full(in, d_value, d_eta, d_n_iter, d_pair_status);
    return pfw_run_linear<false>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}

PISA_API int pisa_hip_profiled_metric_matrix_best_wide(int32_t kind, const double *d_data, const double *d_expected,
                                                       const double *d_sigma2, const double *d_response,
                                                       int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                       const double *d_center, const double *d_lower,
                                                       const double *d_upper, int64_t bound_stride_k,
                                                       const double *d_offset, int32_t k0, int32_t n_params,
                                                       int32_t max_iter, int64_t n_trials, int64_t n_templates,
                                                       int64_t n_bins, double *d_best, int32_t *d_arg, double *d_at,
                                                       double *d_eta_best, double *d_eta_at, int32_t *d_trial_status,
                                                       int32_t *d_status, void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status, d_lower, d_upper, bound_stride_k);
    const PfArgs a = pf_args_best(in, d_offset, k0, d_best, d_arg, d_at, d_eta_best, d_eta_at, d_trial_status);
    return pfw_run_linear<true>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}
