// profile.hip -- trial ensembles with linearised nuisance parameters fitted PER (trial, template) pair: for data row t,
// template row k and J <= 8 nuisance displacements eta the template is mu(eta) = E[k] + sum_j R[k][j] eta_j, eta is
// fitted by a damped Newton iteration on Phi (profile_device.hpp: the solver, free of HIP types; DESIGN.md §4,
// "Profiled trial ensembles": the definition) and the reported entry is the metric of ens_direct_kernel (ensemble.hip)
// on the template row mu(eta_hat), prior terms joined.  llh, poisson_llh, chi2, mod_chi2; as a [T][K] matrix with
// eta_hat, iteration counts and status bits per pair, or reduced per trial to (best, arg, at k0) with the two eta.
//
// Mapping.  One lane owns one trial; a workgroup is ONE wavefront: a strip of 64 trials against one template (full
// output: grid = strips x templates, the template index fastest so that the strip's data rows are re-read from L2) or
// against all templates in ascending order (reduced output: grid = strips).  The bins go through LDS 16 at a time:
// the strip's data transposed ([bin][trial], 65 doubles apart: the coalesced global read stores without bank
// conflicts and a lane reads its own column), E / S2 / R of the chunk as wavefront-uniform broadcasts.  Gradient,
// packed Hessian, eta, trial point and step live in registers (J is a template parameter: every loop unrolls).  All
// lanes sweep the bins together; a lane whose pair is done idles until the wavefront's slowest pair is.  One
// wavefront per workgroup instead of four: no wavefront waits for another's slowest pair, the barriers around the
// staging cost nothing, and the reduced form (one workgroup per strip walks all templates) has four times the
// workgroups -- 157 for 10^4 trials instead of 40 on 256 compute units.
//
// Placement: the bits of entry (t, k) depend on row t of D and row k of E / S2 / R / c alone.  Every sum over bins is
// one chain per lane in ascending bin order whatever the chunk; there is no cross-lane reduction and no atomic; the
// reduced form compares the same doubles in ascending k with a strict comparison (the smallest k wins a tie).  Where
// a call has too few strips to fill the device the templates of a strip are split over workgroups in contiguous ranges
// and a second launch joins the ranges in ascending order with the same comparison: whatever the split, the output
// is that of one walk over all templates.  The join buffer is a `DeviceScratch` (common.hpp): reduced-form calls on
// different streams must not overlap.
//
// The kernels and the launch layer live in profile_kernel.hpp, which profile_bounded.hip (eta fitted inside a box)
// includes as well; profile_wide.hip runs its own kernels through the same launch layer.
#include "profile_kernel.hpp"

using namespace pisa;

PISA_API int pisa_hip_profiled_metric_matrix(int32_t kind, const double *d_data, const double *d_expected,
                                             const double *d_sigma2, const double *d_response,
                                             int64_t response_stride_k, const double *d_inv_prior_sigma,
                                             const double *d_center, int32_t n_params, int32_t max_iter,
                                             int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_value,
                                             double *d_eta, int32_t *d_n_iter, int32_t *d_pair_status,
                                             int32_t *d_status, void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status);
    const PfArgs a = pf_args_full(in, d_value, d_eta, d_n_iter, d_pair_status);
    return pf_run<false, false>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}

PISA_API int pisa_hip_profiled_metric_matrix_best(int32_t kind, const double *d_data, const double *d_expected,
                                                  const double *d_sigma2, const double *d_response,
                                                  int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                  const double *d_center, const double *d_offset, int32_t k0,
                                                  int32_t n_params, int32_t max_iter, int64_t n_trials,
                                                  int64_t n_templates, int64_t n_bins, double *d_best, int32_t *d_arg,
                                                  double *d_at, double *d_eta_best, double *d_eta_at,
                                                  int32_t *d_trial_status, int32_t *d_status, void *stream) {
    const PfArgs in = pf_args_in(d_data, d_expected, d_sigma2, d_response, response_stride_k, d_inv_prior_sigma,
                                 d_center, d_status);
    const PfArgs a = pf_args_best(in, d_offset, k0, d_best, d_arg, d_at, d_eta_best, d_eta_at, d_trial_status);
    return pf_run<true, false>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}
