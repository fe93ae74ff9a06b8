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
#include "profile_kernel.hpp"
#include "profile_wide_device.hpp"

using namespace pisa;

static_assert(PFW_MAX_PARAMS == PISA_HIP_PROFILE_WIDE_MAX_PARAMS, "profile_wide_device.hpp and pisa_hip.h disagree");
static_assert(sizeof(PfwShared) % sizeof(double) == 0, "the response chunk follows the state");

namespace pisa {

constexpr int PFW_FILL_BLOCKS = 4096;      // workgroups of one wavefront that give 256 CUs x 4 SIMDs four each

struct PfwDevice {
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f((int)threadIdx.x);
        __syncthreads();
    }
};

// the chunk of bins [c0, c0 + 64) of data row t and template row k: lane cc takes bin c0 + cc
template <bool WITH_S2>
__device__ __forceinline__ void pfw_stage(const PfArgs &a, PfwShared &S, double *R, int J, int64_t t, int64_t k,
                                          int64_t c0, int lane) {
    const int64_t b = c0 + lane;
    const bool in = b < a.B;
    S.cD[lane] = in ? a.D[t * a.B + b] : 0.0;
    S.cE[lane] = in ? a.E[k * a.B + b] : 0.0;
    S.cS2[lane] = (WITH_S2 && in) ? a.S2[k * a.B + b] : 0.0;
    const double *r = a.R + k * a.r_stride_k + b;
    for (int j = 0; j < J; j++) R[j * PFW_LD + lane] = in ? r[(int64_t)j * a.B] : 0.0;
}

template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(PFW_LANES)
profile_wide_kernel(const PfArgs a, const int J, const int bounded) {
    constexpr bool WITH_S2 = KIND == PF_MOD_CHI2;
    constexpr bool MAXIMISE = PfKind<KIND>::is_llh;
    extern __shared__ double pfw_lds[];
    PfwShared &S = *reinterpret_cast<PfwShared *>(pfw_lds);
    double *const R = pfw_lds + sizeof(PfwShared) / sizeof(double);
    PfwDevice x;
    const int lane = (int)threadIdx.x;
    const int64_t t = REDUCE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / a.K;
    const bool split = REDUCE && a.n_split > 1;
    const int64_t k_begin = REDUCE ? (int64_t)blockIdx.y * a.k_chunk : (int64_t)blockIdx.x % a.K;
    const int64_t k_end = REDUCE ? (k_begin + a.k_chunk < a.K ? k_begin + a.k_chunk : a.K) : k_begin + 1;
    double *const eta_best = !REDUCE ? nullptr
                             : split ? a.ws_eta + ((int64_t)blockIdx.y * a.T + t) * J : a.eta_best + t * J;
    // the rows of the response chunk past J, which the tiles read, stay zero
    for (int j = J; j < pfw_padded(J); j++) R[j * PFW_LD + lane] = 0.0;
    double best_v = 0.0;
    int best_k = -1;
    int32_t st_best = 0, st_at = 0;
    bool negative = false;
    for (int64_t k = k_begin; k < k_end; k++) {
        __syncthreads();
        x.each([&](int l) {
            if (l >= J) return;
            S.ips[l] = a.ips ? a.ips[l] : 0.0;
            S.cen[l] = a.center ? a.center[k * J + l] : 0.0;
            S.lo[l] = a.lower ? a.lower[k * a.b_stride_k + l] : -INFINITY;
            S.hi[l] = a.upper ? a.upper[k * a.b_stride_k + l] : INFINITY;
        });
        pfw_init(S, x, J, bounded != 0, true);
        // ---- the fit
        while (!S.done) {
            x.each([&](int l) { pfw_sweep_begin(S, l); });
            for (int64_t c0 = 0; c0 < a.B; c0 += PFW_CHUNK) {
                const int nb = (int)(a.B - c0 < PFW_CHUNK ? a.B - c0 : PFW_CHUNK);
                x.each([&](int l) { pfw_stage<WITH_S2>(a, S, R, J, t, k, c0, l); });
                x.each([&](int l) { pfw_bins<KIND>(S, R, l, nb); });
                x.each([&](int l) { pfw_chains(S, R, l, nb); });
            }
            pfw_decide<KIND>(S, x, a.max_iter);
        }
        // ---- the metric at the fitted point, as ens_direct_kernel forms it
        x.each([&](int l) { pfw_value_begin(S, l); });
        for (int64_t c0 = 0; c0 < a.B; c0 += PFW_CHUNK) {
            const int nb = (int)(a.B - c0 < PFW_CHUNK ? a.B - c0 : PFW_CHUNK);
            x.each([&](int l) { pfw_stage<WITH_S2>(a, S, R, J, t, k, c0, l); });
            x.each([&](int l) { pfw_value_bins<KIND>(S, R, l, nb); });
            x.each([&](int l) { pfw_value_chain(S, l, nb); });
        }
        x.each([&](int l) { pfw_value_end<KIND>(S, l); });
        const double val = S.value;
        const int32_t pst = pfw_status(S);
        if (S.negative) negative = true;
        if (REDUCE) {
            const double v = a.offset ? val + a.offset[k] : val;
            if (pf_better<MAXIMISE>(v, best_v, best_k < 0)) {
                best_v = v;
                best_k = (int)k;
                st_best = pst;
                if (lane < J) eta_best[lane] = S.eta[lane];
            }
            if ((int)k == a.k0) {
                st_at = pst;
                if (lane == 0) {
                    a.at[t] = v;
                    if (split) a.ws_st_at[t] = pst;
                }
                if (lane < J) a.eta_at[t * J + lane] = S.eta[lane];
            }
        } else {
            const int64_t o = t * a.K + k;
            if (lane == 0) {
                a.value[o] = val;
                a.pair_status[o] = pst;
                if (a.n_iter) a.n_iter[o] = S.n_iter;
            }
            if (a.eta && lane < J) a.eta[o * J + lane] = S.eta[lane];
        }
    }
    if (lane != 0) return;
    if (REDUCE) {
        if (split) {
            const int64_t o = (int64_t)blockIdx.y * a.T + t;
            a.ws_best[o] = best_v;
            a.ws_arg[o] = best_k;
            a.ws_st[o] = st_best;
        } else {
            a.best[t] = best_v;
            a.arg[t] = best_k;
            a.trial_status[t] = st_best | st_at;
        }
    }
    if (negative) a.status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
}

// a row unit is one trial; J and `bounded` are run-time values, the response chunk's LDS is sized by J here
template <bool REDUCE>
static int pfw_run(int32_t kind, int32_t n_params, int32_t max_iter, int64_t T, int64_t K, int64_t B, const PfArgs &a,
                   void *stream) {
    const int bounded = a.lower || a.upper;
    return pf_run_any<REDUCE>(kind, n_params, PISA_HIP_PROFILE_WIDE_MAX_PARAMS, max_iter, T, K, B, 1, PFW_FILL_BLOCKS,
                              bounded, a, stream, [&](auto c, const PfArgs &aa, dim3 grid, hipStream_t st) {
        const size_t lds = sizeof(PfwShared) + (size_t)pfw_chunk_doubles(n_params) * sizeof(double);
        hipLaunchKernelGGL((profile_wide_kernel<decltype(c)::value, REDUCE>), grid, dim3(PFW_LANES), lds, st, aa,
                           n_params, bounded);
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
    return pfw_run<false>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
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
    return pfw_run<true>(kind, n_params, max_iter, n_trials, n_templates, n_bins, a, stream);
}
