// profile_wide_kernel.hpp -- the body of the wide kernels of the profiled trial ensembles and their launch, shared by
// profile_wide.hip (the linear response) and profile_loglinear.hip (the log-linear one).  The mapping -- one wavefront =
// one workgroup = one pair, the state in LDS, the bins in chunks of 64, lanes owning bins and then chains -- is
// described at the top of profile_wide.hip; the form of the response (`PFW_LINEAR`, `PFW_LOGLINEAR` of
// profile_wide_device.hpp) is a template parameter that reaches the two phases whose lanes own bins and nothing else.
// Each file that includes this header declares its own `__global__` kernels around `pfw_kernel_body` and has its own
// join buffer (`g_pf_work` of profile_kernel.hpp).
#pragma once
#include "profile_kernel.hpp"
#include "profile_wide_device.hpp"

namespace pisa {

static_assert(PFW_MAX_PARAMS == PISA_HIP_PROFILE_WIDE_MAX_PARAMS, "profile_wide_device.hpp and pisa_hip.h disagree");
static_assert(sizeof(PfwShared) % sizeof(double) == 0, "the response chunk follows the state");
static_assert(PFW_LINEAR == PISA_HIP_RESPONSE_LINEAR && PFW_LOGLINEAR == PISA_HIP_RESPONSE_LOGLINEAR, "response forms");

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

// one workgroup of a wide kernel; its dynamic LDS holds the state, then the response chunk
template <int KIND, bool REDUCE, int FORM>
__device__ __forceinline__ void pfw_kernel_body(const PfArgs a, const int J, const int bounded) {
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
                x.each([&](int l) { pfw_bins<KIND, FORM>(S, R, l, nb); });
                x.each([&](int l) { pfw_chains(S, R, l, nb); });
            }
            pfw_decide<KIND>(S, x, a.max_iter);
        }
        // ---- the metric at the fitted point, as ens_direct_kernel forms it
        x.each([&](int l) { pfw_value_begin(S, l); });
        for (int64_t c0 = 0; c0 < a.B; c0 += PFW_CHUNK) {
            const int nb = (int)(a.B - c0 < PFW_CHUNK ? a.B - c0 : PFW_CHUNK);
            x.each([&](int l) { pfw_stage<WITH_S2>(a, S, R, J, t, k, c0, l); });
            x.each([&](int l) { pfw_value_bins<KIND, FORM>(S, R, l, nb); });
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

// A row unit is one trial; J and `bounded` are run-time values, the response chunk's LDS is sized by J here.
// `launch(kind constant, a, grid, block, lds bytes, stream, J, bounded)` starts the including file's kernel of that kind.
template <bool REDUCE, class L>
static int pfw_run(int32_t kind, int32_t n_params, int32_t max_iter, int64_t T, int64_t K, int64_t B, const PfArgs &a,
                   void *stream, L launch) {
    const int bounded = a.lower || a.upper;
    return pf_run_any<REDUCE>(kind, n_params, PISA_HIP_PROFILE_WIDE_MAX_PARAMS, max_iter, T, K, B, 1, PFW_FILL_BLOCKS,
                              bounded, a, stream, [&](auto c, const PfArgs &aa, dim3 grid, hipStream_t st) {
        const size_t lds = sizeof(PfwShared) + (size_t)pfw_chunk_doubles(n_params) * sizeof(double);
        return launch(c, aa, grid, dim3(PFW_LANES), lds, st, (int)n_params, bounded);
    });
}

}  // namespace pisa
