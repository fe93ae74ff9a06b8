// profile_kernel.hpp -- the kernels and the launch layer of the profiled trial ensembles, shared by profile.hip (the
// unbounded entry points) and profile_bounded.hip (eta fitted inside a box per template): one kernel template with a
// BOUNDED flag, instantiated by the file that includes this header for the forms its entry points reach.  What the
// kernel computes, its mapping and its placement rule are described at the top of profile.hip.  The launch layer at the
// end of the file -- the checks (`pf_check`), the filling of `PfArgs` (`pf_args_*`), the split of the reduced form
// (`pf_plan_split`) and the run with its join (`pf_run_any`) -- serves profile_wide.hip's kernels as well, and
// profile_hesse.hip takes the checks from it.
//
// BOUNDED.  The bounds lo / hi of template k ([J] doubles each) are wavefront-uniform: they are staged beside the
// prior weights and the centres in LDS (2 J more doubles, in the bounded instantiations only) and read where they are
// used, never held in registers; the bound set of a step is one bitmask per lane (`pf_bind`, profile_device.hpp).
// Everything else -- the staging of the bins, the sweeps, the reduced output, the split of a strip's templates over
// workgroups and the join -- is the same code, and the unbounded instantiations are what they were before the flag
// existed ("Profiled trial ensembles: bounds").
#pragma once
#include "common.hpp"
#include "ensemble_device.hpp"
#include "profile_device.hpp"

namespace pisa {

static_assert(PF_MAX_PARAMS == PISA_HIP_PROFILE_MAX_PARAMS, "profile_device.hpp and pisa_hip.h disagree");
static_assert(PF_LLH == PISA_HIP_METRIC_LLH && PF_POISSON_LLH == PISA_HIP_METRIC_POISSON_LLH &&
              PF_CHI2 == PISA_HIP_METRIC_CHI2 && PF_MOD_CHI2 == PISA_HIP_METRIC_MOD_CHI2, "metric kinds");
static_assert(PF_NOT_CONVERGED == PISA_HIP_PROFILE_NOT_CONVERGED && PF_BOUNDARY == PISA_HIP_PROFILE_BOUNDARY &&
              PF_NOT_POSDEF == PISA_HIP_PROFILE_NOT_POSDEF && PF_START_OUTSIDE == PISA_HIP_PROFILE_START_OUTSIDE &&
              PF_BAD_BOUNDS == PISA_HIP_PROFILE_BAD_BOUNDS,
              "status bits");

constexpr int PF_LANES = 64;               // one wavefront: a strip of 64 trials
constexpr int PF_BK = 16;                  // bins per chunk
constexpr int PF_LD = PF_LANES + 1;        // doubles between two bins of the transposed data chunk
constexpr int64_t PF_MAX_BLOCKS = (int64_t)1 << 26;   // x 64 lanes = the 2^32 threads a grid may hold
constexpr int PF_MAX_ITER = 4096;          // bound of max_iter: a launch ends after (max_iter + 1) * 41 sweeps at most

struct PfArgs {
    const double *D, *E, *S2, *R, *ips, *center, *offset;
    int64_t r_stride_k;   // doubles between the responses of two templates (0: shared)
    int64_t B;
    int T, K, k0, max_iter;
    double *value, *eta;            // full: [T][K], [T][K][J] (eta may be null)
    int32_t *n_iter, *pair_status;  // full: [T][K] (n_iter may be null)
    double *best, *at, *eta_best, *eta_at;   // reduced: [T], [T], [T][J], [T][J]
    int32_t *arg, *trial_status;    // reduced: [T]
    int32_t *status;
    // reduced output with the templates of a strip split over n_split workgroups (blockIdx.y: templates
    // [y k_chunk, (y + 1) k_chunk)): each writes its range's (best, arg, flags, eta) and profile_join_kernel joins them
    int n_split, k_chunk;
    double *ws_best, *ws_eta;       // [n_split][T], [n_split][T][J]
    int32_t *ws_arg, *ws_st, *ws_st_at;   // [n_split][T], [n_split][T], [T]
    // the bounded form: [K][J] with b_stride_k doubles between templates (0: one [J] block shared); null: no bound
    // on that side
    const double *lower, *upper;
    int64_t b_stride_k;
};

constexpr int PF_FILL_BLOCKS = 2048;       // workgroups of one wavefront that fill 256 CUs x 4 SIMDs twice over
constexpr int PF_MAX_SPLIT = 1024;

// is v better than best?  llh kinds: larger, chi2 kinds: smaller; strict, so that the smaller column keeps a tie; a NaN
// never wins and never holds against a number
template <bool MAXIMISE>
__device__ __forceinline__ bool pf_better(double v, double best, bool first) {
    return first || (MAXIMISE ? v > best : v < best) || (best != best && v == v);
}

// the chunk of bins [c0, c0 + 16): the strip's data transposed, then E, S2 and the J response rows of template k
template <int J, bool WITH_S2>
__device__ __forceinline__ void pf_stage(const PfArgs &a, int64_t t0, int64_t k, int64_t c0, double *sD, double *sT) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
#pragma unroll 2
    for (int i = 0; i < PF_BK; i++) {
        const int idx = tid + PF_LANES * i, r = idx / PF_BK, cc = idx % PF_BK;
        const int64_t b = c0 + cc, tt = t0 + r;
        sD[cc * PF_LD + r] = (b < a.B && tt < a.T) ? a.D[tt * a.B + b] : 0.0;
    }
    for (int idx = tid; idx < (J + 2) * PF_BK; idx += PF_LANES) {
        const int row = idx / PF_BK, cc = idx % PF_BK;
        const int64_t b = c0 + cc;
        double v = 0.0;
        if (b < a.B) {
            if (row == 0)
                v = a.E[k * a.B + b];
            else if (row == 1)
                v = WITH_S2 ? a.S2[k * a.B + b] : 0.0;
            else
                v = a.R[k * a.r_stride_k + (int64_t)(row - 2) * a.B + b];
        }
        sT[idx] = v;
    }
    __syncthreads();
}

// FULL: grid.x = strip * K + k; REDUCE: grid.x = strip, the workgroup walks the templates in ascending order
template <int KIND, int J, bool REDUCE, bool BOUNDED>
__global__ void __launch_bounds__(PF_LANES)
profile_kernel(const PfArgs a) {
    constexpr bool WITH_S2 = KIND == PF_MOD_CHI2;
    constexpr bool MAXIMISE = PfKind<KIND>::is_llh;
    __shared__ double sD[PF_BK * PF_LD];
    __shared__ double sT[(J + 2) * PF_BK];
    const int lane = (int)threadIdx.x;
    const int64_t strip = REDUCE ? (int64_t)blockIdx.x : (int64_t)blockIdx.x / a.K;
    const int64_t t0 = strip * PF_LANES, t = t0 + lane;
    const bool split = REDUCE && a.n_split > 1;
    const int64_t k_begin = REDUCE ? (int64_t)blockIdx.y * a.k_chunk : (int64_t)blockIdx.x % a.K;
    const int64_t k_end = REDUCE ? (k_begin + a.k_chunk < a.K ? k_begin + a.k_chunk : a.K) : k_begin + 1;
    const bool live = t < a.T;
    // where this workgroup's best eta goes: the output row, or its range's row of the join buffer
    double *const eta_best = !REDUCE ? nullptr
                             : split ? a.ws_eta + ((int64_t)blockIdx.y * a.T + t) * J : a.eta_best + t * J;
    // the prior weights and the template's centres (BOUNDED: and its bounds): wavefront-uniform, read from LDS where
    // they are used
    __shared__ double sP[(BOUNDED ? 4 : 2) * J];
    const double *ips = sP, *cen = sP + J;
    const double *lo = BOUNDED ? sP + 2 * J : sP, *hi = BOUNDED ? sP + 3 * J : sP;   // (read by BOUNDED alone)
    double best_v = 0.0, at_v = 0.0;
    int best_k = -1;
    int32_t st_best = 0, st_at = 0;
    bool negative = false;
    for (int64_t k = k_begin; k < k_end; k++) {
        __syncthreads();
        if (lane < J) {
            sP[lane] = a.ips ? a.ips[lane] : 0.0;
            sP[J + lane] = a.center ? a.center[k * J + lane] : 0.0;
            if constexpr (BOUNDED) {
                sP[2 * J + lane] = a.lower ? a.lower[k * a.b_stride_k + lane] : -INFINITY;
                sP[3 * J + lane] = a.upper ? a.upper[k * a.b_stride_k + lane] : INFINITY;
            }
        }
        // (the barrier that opens the first staging below publishes them; the bounded start reads the box at once)
        PfState<J> st;
        if constexpr (BOUNDED) {
            __syncthreads();
            pf_init_bounded<J>(st, lo, hi);
        } else {
            pf_init<J>(st);
        }
        if (!live) st.done = true;
        // ---- the fit: every lane of the wavefront sweeps the bins until the slowest pair is done
        while (__any(!st.done)) {
            const bool run = !st.done;
            if (run) pf_sweep_begin<J>(st);
            for (int64_t c0 = 0; c0 < a.B; c0 += PF_BK) {
                pf_stage<J, WITH_S2>(a, t0, k, c0, sD, sT);
                if (!run) continue;
                const int nb = (int)(a.B - c0 < PF_BK ? a.B - c0 : PF_BK);
#pragma clang loop unroll(disable)
                for (int cc = 0; cc < nb; cc++) {
                    double r[J];
#pragma unroll
                    for (int j = 0; j < J; j++) r[j] = sT[(2 + j) * PF_BK + cc];
                    pf_bin<KIND, J>(st, sD[cc * PF_LD + lane], sT[cc], sT[PF_BK + cc], r);
                }
            }
            if (run) {
                if constexpr (BOUNDED)
                    pf_decide_bounded<KIND, J>(st, ips, cen, lo, hi, a.max_iter);
                else
                    pf_decide<KIND, J>(st, ips, cen, a.max_iter);
            }
        }
        // ---- the metric at the fitted point, as ens_direct_kernel forms it
        PfValue pv;
        pf_value_begin(pv);
        for (int64_t c0 = 0; c0 < a.B; c0 += PF_BK) {
            pf_stage<J, WITH_S2>(a, t0, k, c0, sD, sT);
            const int nb = (int)(a.B - c0 < PF_BK ? a.B - c0 : PF_BK);
#pragma clang loop unroll(disable)
            for (int cc = 0; cc < nb; cc++) {
                double r[J];
#pragma unroll
                for (int j = 0; j < J; j++) r[j] = sT[(2 + j) * PF_BK + cc];
                pf_value_bin<KIND, J>(pv, st.eta, sD[cc * PF_LD + lane], sT[cc], sT[PF_BK + cc], r);
            }
        }
        if (!live) continue;
        const double val = pf_value_end<KIND, J>(pv, st.eta, ips, cen);
        const int32_t pst = pf_status<J>(st);
        if (pv.negative) negative = true;
        if (REDUCE) {
            const double v = a.offset ? val + a.offset[k] : val;
            if (pf_better<MAXIMISE>(v, best_v, best_k < 0)) {
                best_v = v;
                best_k = (int)k;
                st_best = pst;
                // (the row is rewritten whenever a later template is better: the last write is arg's)
#pragma unroll
                for (int j = 0; j < J; j++) eta_best[j] = st.eta[j];
            }
            if ((int)k == a.k0) {
                at_v = v;
                st_at = pst;
                a.at[t] = v;
                if (split) a.ws_st_at[t] = pst;
#pragma unroll
                for (int j = 0; j < J; j++) a.eta_at[t * J + j] = st.eta[j];
            }
        } else {
            const int64_t o = t * a.K + k;
            a.value[o] = val;
            a.pair_status[o] = pst;
            if (a.n_iter) a.n_iter[o] = st.n_iter;
            if (a.eta) {
#pragma unroll
                for (int j = 0; j < J; j++) a.eta[o * J + j] = st.eta[j];
            }
        }
    }
    if (REDUCE && live) {
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
    (void)at_v;
    if (negative) a.status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
}

// joins the ranges of a split reduced launch per trial, in ascending range order with the comparison of the ranges
// themselves: the result is that of one walk over all templates
template <bool MAXIMISE>
__global__ void __launch_bounds__(256)
profile_join_kernel(const PfArgs a, int J) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    double best_v = 0.0;
    int win = -1;
    for (int s = 0; s < a.n_split; s++) {
        const double v = a.ws_best[(int64_t)s * a.T + t];
        if (pf_better<MAXIMISE>(v, best_v, win < 0)) {
            best_v = v;
            win = s;
        }
    }
    const int64_t o = (int64_t)win * a.T + t;
    a.best[t] = best_v;
    a.arg[t] = a.ws_arg[o];
    a.trial_status[t] = a.ws_st[o] | a.ws_st_at[t];
    for (int j = 0; j < J; j++) a.eta_best[t * J + j] = a.ws_eta[o * J + j];
}

// join buffer of the split reduced form: one per file that includes this header, so the bounded, the unbounded and
// the wide entry points share no memory
[[maybe_unused]] static DeviceScratch g_pf_work;   // (profile_hesse.hip has no reduced form)

// ------------------------------------------------------------------------------------------------ the launch layer
// (of profile.hip, profile_bounded.hip and profile_wide.hip; profile_hesse.hip takes `pf_check`)

// What the narrow, bounded, wide and hesse entry points check alike: the kind, 1 <= n_params <= most, the sizes, the
// required inputs, sigma2 for mod_chi2, and both strides: the response of template k begins k * stride doubles in, 0
// (shared by all templates) or whole [J][B] blocks; its bounds (`boxed`) likewise, 0 or whole [J] blocks.
inline bool pf_check(int32_t kind, int32_t n_params, int32_t most, int64_t T, int64_t K, int64_t B, const double *D,
                     const double *E, const double *S2, const double *R, const int32_t *status, int64_t r_stride_k,
                     bool boxed, int64_t b_stride_k) {
    return kind >= PISA_HIP_METRIC_LLH && kind <= PISA_HIP_METRIC_MOD_CHI2 && n_params >= 1 && n_params <= most &&
           ens_check_sizes(T, K, B) && D && E && R && status && (kind != PISA_HIP_METRIC_MOD_CHI2 || S2) &&
           (r_stride_k == 0 || r_stride_k >= (int64_t)n_params * B) &&
           (!boxed || b_stride_k == 0 || b_stride_k >= (int64_t)n_params);
}

// the arguments of an entry point as the kernels take them: the inputs (bounds: null where the form has none) ...
inline PfArgs pf_args_in(const double *D, const double *E, const double *S2, const double *R, int64_t r_stride_k,
                         const double *ips, const double *center, int32_t *status, const double *lower = nullptr,
                         const double *upper = nullptr, int64_t b_stride_k = 0) {
    PfArgs a = {};
    a.D = D, a.E = E, a.S2 = S2, a.R = R, a.r_stride_k = r_stride_k, a.ips = ips, a.center = center;
    a.lower = lower, a.upper = upper, a.b_stride_k = b_stride_k, a.status = status;
    return a;
}

// ... with the full output ...
inline PfArgs pf_args_full(PfArgs a, double *value, double *eta, int32_t *n_iter, int32_t *pair_status) {
    a.value = value, a.eta = eta, a.n_iter = n_iter, a.pair_status = pair_status;
    return a;
}

// ... or the reduced one
inline PfArgs pf_args_best(PfArgs a, const double *offset, int32_t k0, double *best, int32_t *arg, double *at,
                           double *eta_best, double *eta_at, int32_t *trial_status) {
    a.offset = offset, a.k0 = k0;
    a.best = best, a.arg = arg, a.at = at, a.eta_best = eta_best, a.eta_at = eta_at, a.trial_status = trial_status;
    return a;
}

// The split of the reduced form: with fewer row units (strips of the narrow form, trials of the wide one) than `fill`
// workgroups the templates of a unit go to several workgroups, in contiguous ranges that all hold a template; the
// ranges' results go through `work`.
inline int pf_plan_split(PfArgs &a, int64_t units, int64_t fill, int n_params, DeviceScratch &work) {
    const int64_t K = a.K, T = a.T;
    if (units >= fill || K <= 1) return PISA_HIP_OK;
    int64_t want = (fill + units - 1) / units;
    if (want > K) want = K;
    if (want > PF_MAX_SPLIT) want = PF_MAX_SPLIT;
    const int64_t chunk = (K + want - 1) / want;
    const int64_t n_split = (K + chunk - 1) / chunk;
    if (n_split <= 1) return PISA_HIP_OK;
    const int64_t per = n_split * T;               // doubles: best, eta [J], and arg + flags as one more; + T
    double *w;
    const int rc = work.reserve(per * (2 + n_params) + T, &w);
    if (rc != PISA_HIP_OK) return rc;
    a.n_split = (int)n_split;
    a.k_chunk = (int)chunk;
    a.ws_best = w;
    a.ws_eta = w + per;
    a.ws_arg = reinterpret_cast<int32_t *>(w + per * (1 + n_params));
    a.ws_st = a.ws_arg + per;
    a.ws_st_at = a.ws_st + per;
    return PISA_HIP_OK;
}

// One run of a matrix entry point, narrow or wide: the checks, the sizes, the split, the launch of the form's kernel
// (`launch(kind constant, a, grid, stream)`, which returns after PISA_CHECK_LAUNCH) and the join of a split run.
// `rows`: the trials of one row unit of the form (a strip of 64, or 1); full output: a workgroup per (unit, template).
template <bool REDUCE, class L>
static int pf_run_any(int32_t kind, int32_t n_params, int32_t most, int32_t max_iter, int64_t T, int64_t K, int64_t B,
                      int rows, int64_t fill, bool boxed, PfArgs a, void *stream, L launch) {
    if (!pf_check(kind, n_params, most, T, K, B, a.D, a.E, a.S2, a.R, a.status, a.r_stride_k, boxed, a.b_stride_k))
        return PISA_HIP_ERR_INVALID;
    if (max_iter < 0 || max_iter > PF_MAX_ITER) return PISA_HIP_ERR_INVALID;
    if (!ens_check_outputs<REDUCE>(a.value, a.best, a.arg, a.at, a.k0, K)) return PISA_HIP_ERR_INVALID;
    if (REDUCE ? (!a.eta_best || !a.eta_at || !a.trial_status) : !a.pair_status) return PISA_HIP_ERR_INVALID;
    const int64_t units = (T + rows - 1) / rows;
    const int64_t blocks = REDUCE ? units : units * K;
    // (a grid holds at most 2^32 threads: 2^26 workgroups of 64 lanes)
    if (blocks > PF_MAX_BLOCKS) return PISA_HIP_ERR_INVALID;
    a.B = B;
    a.T = (int)T;
    a.K = (int)K;
    a.max_iter = max_iter;
    a.n_split = 1;
    a.k_chunk = (int)K;
    if (REDUCE) {
        const int rc = pf_plan_split(a, units, fill, n_params, g_pf_work);
        if (rc != PISA_HIP_OK) return rc;
    }
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)blocks, (unsigned)a.n_split);
    return dispatch_int<PF_LLH, PF_POISSON_LLH, PF_CHI2, PF_MOD_CHI2>(kind, [&](auto c) {
        const int rc = launch(c, a, grid, st);
        if (rc != PISA_HIP_OK || a.n_split == 1) return rc;
        const unsigned jb = (unsigned)((a.T + 255) / 256);
        hipLaunchKernelGGL((profile_join_kernel<PfKind<decltype(c)::value>::is_llh>), dim3(jb), dim3(256), 0, st, a,
                           n_params);
        PISA_CHECK_LAUNCH("profile_join_kernel");
        return PISA_HIP_OK;
    });
}

// the narrow form: a row unit is a strip of 64 trials, J a template parameter
template <bool REDUCE, bool BOUNDED>
static int pf_run(int32_t kind, int32_t n_params, int32_t max_iter, int64_t T, int64_t K, int64_t B, const PfArgs &a,
                  void *stream) {
    return pf_run_any<REDUCE>(kind, n_params, PISA_HIP_PROFILE_MAX_PARAMS, max_iter, T, K, B, PF_LANES, PF_FILL_BLOCKS,
                              BOUNDED, a, stream, [&](auto c, const PfArgs &aa, dim3 grid, hipStream_t st) {
        return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(n_params, [&](auto j) {
            hipLaunchKernelGGL((profile_kernel<decltype(c)::value, decltype(j)::value, REDUCE, BOUNDED>), grid,
                               dim3(PF_LANES), 0, st, aa);
            PISA_CHECK_LAUNCH("profile_kernel");
            return PISA_HIP_OK;
        });
    });
}

}  // namespace pisa
