// ensemble_mc.hip -- the metrics that account for finite MC statistics in the trial-ensemble matrix:
//     M[t][k] = nansum_b w(kind; D[t][b], E[k][b], S2[k][b])
// for correct_chi2, mcllh_mean, mcllh_eff and conv_llh, w the per-bin formula of `metric_bin_wide`
// (metric_flux.hip; stats.py:328-596, 697-730, likelihood_functions.py:22-63) with every rule kept, as a
// [n_trials][n_templates] matrix or reduced per trial to (best, arg, value at a given column).
//
// What the batch form does not repeat per pair.  One preparation launch (`emc_prep_kernel`) writes, per template bin
// and per data bin, everything that depends on that row alone:
//   correct_chi2   template: lam = max(E, SMALL_POS), tv = S2 + lam, ln tv             pair: (d - lam)^2 / tv + ln tv
//   mcllh_*        template, S2 > 0: alpha = lam^2 / S2 + a, c0 = alpha ln beta - lgamma(alpha), log1p(beta)
//                  template, S2 == 0 (the mixture's Poisson branch): ln lam, lam
//                  data: lgamma(d + 1)
//                  pair: ((c0 + lgamma(d + alpha)) - lgamma(d + 1)) - (d + alpha) log1p(beta): ONE lgamma
//   conv_llh       template: the normalisation sum of the 101 Gaussian weights, n1(mu) = exp(log_poisson(mu, mu)),
//                  conv_poisson(mu, mu, s), -ln s - ln(2 pi) / 2 and s = max(sqrt(S2), SMALL_POS)
//                  data: lgamma(max(d, SMALL_POS) + 1) and ln max(SMALL_POS, n1(d))
//                  per workgroup and bin, in LDS: L_j = ln(x_j + mu) and q_j = c_y(x_j) - (x_j + mu) of the 101
//                  half-step-shifted nodes of each of the tile's 16 templates (a node with x_j + mu <= 0 is closed:
//                  L_j = 0, q_j = -inf, its term exp(-inf) = 0 -- f_x ascends, so the open nodes are those from the
//                  first positive f_x on), shared by the tile's 16 trials
//                  pair: conv = sum_j exp((d L_j + q_j) - lgamma(d + 1)), 101 x (mul, add, sub, exp, add), then
//                  ln max(SMALL_POS, conv / norm * n1(mu) / conv_poisson(mu, mu, s)) - ln max(SMALL_POS, n1(d))
// conv_llh's second term is norm_conv_poisson(d, d, s) = conv_poisson(d, d, s) n1(d) / conv_poisson(d, d, s): on the
// real numbers n1(d), the NaN of 0 ln 0 at d = 0 (which max(SMALL_POS, .) turns into SMALL_POS, as it does the NaN
// of n1(0) on the template side at mu = 0).  The kernel uses that identity, so the term costs nothing per pair; it
// differs from the quotient as written by that quotient's own two roundings.
//
// What is guaranteed, as in ensemble.hip: the bits of entry (t, k) depend on row t of D and row k of E / S2 only.
// A prepared value is a function of its own bin, a node table of its own (mu, s); every sum over bins is ONE chain
// per lane in ascending bin order with the rounding errors kept (`ens_two_sum`, ensemble_device.hpp)
// and added last; no atomic touches the result and no pair's bins are split over lanes.  The full and the reduced
// output are those of every kernel in which a lane owns a pair (`EnsOut`, ensemble_device.hpp).
#include "common.hpp"
#include "ensemble_device.hpp"
#include "metric_device.hpp"

#include <math.h>

namespace pisa {

constexpr int EMC_THREADS = 256;
// 16 trials x 16 templates per workgroup; the cheap kinds stage 64 bins per chunk, rows 65 doubles apart (ensemble.hip)
constexpr int EMC_TILE = 16;
constexpr int EMC_BK = 64;
constexpr int EMC_LD = EMC_BK + 1;
constexpr int EMC_NODES = 2 * (50 + 1) - 1;      // stats.py:494-503
constexpr int EMC_PLANES_CHEAP = 3;
constexpr int EMC_PLANES_CONV = 5;

__device__ __forceinline__ double emc_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool emc_finite(double x) { return x - x == 0.0; }

// node j of conv_poisson's grid over +-3 s, shifted by half a step (stats.py:494-503), and its Gaussian log-weight
// from c0 = -ln s - ln(2 pi) / 2
__device__ __forceinline__ void emc_node(int j, double s, double c0, double &x, double &cy) {
    const double start = -3 * s, stop = 3 * s;
    const double step = (stop - start) / EMC_NODES;
    const double shift = 3 * s / (double)EMC_NODES;
    x = (j * step + start) + shift;
    cy = c0 - x * x / (2 * (s * s));
}

__device__ __forceinline__ double emc_log_poisson(double k, double l) { return k * log(l) - l - lgamma(k + 1); }

// conv_poisson(l, l, s) as written (stats.py:479-527) and the normalisation sum, for the preparation
__device__ double emc_conv_self(double l, double s, double c0, double &norm) {
    const double k = l;
    const double lg = lgamma(k + 1);
    double conv = 0.0;
    norm = 0.0;
    bool open_ = false;
    for (int j = 0; j < EMC_NODES; j++) {
        double x, cy;
        emc_node(j, s, c0, x, cy);
        norm += exp(cy);
        const double fx = x + l;
        open_ = open_ || fx > 0;
        if (open_) {
            double fy = k * log(fx) - fx - lg;
            if (fy != fy) fy = 0.0;
            conv += exp(cy + fy);
        }
    }
    return conv / norm;
}

// ----------------------------------------------------------------------------------------------- preparation
// element i < K B: template bin (k, b) -> planes P[p][k][b]; element K B <= i < (K + T) B: data bin -> planes G[p][t][b]
template <int KIND>
__global__ void __launch_bounds__(EMC_THREADS)
emc_prep_kernel(const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ S2,
                int64_t n_tb, int64_t n_kb, double *__restrict__ P, double *__restrict__ G,
                int32_t *__restrict__ status) {
    constexpr bool MIX = KIND == PISA_HIP_METRIC_MCLLH_MEAN || KIND == PISA_HIP_METRIC_MCLLH_EFF;
    constexpr bool CONV = KIND == PISA_HIP_METRIC_CONV_LLH;
    const int64_t i = (int64_t)blockIdx.x * EMC_THREADS + threadIdx.x;
    bool negative = false;
    if (i < n_kb) {
        const double e = E[i], s2 = S2[i];
        const bool finite = emc_finite(e);
        if (s2 < 0.0 || (MIX && e < 0.0)) negative = true;
        const double lam = e < SMALL_POS ? SMALL_POS : e;
        double p0, p1, p2;
        if (KIND == PISA_HIP_METRIC_CORRECT_CHI2) {
            const double tv = s2 + lam;
            p0 = lam;
            p1 = tv;
            p2 = log(tv);
        } else if (MIX) {
            const double a = KIND == PISA_HIP_METRIC_MCLLH_EFF ? 1.0 : 0.0;
            if (s2 < 0) {                       // (lam <= 0 cannot be after the clip)
                p0 = -2.0;
                p1 = p2 = 0.0;
            } else if (s2 == 0) {
                p0 = -1.0;
                p1 = log(lam);
                p2 = lam;
            } else {
                const double alpha = (lam * lam) / s2 + a;
                const double beta = lam / s2 + 0.0;
                p0 = alpha;
                p1 = alpha * log(beta) - lgamma(alpha);
                p2 = log1p(beta);
            }
        } else {
            const double sq = sqrt(s2);
            const double s = sq > SMALL_POS ? sq : SMALL_POS;          // Python's max(SMALL_POS, x): NaN -> SMALL_POS
            const double lc = e > SMALL_POS ? e : SMALL_POS;
            const double c0 = -log(s) - 0.5 * log(2 * 3.141592653589793);
            double norm;
            const double n2 = emc_conv_self(lc, s, c0, norm);
            p0 = norm;
            p1 = exp(emc_log_poisson(e, e));    // the raw expectation: NaN at 0 (0 ln 0)
            p2 = n2;
            P[3 * n_kb + i] = c0;
            P[4 * n_kb + i] = s;
        }
        P[i] = finite ? p0 : emc_nan();
        P[n_kb + i] = p1;
        P[2 * n_kb + i] = p2;
    } else if (i - n_kb < n_tb) {
        const int64_t o = i - n_kb;
        const double d = D[o];
        if (MIX && d < 0.0) negative = true;
        if (MIX) G[o] = lgamma(d + 1.0);
        if (CONV) {
            const double dc = d > SMALL_POS ? d : SMALL_POS;
            const double n1 = exp(emc_log_poisson(d, d));
            G[o] = lgamma(dc + 1);
            G[n_tb + o] = log(n1 > SMALL_POS ? n1 : SMALL_POS);
        }
    }
    if (negative) status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
}

// ------------------------------------------------------------------ correct_chi2, mcllh_mean, mcllh_eff
// grid.x: strips of 16 trials; FULL: grid.y = tiles of 16 templates, REDUCE: the workgroup walks all of them
template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(EMC_THREADS)
emc_pair_kernel(const double *__restrict__ D, const double *__restrict__ P, const double *__restrict__ G,
                const double *__restrict__ offset, int k0, int T, int K, int64_t B, double *__restrict__ out,
                double *__restrict__ best, int32_t *__restrict__ arg, double *__restrict__ at) {
    constexpr bool MIX = KIND != PISA_HIP_METRIC_CORRECT_CHI2;
    __shared__ double sD[EMC_TILE * EMC_LD];
    __shared__ double sG[MIX ? EMC_TILE * EMC_LD : 8];
    __shared__ double sP[EMC_PLANES_CHEAP][EMC_TILE * EMC_LD];
    const int tid = (int)threadIdx.x, ti = tid >> 4, ki = tid & 15;
    const int64_t t0 = (int64_t)blockIdx.x * EMC_TILE;
    const int64_t t = t0 + ti;
    const int64_t n_kb = (int64_t)K * B;
    const int n_kt = ens_tiles(K, EMC_TILE);
    const int kt_begin = REDUCE ? 0 : (int)blockIdx.y, kt_end = REDUCE ? n_kt : (int)blockIdx.y + 1;
    EnsOut<MIX, REDUCE> res;
    for (int kt = kt_begin; kt < kt_end; kt++) {
        const int64_t k = (int64_t)kt * EMC_TILE + ki;
        double sum = 0.0, comp = 0.0;
        for (int64_t c0 = 0; c0 < B; c0 += EMC_BK) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EMC_TILE * EMC_BK / EMC_THREADS; i++) {
                const int idx = tid + EMC_THREADS * i, r = idx / EMC_BK, cc = idx % EMC_BK;
                const int64_t b = c0 + cc, tt = t0 + r, kk = (int64_t)kt * EMC_TILE + r;
                const bool in_t = b < B && tt < T, in_k = b < B && kk < K;
                sD[r * EMC_LD + cc] = in_t ? D[tt * B + b] : 0.0;
                if (MIX) sG[r * EMC_LD + cc] = in_t ? G[tt * B + b] : 0.0;
#pragma unroll
                for (int p = 0; p < EMC_PLANES_CHEAP; p++)
                    sP[p][r * EMC_LD + cc] = in_k ? P[p * n_kb + kk * B + b] : 1.0;
            }
            __syncthreads();
            const int nb = (int)(B - c0 < EMC_BK ? B - c0 : EMC_BK);
            const double *pd = sD + ti * EMC_LD, *pg = sG + (MIX ? ti * EMC_LD : 0);
            const double *p0 = sP[0] + ki * EMC_LD, *p1 = sP[1] + ki * EMC_LD, *p2 = sP[2] + ki * EMC_LD;
            for (int cc = 0; cc < nb; cc++) {
                const double d = pd[cc], a = p0[cc], b1 = p1[cc], b2 = p2[cc];
                // as metric_kernel (metric_flux.hip): a non-finite input is a NaN bin, which np.nansum drops
                if (!emc_finite(d) || a != a) continue;
                double v;
                if (!MIX) {
                    const double dl = d - a;                // a = lam, b1 = s2 + lam, b2 = ln(s2 + lam)
                    v = (dl * dl) / b1 + b2;
                } else {
                    const double g = pg[cc];
                    if (a >= 0.0)                           // a = alpha, b1 = c0, b2 = log1p(beta)
                        v = ((b1 + lgamma(d + a)) - g) - (d + a) * b2;
                    else if (a == -1.0)                     // s2 == 0: b1 = ln lam, b2 = lam
                        v = (d * b1 - b2) - g;
                    else                                    // s2 < 0 (the status word carries the error)
                        v = d == 0 ? 0.0 : -HUGE_VAL;
                }
                if (v == v) ens_two_sum(sum, comp, v);      // np.nansum
            }
        }
        if (t < T && k < K) res.entry(sum + comp, t, k, K, offset, k0, out);
    }
    res.finish(t, T, ki, k0, best, arg, at);
}

// ------------------------------------------------------------------------------------------------- conv_llh
// One bin at a time: the node tables of the tile's 16 templates (2 x 101 x 16 doubles = 25.9 KB, node-major: the 16
// templates a wavefront reads at one node are consecutive) are built by the whole workgroup, then every lane runs its
// pair's 101 terms.
template <bool REDUCE>
__global__ void __launch_bounds__(EMC_THREADS)
emc_conv_kernel(const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ P,
                const double *__restrict__ G, const double *__restrict__ offset, int k0, int T, int K, int64_t B,
                int64_t n_tb, double *__restrict__ out, double *__restrict__ best, int32_t *__restrict__ arg,
                double *__restrict__ at) {
    __shared__ double tL[EMC_NODES * EMC_TILE];
    __shared__ double tQ[EMC_NODES * EMC_TILE];
    __shared__ double sW[3 * EMC_TILE];
    const int tid = (int)threadIdx.x, ti = tid >> 4, ki = tid & 15;
    const int64_t t0 = (int64_t)blockIdx.x * EMC_TILE;
    const int64_t t = t0 + ti;
    const int64_t n_kb = (int64_t)K * B;
    const int n_kt = ens_tiles(K, EMC_TILE);
    const int kt_begin = REDUCE ? 0 : (int)blockIdx.y, kt_end = REDUCE ? n_kt : (int)blockIdx.y + 1;
    EnsOut<true, REDUCE> res;
    for (int kt = kt_begin; kt < kt_end; kt++) {
        const int64_t k = (int64_t)kt * EMC_TILE + ki;
        const bool live = t < T && k < K;
        double sum = 0.0, comp = 0.0;
        for (int64_t b = 0; b < B; b++) {
            __syncthreads();
            for (int idx = tid; idx < EMC_NODES * EMC_TILE; idx += EMC_THREADS) {
                const int j = idx >> 4, r = idx & 15;
                const int64_t kk = (int64_t)kt * EMC_TILE + r;
                double L = 0.0, q = -HUGE_VAL;
                if (kk < K) {
                    const double e = E[kk * B + b];
                    const double lc = e > SMALL_POS ? e : SMALL_POS;
                    double x, cy;
                    emc_node(j, P[4 * n_kb + kk * B + b], P[3 * n_kb + kk * B + b], x, cy);
                    const double fx = x + lc;
                    if (fx > 0) {
                        L = log(fx);
                        q = cy - fx;
                    }
                }
                tL[idx] = L;
                tQ[idx] = q;
            }
            if (tid < 3 * EMC_TILE) {
                const int64_t kk = (int64_t)kt * EMC_TILE + (tid & 15);
                sW[tid] = kk < K ? P[(tid >> 4) * n_kb + kk * B + b] : 1.0;
            }
            __syncthreads();
            const double d = live ? D[t * B + b] : 0.0, norm = sW[ki];
            if (live && emc_finite(d) && norm == norm) {    // a non-finite input: a NaN bin, dropped
                const double dc = d > SMALL_POS ? d : SMALL_POS;
                const double lg = G[t * B + b], lb = G[n_tb + t * B + b];
                double conv = 0.0;
                for (int j = 0; j < EMC_NODES; j++)
                    conv += exp((dc * tL[j * EMC_TILE + ki] + tQ[j * EMC_TILE + ki]) - lg);
                const double a = (conv / norm) * sW[EMC_TILE + ki] / sW[2 * EMC_TILE + ki];
                const double v = log(a > SMALL_POS ? a : SMALL_POS) - lb;
                if (v == v) ens_two_sum(sum, comp, v);
            }
        }
        if (live) res.entry(sum + comp, t, k, K, offset, k0, out);
    }
    res.finish(t, T, ki, k0, best, arg, at);
}

// preparation buffers
static DeviceScratch g_emc_work;

template <int KIND, bool REDUCE>
static int emc_launch(const EnsArgs &a) {
    constexpr bool CONV = KIND == PISA_HIP_METRIC_CONV_LLH;
    constexpr int n_p = CONV ? EMC_PLANES_CONV : EMC_PLANES_CHEAP;
    constexpr int n_g = CONV ? 2 : (KIND == PISA_HIP_METRIC_CORRECT_CHI2 ? 0 : 1);
    const int T = (int)a.T, K = (int)a.K;
    const int64_t B = a.B, n_kb = (int64_t)K * B, n_tb = (int64_t)T * B;
    hipStream_t stream = as_stream(a.stream);
    double *w;
    const int rc = g_emc_work.reserve(n_p * n_kb + n_g * n_tb + 1, &w);
    if (rc != PISA_HIP_OK) return rc;
    double *P = w, *G = w + n_p * n_kb;
    const int64_t n_el = n_kb + (n_g ? n_tb : 0);
    hipLaunchKernelGGL((emc_prep_kernel<KIND>), dim3((unsigned)((n_el + EMC_THREADS - 1) / EMC_THREADS)),
                       dim3(EMC_THREADS), 0, stream, a.D, a.E, a.S2, n_g ? n_tb : (int64_t)0, n_kb, P, G, a.status);
    PISA_CHECK_LAUNCH("emc_prep_kernel");
    const dim3 grid((unsigned)ens_tiles(T, EMC_TILE), REDUCE ? 1u : (unsigned)ens_tiles(K, EMC_TILE));
    if constexpr (CONV) {
        hipLaunchKernelGGL((emc_conv_kernel<REDUCE>), grid, dim3(EMC_THREADS), 0, stream, a.D, a.E, P, G, a.offset,
                           a.k0, T, K, B, n_tb, a.out, a.best, a.arg, a.at);
        PISA_CHECK_LAUNCH("emc_conv_kernel");
    } else {
        hipLaunchKernelGGL((emc_pair_kernel<KIND, REDUCE>), grid, dim3(EMC_THREADS), 0, stream, a.D, P, G, a.offset,
                           a.k0, T, K, B, a.out, a.best, a.arg, a.at);
        PISA_CHECK_LAUNCH("emc_pair_kernel");
    }
    return PISA_HIP_OK;
}

template <bool REDUCE>
static int emc_run(int32_t kind, const EnsArgs &a) {
    if (kind != PISA_HIP_METRIC_CORRECT_CHI2 && kind != PISA_HIP_METRIC_MCLLH_MEAN &&
        kind != PISA_HIP_METRIC_MCLLH_EFF && kind != PISA_HIP_METRIC_CONV_LLH)
        return PISA_HIP_ERR_INVALID;
    if (!ens_check_matrix<REDUCE>(a, EMC_TILE) || !a.S2) return PISA_HIP_ERR_INVALID;
    // the preparation has one thread per bin of every row
    if ((a.T + a.K) * a.B > (int64_t)0x7FFFFFFF * EMC_THREADS) return PISA_HIP_ERR_INVALID;
    return dispatch_int<PISA_HIP_METRIC_CORRECT_CHI2, PISA_HIP_METRIC_MCLLH_MEAN, PISA_HIP_METRIC_MCLLH_EFF,
                        PISA_HIP_METRIC_CONV_LLH>(
        kind, [&](auto c) { return emc_launch<decltype(c)::value, REDUCE>(a); });
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_metric_matrix_mc(int32_t kind, const double *d_data, const double *d_expected,
                                       const double *d_sigma2, int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                       double *d_out, int32_t *d_status, void *stream) {
    return emc_run<false>(kind, {d_data, d_expected, d_sigma2, nullptr, 0, n_trials, n_templates, n_bins, d_out,
                                 nullptr, nullptr, nullptr, d_status, stream});
}

PISA_API int pisa_hip_metric_matrix_mc_best(int32_t kind, const double *d_data, const double *d_expected,
                                            const double *d_sigma2, const double *d_offset, int32_t k0,
                                            int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_best,
                                            int32_t *d_arg, double *d_at, int32_t *d_status, void *stream) {
    return emc_run<true>(kind, {d_data, d_expected, d_sigma2, d_offset, k0, n_trials, n_templates, n_bins, nullptr,
                                d_best, d_arg, d_at, d_status, stream});
}
