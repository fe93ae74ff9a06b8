// hist_tail.hip -- the tail of an evaluation for gfx950: the limbs of the accumulate kernels (hist_device.hpp) -> fp64
// maps, rounded once, alone (hist_finalize) or fused with the metric (finalize_metric, finalize_gpllh).
#include "hist_device.hpp"
#include "metric_device.hpp"
#include "gpllh_device.hpp"

namespace pisa {

__global__ void __launch_bounds__(256)
hist_finalize_kernel(const long long *__restrict__ limbs, int64_t n_total_bins,
                     double *__restrict__ hist, double *__restrict__ q1,
                     int32_t *__restrict__ status) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_total_bins) return;
    bool ovf = false;
    if (hist) hist[b] = limbs_to_double(limbs + (b * 2 + 0) * NL, ovf);
    if (q1) q1[b] = limbs_to_double(limbs + (b * 2 + 1) * NL, ovf);
    if (ovf && status) atomicOr(status, 1);
}

// hist_finalize_kernel + metric_kernel (metric_flux.hip) in one workgroup: the
// tail of a template evaluation is launch-bound, not work-bound.  The metric part
// repeats metric_kernel's loop and reduction tree exactly (first 256 threads).
// One instantiation per metric: with a run-time `kind` the lgamma of poisson_llh sets the
// register need of every variant and the 128-VGPR budget of a 1024-thread workgroup spills.
// SPLIT = 4: FOUR workgroups per point, workgroup k takes the bins b = k mod 4 of every container (a quarter of the
// conversions -- what the one-workgroup form spends its time on: 3 per thread at the headline size) and leaves the
// partial sum u_k of the metric over ITS bins in total[4 * point + k].  The reduction tree below adds thread t to
// t + 128, t + 64, lane to lane + 32 .. + 4 -- all multiples of 4 -- before it joins the four residue classes with
// lane + 2 and lane + 1: u_k is exactly what lane k holds in the one-workgroup form before those last two steps, and
//       total = (u_0 + u_2) + (u_1 + u_3)
// added by the caller is the one-workgroup result bit for bit.  Not for chi2 (its all-bins-equal rule needs every bin).
template <int KIND, int SPLIT = 1>
__global__ void __launch_bounds__(1024)
finalize_metric_kernel(long long *__restrict__ limbs, int n_cont, int n_bins,
                       double *__restrict__ hist, double *__restrict__ q1,
                       const double *__restrict__ actual, double *__restrict__ total,
                       int32_t *__restrict__ status, int32_t *__restrict__ mstatus, int clear,
                       const double *__restrict__ scale, const double *__restrict__ extra,
                       int64_t limb_stride, int64_t scale_stride) {
    extern __shared__ __attribute__((aligned(16))) double s_map[];  // [2][n_cont][n_bins]
    __shared__ double s_sum[256];
    __shared__ int s_flag[2];
    constexpr int kind = KIND;
    const int n_tot = n_cont * n_bins;
    const int part = SPLIT > 1 ? (int)(blockIdx.x % SPLIT) : 0;   // this workgroup's bins: b = part mod SPLIT
    {
        // one workgroup (SPLIT of them) per parameter point (pisa_hip_finalize_metric_multi; a single point: 0)
        const int64_t pt = blockIdx.x / SPLIT;
        limbs += pt * limb_stride;
        hist += pt * n_tot;
        q1 += pt * n_tot;
        total += pt * SPLIT;
        if (scale) scale += pt * scale_stride;
    }
    if (threadIdx.x < 2) s_flag[threadIdx.x] = 0;
    // first bin's observed count: requested before anything else, used after the barrier
    double k_first = 0.0;
    if (threadIdx.x < 256 && (int)threadIdx.x < n_bins) k_first = actual[threadIdx.x];
    bool ovf = false;
    // One item = the NL limbs of one (bin, quantity) sum; item `it` sits at limbs + it*NL, so
    // a wave reads one contiguous run.  The limbs were produced by device-scope atomics and
    // come from beyond the L2: every load of (up to) four items per thread is issued before
    // the first conversion, so the kernel pays that latency once.
    // SPLIT > 1: the workgroup's items are numbered l = 2 (container * nb + j) + quantity over ITS nb bins j * SPLIT + part
    const int nb = SPLIT > 1 ? (n_bins - part + SPLIT - 1) / SPLIT : n_bins;
    const int n_items = 2 * n_cont * (nb > 0 ? nb : 0);
    auto item_of = [&](int l) {
        if (SPLIT == 1) return l;
        const int jq = l >> 1, cont = jq / nb, j = jq - cont * nb;
        return 2 * (cont * n_bins + j * SPLIT + part) + (l & 1);
    };
    constexpr int UNR = 4;
    for (int base = 0; base < n_items; base += UNR * (int)blockDim.x) {
        long long w[UNR][NL];
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const int l = base + u * (int)blockDim.x + (int)threadIdx.x;
            const long long *L = limbs + (int64_t)(l < n_items ? item_of(l) : 0) * NL;
#pragma unroll
            for (int k = 0; k < NL; k++) w[u][k] = L[k];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const int l = base + u * (int)blockDim.x + (int)threadIdx.x;
            const int it = l < n_items ? item_of(l) : 0;
            if (l < n_items) {
                if (clear) {
                    long long *L = limbs + (int64_t)it * NL;
#pragma unroll
                    for (int k = 0; k < NL; k++) L[k] = 0;
                }
                const int i = it >> 1, q = it & 1;
                const double d = limbs_to_double(w[u], ovf);
                (q ? q1 : hist)[i] = d;   // the maps are written as histogrammed
                double v = d;
                if (scale) {
                    // per-bin scale factors of a stage that follows the histogram
                    // (discr_sys.hypersurfaces: weights = clip(weights * s, 0, inf), errors *= s;
                    // hypersurfaces.py:251-259) enter the metric's expectation only
                    const double sc = scale[i];
                    const double e = sqrt(d) * sc;   // errors = sqrt(sumw2) * s, variance = errors^2
                    v = q ? e * e : fmax(d * sc, 0.0);
                }
                s_map[q * n_tot + i] = v;
            }
            // conversions one after the other: interleaved they exceed the 128-VGPR budget
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (ovf && status) atomicOr(status, 1);
    __syncthreads();
    const double *expected = s_map, *sigma2 = s_map + n_tot;
    double acc = 0.0;
    if (threadIdx.x < 256) {
        // (SPLIT > 1: b mod SPLIT = thread mod SPLIT -- the threads of the other residue classes have no bin here)
        for (int b = threadIdx.x; b < n_bins && (SPLIT == 1 || (int)(threadIdx.x % SPLIT) == part); b += 256) {
            const double k = (b == (int)threadIdx.x) ? k_first : actual[b];
            double lam = 0.0, s2 = 0.0;
            for (int m = 0; m < n_cont; m++) {
                lam = (m == 0) ? expected[b] : lam + expected[m * n_bins + b];
                s2 = (m == 0) ? sigma2[b] : s2 + sigma2[m * n_bins + b];
            }
            if (extra) {   // maps of other pipelines added to the template (distribution_maker.py:274-281)
                lam += extra[b];
                s2 += extra[n_bins + b];
            }
            double v;
            const bool finite = (k == k) && (lam == lam) && !isinf(k) && !isinf(lam);
            if (!finite) {
                v = __longlong_as_double(0x7ff8000000000000LL);
            } else {
                if (k < 0.0 || lam < 0.0) atomicOr(&s_flag[0], 1);
                if (kind == PISA_HIP_METRIC_CHI2) {
                    const double lc = lam < SMALL_POS ? SMALL_POS : lam;
                    if (!(fabs(k - lc) < 5 * FTYPE_PREC)) atomicOr(&s_flag[1], 1);
                }
                v = metric_bin(kind, k, lam, s2);
            }
            if (v == v) acc += v;  // np.nansum
        }
        s_sum[threadIdx.x] = acc;
    }
    __syncthreads();
    // metric_kernel's reduction tree (s_sum[t] += s_sum[t + off], off = 128 .. 1): the same
    // additions in the same pairing, the last six levels inside wave 0 with lane shuffles
    // instead of LDS round trips and workgroup barriers
    if (threadIdx.x < 128) s_sum[threadIdx.x] += s_sum[threadIdx.x + 128];
    __syncthreads();
    if (threadIdx.x < 64) {
        double v = s_sum[threadIdx.x] + s_sum[threadIdx.x + 64];
#pragma unroll
        for (int off = 32; off >= SPLIT; off >>= 1) v += __shfl_down(v, off);
        if (SPLIT > 1) {
            if ((int)threadIdx.x == part) {
                const bool negative = mstatus && s_flag[0];
                total[part] = negative ? __builtin_nan("") : v;
                if (negative) mstatus[0] = PISA_HIP_ERR_NEGATIVE;
            }
        } else if (threadIdx.x == 0) {
            const bool chi2_zero = (kind == PISA_HIP_METRIC_CHI2) && s_flag[1] == 0;  // stats.py:160-161
            // negative input (stats.py:231-240 raises): the value is NaN as well, so that a host
            // that polls `total` in pinned memory needs to read the status word only then
            const bool negative = mstatus && s_flag[0];
            total[0] = negative ? __builtin_nan("") : (chi2_zero ? 0.0 : v);
            if (negative) mstatus[0] = PISA_HIP_ERR_NEGATIVE;
        }
    }
}

}  // namespace pisa

using namespace pisa;

static int finalize_metric_impl(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                const double *d_actual, const double *d_scale,
                                int64_t scale_point_stride, const double *d_extra, double *total,
                                int32_t *d_status, int32_t *d_metric_status,
                                int32_t clear_limbs, void *stream, int n_parts) {
    if (!d_limbs || !d_hist || !d_sumw2 || !d_actual || !total || n_containers < 1 || n_bins < 1 ||
        n_points < 1 || n_points > PISA_HIP_MAX_POINTS)
        return PISA_HIP_ERR_INVALID;
    if (kind < PISA_HIP_METRIC_LLH || kind > PISA_HIP_METRIC_MOD_CHI2) return PISA_HIP_ERR_INVALID;
    if (n_parts != 1 && n_parts != 4 && n_parts != 16) return PISA_HIP_ERR_INVALID;
    const bool split = n_parts > 1;
    if (split && kind == PISA_HIP_METRIC_CHI2) return PISA_HIP_ERR_INVALID;
    if ((int64_t)n_containers * n_bins > PISA_HIP_FINALIZE_METRIC_MAX) return PISA_HIP_ERR_INVALID;
    const int n_tot = (int)(n_containers * n_bins);
    // a thread per accumulator of the workgroup's share where 1 024 threads allow it
    int threads = (((split ? (2 * n_tot + n_parts - 1) / n_parts : n_tot) + 63) / 64) * 64;
    if (threads < 256) threads = 256;  // the metric reduction tree is 256 wide
    if (threads > 1024) threads = 1024;
    const int64_t limb_stride = (int64_t)n_tot * 2 * NL;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)(n_points * n_parts)), dim3(threads), (size_t)n_tot * 16,
                           as_stream(stream), (long long *)d_limbs, (int)n_containers, (int)n_bins, d_hist, d_sumw2,
                           d_actual, total, d_status, d_metric_status, (int)clear_limbs, d_scale, d_extra,
                           limb_stride, (int64_t)scale_point_stride);
    };
    if (n_parts == 16) {
        switch (kind) {
        case PISA_HIP_METRIC_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_LLH, 16>); break;
        case PISA_HIP_METRIC_POISSON_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_POISSON_LLH, 16>); break;
        default: launch(finalize_metric_kernel<PISA_HIP_METRIC_MOD_CHI2, 16>);
        }
    } else if (split) {
        switch (kind) {
        case PISA_HIP_METRIC_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_LLH, 4>); break;
        case PISA_HIP_METRIC_POISSON_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_POISSON_LLH, 4>); break;
        default: launch(finalize_metric_kernel<PISA_HIP_METRIC_MOD_CHI2, 4>);
        }
    } else {
        switch (kind) {
        case PISA_HIP_METRIC_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_LLH>); break;
        case PISA_HIP_METRIC_POISSON_LLH: launch(finalize_metric_kernel<PISA_HIP_METRIC_POISSON_LLH>); break;
        case PISA_HIP_METRIC_CHI2: launch(finalize_metric_kernel<PISA_HIP_METRIC_CHI2>); break;
        default: launch(finalize_metric_kernel<PISA_HIP_METRIC_MOD_CHI2>);
        }
    }
    PISA_CHECK_LAUNCH("finalize_metric_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_finalize_metric_multi(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                            int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                            const double *d_actual, const double *d_scale,
                                            int64_t scale_point_stride, const double *d_extra, double *total,
                                            int32_t *d_status, int32_t *d_metric_status,
                                            int32_t clear_limbs, void *stream) {
    return finalize_metric_impl(d_limbs, n_points, n_containers, n_bins, d_hist, d_sumw2, kind, d_actual, d_scale,
                                scale_point_stride, d_extra, total, d_status, d_metric_status, clear_limbs, stream, 1);
}

PISA_API int pisa_hip_finalize_metric_split(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                            int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                            const double *d_actual, const double *d_scale,
                                            int64_t scale_point_stride, const double *d_extra, double *partial,
                                            int32_t *d_status, int32_t *d_metric_status,
                                            int32_t clear_limbs, void *stream) {
    return finalize_metric_impl(d_limbs, n_points, n_containers, n_bins, d_hist, d_sumw2, kind, d_actual, d_scale,
                                scale_point_stride, d_extra, partial, d_status, d_metric_status, clear_limbs, stream, 4);
}

PISA_API int pisa_hip_finalize_metric_parts(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                            int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                            const double *d_actual, const double *d_scale,
                                            int64_t scale_point_stride, const double *d_extra, double *partial,
                                            int32_t n_parts, int32_t *d_status, int32_t *d_metric_status,
                                            int32_t clear_limbs, void *stream) {
    if (n_parts != 4 && n_parts != 16) return PISA_HIP_ERR_INVALID;
    return finalize_metric_impl(d_limbs, n_points, n_containers, n_bins, d_hist, d_sumw2, kind, d_actual, d_scale,
                                scale_point_stride, d_extra, partial, d_status, d_metric_status, clear_limbs, stream,
                                n_parts);
}

PISA_API int pisa_hip_finalize_metric_scaled(int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                                             double *d_hist, double *d_sumw2, int32_t kind,
                                             const double *d_actual, const double *d_scale,
                                             const double *d_extra, double *total, int32_t *d_status,
                                             int32_t *d_metric_status, int32_t clear_limbs,
                                             void *stream) {
    return pisa_hip_finalize_metric_multi(d_limbs, 1, n_containers, n_bins, d_hist, d_sumw2, kind, d_actual,
                                          d_scale, 0, d_extra, total, d_status, d_metric_status, clear_limbs,
                                          stream);
}

PISA_API int pisa_hip_finalize_metric(int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                                      double *d_hist, double *d_sumw2, int32_t kind,
                                      const double *d_actual, double *total, int32_t *d_status,
                                      int32_t *d_metric_status, int32_t clear_limbs,
                                      void *stream) {
    return pisa_hip_finalize_metric_scaled(d_limbs, n_containers, n_bins, d_hist, d_sumw2, kind, d_actual,
                                           nullptr, nullptr, total, d_status, d_metric_status, clear_limbs,
                                           stream);
}

PISA_API int pisa_hip_hist_finalize(const int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                                    double *d_hist, double *d_sumw2, int32_t *d_status,
                                    void *stream) {
    if (!d_limbs || n_containers < 1 || n_bins < 1) return PISA_HIP_ERR_INVALID;
    int64_t total = (int64_t)n_containers * n_bins;
    dim3 block(256), grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(hist_finalize_kernel, grid, block, 0, as_stream(stream),
                       (const long long *)d_limbs, total, d_hist, d_sumw2, d_status);
    PISA_CHECK_LAUNCH("hist_finalize_kernel");
    return PISA_HIP_OK;
}

// The fused tail of an evaluation with the generalized Poisson-gamma likelihood: limbs -> maps (written as
// histogrammed, limbs cleared) -> alpha, beta of every container (gpllh_params) -> the bin (gpllh_bin) -> the total
// (gpllh_publish_and_total).  One 64-thread workgroup per (bin, point): the same values, in the same order, as
// pisa_hip_hist_finalize + pisa_hip_gpllh_params + pisa_hip_generalized_poisson_llh.
__global__ void __launch_bounds__(64)
finalize_gpllh_kernel(long long *__restrict__ limbs, int n_cont, int n_bins, double *__restrict__ hist,
                      double *__restrict__ q1, const double *__restrict__ actual, const double *__restrict__ n_mc,
                      const double *__restrict__ adjust, const uint8_t *__restrict__ empty,
                      double *__restrict__ per_bin, double *__restrict__ scratch, int64_t cap,
                      unsigned int *__restrict__ done, double *__restrict__ total, int32_t *__restrict__ status, int32_t *__restrict__ mstatus,
                      int clear, int64_t limb_stride) {
    extern __shared__ __attribute__((aligned(16))) double s_tab[];   // [4][n_cont] + s, delta
    const int b = blockIdx.x, pt = blockIdx.y;
    const int64_t n_tot = (int64_t)n_cont * n_bins;
    limbs += pt * limb_stride;
    hist += pt * n_tot;
    q1 += pt * n_tot;
    double *c_w = s_tab, *c_a = s_tab + n_cont, *c_b = s_tab + 2 * n_cont, *c_n = s_tab + 3 * n_cont;
    bool ovf = false, neg = false;
    for (int c = threadIdx.x; c < n_cont; c += 64) {
        const int64_t i = (int64_t)c * n_bins + b;
        long long *L = limbs + i * 2 * NL;
        const double sw = limbs_to_double(L, ovf), sw2 = limbs_to_double(L + NL, ovf);
        if (clear) {
#pragma unroll
            for (int k = 0; k < 2 * NL; k++) L[k] = 0;
        }
        hist[i] = sw;
        q1[i] = sw2;
        const double n = n_mc[i];
        neg = gpllh_params(sw, sw2, n, adjust[c], c_a[c], c_b[c], c_w[c]) || neg;
        c_n[c] = n;
    }
    if (ovf && status) atomicOr(status, 1);
    if (neg) mstatus[0] = PISA_HIP_ERR_NEGATIVE;
    __syncthreads();
    const double kd = actual[b];
    const int64_t lds_k = gpllh_lds_k(cap);
    double *sbuf = s_tab + 4 * n_cont;
    int64_t bcap = lds_k;
    if (kd > (double)lds_k && scratch) {
        sbuf = scratch + ((int64_t)pt * n_bins + b) * 2 * (cap + 1);
        bcap = cap;
    }
    int err = 0;
    const double v = gpllh_bin(kd, empty && empty[b], n_cont, c_w, c_a, c_b, c_n, sbuf, bcap, err);
    if (err && threadIdx.x == 0) mstatus[0] = err;
    gpllh_publish_and_total(v, b, n_bins, per_bin + (int64_t)pt * n_bins, done + pt, total + pt);
}

PISA_API int pisa_hip_finalize_gpllh(int64_t *d_limbs, int32_t n_points, int32_t n_containers, int64_t n_bins,
                                     double *d_hist, double *d_sumw2, const double *d_actual, const double *d_n_mc,
                                     const double *d_adjust, const uint8_t *d_empty, double *d_per_bin,
                                     double *d_scratch, int64_t scratch_k, uint32_t *d_done, double *total,
                                     int32_t *d_status,
                                     int32_t *d_metric_status, int32_t clear_limbs, void *stream) {
    if (!d_limbs || !d_hist || !d_sumw2 || !d_actual || !d_n_mc || !d_adjust || !d_per_bin || !d_done || !total ||
        !d_metric_status || n_containers < 1 || n_containers > PISA_HIP_GPLLH_MAX_CONTAINERS || n_bins < 1 ||
        n_bins > 0x7FFFFFFF || n_points < 1 || n_points > PISA_HIP_MAX_POINTS || scratch_k < 0)
        return PISA_HIP_ERR_INVALID;
    if (scratch_k > PISA_HIP_GPLLH_LDS_K && !d_scratch) return PISA_HIP_ERR_INVALID;
    const int64_t limb_stride = (int64_t)n_containers * n_bins * 2 * NL;
    hipLaunchKernelGGL(finalize_gpllh_kernel, dim3((unsigned)n_bins, (unsigned)n_points), dim3(64),
                       gpllh_lds_bytes(n_containers, scratch_k), as_stream(stream), (long long *)d_limbs,
                       (int)n_containers, (int)n_bins, d_hist, d_sumw2, d_actual, d_n_mc, d_adjust, d_empty,
                       d_per_bin, scratch_k > PISA_HIP_GPLLH_LDS_K ? d_scratch : nullptr, scratch_k, (unsigned int *)d_done, total,
                       d_status,
                       d_metric_status, (int)clear_limbs, limb_stride);
    PISA_CHECK_LAUNCH("finalize_gpllh_kernel");
    return PISA_HIP_OK;
}
