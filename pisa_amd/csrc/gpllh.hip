// gpllh.hip -- the generalized Poisson-gamma likelihood on maps (stats.py generalized_poisson_llh) and its
// inputs (stages/likelihood/generalized_llh_params.py):
//   gpllh_bin_sums_kernel   Sigma w, Sigma w^2 over the events of each bin (CSR event lists)
//   gpllh_params_kernel     (Sigma w, Sigma w^2, n, mean adjustment) -> alpha, beta, pseudo-filled weight sum
//   gpllh_metric_kernel     per-bin values (gpllh_device.hpp) and their total
// The fused tail of an evaluation (limbs -> the same three steps in one launch) is finalize_gpllh_kernel in hist_tail.hip.
#include "gpllh_device.hpp"

namespace pisa {

// One workgroup per bin: its events are d_index[d_offsets[b] .. d_offsets[b + 1]); thread t adds every 256th of
// them in sequence, a fixed tree joins the threads.
__global__ void __launch_bounds__(256)
gpllh_bin_sums_kernel(const double *__restrict__ w, const int64_t *__restrict__ index,
                      const int64_t *__restrict__ offsets, double *__restrict__ sw, double *__restrict__ sw2,
                      int32_t *__restrict__ status) {
    __shared__ double s1[256], s2[256];
    const int64_t b = blockIdx.x;
    const int64_t lo = offsets[b], hi = offsets[b + 1];
    double a1 = 0.0, a2 = 0.0;
    bool neg = false;
    for (int64_t e = lo + threadIdx.x; e < hi; e += 256) {
        const double x = w[index[e]];
        neg = neg || !(x >= 0.0);
        a1 += x;
        a2 += x * x;
    }
    if (neg) status[0] = PISA_HIP_ERR_NEGATIVE;   // generalized_llh_params.py: 'SOME WEIGHTS BELOW ZERO'
    s1[threadIdx.x] = a1;
    s2[threadIdx.x] = a2;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s1[threadIdx.x] += s1[threadIdx.x + off];
            s2[threadIdx.x] += s2[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sw[b] = s1[0];
        sw2[b] = s2[0];
    }
}

__global__ void __launch_bounds__(256)
gpllh_params_kernel(const double *__restrict__ sw, const double *__restrict__ sw2, const double *__restrict__ n_mc,
                    const double *__restrict__ adjust, int64_t n_bins, int64_t n_tot, double *__restrict__ alpha,
                    double *__restrict__ beta, double *__restrict__ wsum, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tot) return;
    double a, b, w;
    if (gpllh_params(sw[i], sw2[i], n_mc[i], adjust[i / n_bins], a, b, w)) status[0] = PISA_HIP_ERR_NEGATIVE;
    alpha[i] = a;
    beta[i] = b;
    wsum[i] = w;
}

__global__ void __launch_bounds__(64)
gpllh_metric_kernel(const double *__restrict__ actual, const double *__restrict__ weights,
                    const double *__restrict__ alpha, const double *__restrict__ beta,
                    const double *__restrict__ n_mc, int n_cont, int n_bins, const uint8_t *__restrict__ empty,
                    double *__restrict__ scratch, int64_t cap, double *__restrict__ per_bin,
                    unsigned int *__restrict__ done, double *__restrict__ total, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double s_tab[];   // [4][n_cont] + s, delta
    const int b = blockIdx.x;
    double *c_w = s_tab, *c_a = s_tab + n_cont, *c_b = s_tab + 2 * n_cont, *c_n = s_tab + 3 * n_cont;
    for (int c = threadIdx.x; c < n_cont; c += 64) {
        const int64_t i = (int64_t)c * n_bins + b;
        c_w[c] = weights[i];
        c_a[c] = alpha[i];
        c_b[c] = beta[i];
        c_n[c] = n_mc[i];
    }
    __syncthreads();
    const double kd = actual[b];
    const int64_t lds_k = gpllh_lds_k(cap);
    double *sbuf = s_tab + 4 * n_cont;
    int64_t bcap = lds_k;
    if (kd > (double)lds_k && scratch) {
        sbuf = scratch + (int64_t)b * 2 * (cap + 1);
        bcap = cap;
    }
    int err = 0;
    const double v = gpllh_bin(kd, empty && empty[b], n_cont, c_w, c_a, c_b, c_n, sbuf, bcap, err);
    if (err && threadIdx.x == 0) status[0] = err;
    gpllh_publish_and_total(v, b, n_bins, per_bin, done, total);
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_gpllh_bin_sums(const double *d_weights, const int64_t *d_index, const int64_t *d_offsets,
                                     int64_t n_bins, double *d_sumw, double *d_sumw2, int32_t *d_status,
                                     void *stream) {
    if (n_bins < 1 || n_bins > 0x7FFFFFFF || !d_offsets || !d_sumw || !d_sumw2 || !d_status) return PISA_HIP_ERR_INVALID;
    hipLaunchKernelGGL(gpllh_bin_sums_kernel, dim3((unsigned)n_bins), dim3(256), 0, as_stream(stream), d_weights,
                       d_index, d_offsets, d_sumw, d_sumw2, d_status);
    PISA_CHECK_LAUNCH("gpllh_bin_sums_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_gpllh_params(const double *d_sumw, const double *d_sumw2, const double *d_n_mc,
                                   const double *d_adjust, int32_t n_containers, int64_t n_bins, double *d_alpha,
                                   double *d_beta, double *d_weights, int32_t *d_status, void *stream) {
    if (n_containers < 1 || n_bins < 1 || !d_sumw || !d_sumw2 || !d_n_mc || !d_adjust || !d_alpha || !d_beta ||
        !d_weights || !d_status)
        return PISA_HIP_ERR_INVALID;
    const int64_t n_tot = (int64_t)n_containers * n_bins;
    hipLaunchKernelGGL(gpllh_params_kernel, dim3((unsigned)((n_tot + 255) / 256)), dim3(256), 0, as_stream(stream),
                       d_sumw, d_sumw2, d_n_mc, d_adjust, n_bins, n_tot, d_alpha, d_beta, d_weights, d_status);
    PISA_CHECK_LAUNCH("gpllh_params_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_generalized_poisson_llh(const double *d_actual, const double *d_weights, const double *d_alpha,
                                              const double *d_beta, const double *d_n_mc, int32_t n_containers,
                                              int64_t n_bins, const uint8_t *d_empty, double *d_scratch,
                                              int64_t scratch_k, double *d_per_bin, uint32_t *d_done,
                                              double *d_total, int32_t *d_status, void *stream) {
    if (n_containers < 1 || n_containers > PISA_HIP_GPLLH_MAX_CONTAINERS || n_bins < 1 || n_bins > 0x7FFFFFFF ||
        scratch_k < 0 || !d_actual || !d_weights || !d_alpha || !d_beta || !d_n_mc || !d_per_bin || !d_done || !d_total ||
        !d_status)
        return PISA_HIP_ERR_INVALID;
    if (scratch_k > PISA_HIP_GPLLH_LDS_K && !d_scratch) return PISA_HIP_ERR_INVALID;
    hipLaunchKernelGGL(gpllh_metric_kernel, dim3((unsigned)n_bins), dim3(64), gpllh_lds_bytes(n_containers, scratch_k),
                       as_stream(stream), d_actual, d_weights, d_alpha, d_beta, d_n_mc, (int)n_containers,
                       (int)n_bins, d_empty, scratch_k > PISA_HIP_GPLLH_LDS_K ? d_scratch : nullptr, scratch_k,
                       d_per_bin, (unsigned int *)d_done, d_total, d_status);
    PISA_CHECK_LAUNCH("gpllh_metric_kernel");
    return PISA_HIP_OK;
}
