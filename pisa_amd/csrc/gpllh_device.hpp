// gpllh_device.hpp -- the generalized Poisson-gamma likelihood (arXiv:1902.08831, eq. 91) shared by the
// unfused kernels (gpllh.hip) and the fused tail of an evaluation (hist_tail.hip): both call these functions with
// the same inputs in the same launch shape, so the two paths agree bit for bit.
//
// Launch shape of the bin evaluation: ONE wavefront (a 64-thread workgroup) per bin.  Bins whose every container
// has more than 100 MC events take the Poisson branch (lane 0, a few flops); the others run the k-step recursion
// of eq. 91 with the lanes splitting the j-sum and a butterfly reduction joining them (every lane ends with the
// same bits).  s and delta live in LDS up to PISA_HIP_GPLLH_LDS_K, beyond it in a caller-sized global scratch.
#pragma once
#include "common.hpp"

namespace pisa {

constexpr double GPLLH_PSEUDO_WEIGHT = 0.001;   // generalized_llh_params.py: PSEUDO_WEIGHT
constexpr double GPLLH_LOG_SMALL = -23.025850929940457;   // log(1e-10), stats.py: empty bins with data
constexpr double GPLLH_TINY = 1e-300;                      // poisson.py fast_pgmix

// generalized_llh_params.apply_function for one (container, bin): Sigma w, Sigma w^2 and the MC count n of the bin,
// `adj` the container's mean adjustment.  An empty bin gets one pseudo-weight.  Returns true on a negative input.
__device__ __forceinline__ bool gpllh_params(double sw, double sw2, double n, double adj, double &alpha,
                                             double &beta, double &wsum) {
    const bool bad = !(sw >= 0.0) || !(sw2 >= 0.0) || !(n >= 0.0);
    if (!(n > 0.0)) {
        sw = GPLLH_PSEUDO_WEIGHT;
        sw2 = GPLLH_PSEUDO_WEIGHT * GPLLH_PSEUDO_WEIGHT;
        n = 1.0;
    }
    wsum = sw;
    const double mean = sw / n, var_z = sw2 / n;
    if (var_z != 0.0) {
        beta = mean / var_z;
        alpha = (n + adj) * ((mean * mean) / var_z);
    } else {
        beta = 1.0;
        alpha = (n + adj) * GPLLH_PSEUDO_WEIGHT;
    }
    return bad;
}

__device__ __forceinline__ double wave_sum(double v) {
    // butterfly: lane l adds lane l ^ m; addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// One bin, evaluated by the whole (single-wave) workgroup; every thread must call it (it holds barriers).
// c_w / c_a / c_b / c_n: per-container weight sum (pseudo-filled), alpha, beta, MC count of the bin, in LDS.
// sbuf: 2 (cap + 1) doubles (LDS or the bin's global scratch), cap >= k or the bin fails with INVALID.
// Returns the bin's value on every lane; *err receives PISA_HIP_ERR_* (0 if none).
__device__ __noinline__ double gpllh_bin(double kd, bool empty, int n_cont, const double *c_w, const double *c_a,
                                         const double *c_b, const double *c_n, double *sbuf, int64_t cap,
                                         int &err) {
    const int lane = (int)threadIdx.x;
    err = 0;
    if (!(kd >= 0.0)) {
        err = PISA_HIP_ERR_NEGATIVE;
        return 0.0;
    }
    const long long k = (long long)kd;   // np.int64(data): truncated
    if (empty) return k > 0 ? GPLLH_LOG_SMALL : 0.0;
    bool all_high = true;
    for (int c = 0; c < n_cont; c++) {
        if (!(c_w[c] >= 0.0)) err = PISA_HIP_ERR_NEGATIVE;
        all_high = all_high && c_n[c] > 100.0;
    }
    if (err) return 0.0;
    if (all_high) {
        double W = 0.0;
        for (int c = 0; c < n_cont; c++) W += c_w[c];
        if (k == 0) return -W;   // the limit of k log k (the reference evaluates 0 log 0 = NaN)
        const double x = (double)k;
        return x * log(W) - W - (x * log(x) - x);
    }
    // eq. 91 over the containers with finite alpha and beta (poisson_gamma.c generalized_pg_mixture)
    double prefac = 1.0;
    for (int c = 0; c < n_cont; c++) {
        const double a = c_a[c], b = c_b[c];
        if (isfinite(a) && isfinite(b)) {
            if (!(a > 0.0) || !(b > 0.0)) err = PISA_HIP_ERR_INVALID;
            prefac *= pow(1.0 / (1.0 + 1.0 / b), a);
        }
    }
    if (err) return 0.0;
    if (k > cap) {
        err = PISA_HIP_ERR_INVALID;
        return 0.0;
    }
    double *s = sbuf, *delta = sbuf + (cap + 1);
    // s_i = sum_c alpha_c r_c^i, r_c = 1 / (1 + beta_c), i = 1 .. k (lanes over i)
    for (long long i = 1 + lane; i <= k; i += 64) {
        double acc = 0.0;
        for (int c = 0; c < n_cont; c++) {
            const double a = c_a[c], b = c_b[c];
            if (isfinite(a) && isfinite(b)) acc += a * pow(1.0 / (1.0 + b), (double)i);
        }
        s[i] = acc;
    }
    if (lane == 0) delta[0] = 1.0;
    __syncthreads();
    // delta_i = (1/i) sum_{j=1..i} s_j delta_{i-j}: lane l takes j = 1 + l, 1 + l + 64, ...
    for (long long i = 1; i <= k; i++) {
        double part = 0.0;
        for (long long j = 1 + lane; j <= i; j += 64) part += s[j] * delta[i - j];
        const double d = wave_sum(part) / (double)i;
        if (lane == 0) delta[i] = d;
        __syncthreads();
    }
    const double ret = prefac * delta[k];
    if (ret != ret) return 1.0;               // fast_pgmix: NaN -> 1
    if (ret > GPLLH_TINY) return log(ret);    // (+inf stays +inf)
    if (ret >= 0.0) return log(GPLLH_TINY);
    return __longlong_as_double(0x7ff8000000000000LL);
}

// Called by every workgroup after its bin: lane 0 publishes the value; the last workgroup of the point to
// arrive adds all bins in a fixed order (lane l: bins l, l + 64, ... in sequence, then the butterfly) and
// resets the arrival counter for the next launch.
__device__ __forceinline__ void gpllh_publish_and_total(double v, int b, int n_bins, double *per_bin,
                                                        unsigned int *done, double *total) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        per_bin[b] = v;
        __threadfence();
        const unsigned prev = atomicAdd(done, 1u);
        s_last = prev == (unsigned)(n_bins - 1);
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_bins; i += 64)
        acc += __hip_atomic_load(per_bin + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
        total[0] = acc;   // np.sum: NaN and inf propagate
        *done = 0u;
    }
}

__host__ __device__ inline int64_t gpllh_lds_k(int64_t cap) { return cap < PISA_HIP_GPLLH_LDS_K ? cap : PISA_HIP_GPLLH_LDS_K; }

inline size_t gpllh_lds_bytes(int n_cont, int64_t cap) {
    return (size_t)(4 * n_cont + 2 * (gpllh_lds_k(cap) + 1)) * sizeof(double);
}

}  // namespace pisa
