// fisher.hip -- the Fisher matrix and pull vector of a set of templates (pisa/utils/fisher_matrix.py
// build_fisher_matrix :41-75, pisa/utils/pull_method.py get_derivative_map :48-86 and calculate_pulls :131-193).
//   fisher_kernel   totals of the points -> per-bin gradients -> F_ij and d_p, one workgroup
// Bins are taken in chunks staged in LDS: every thread first forms the totals, the std dev and the gradients of
// some bins of the chunk (parallel over bins), then every matrix entry / pull component runs its OWN sequential
// chain over the chunk's bins in ascending order, its accumulator carried in a register from chunk to chunk.  One
// chain per entry is the reference's loop order (fmatrix += np.outer(g, g) / sigma, bin after bin); a tree over the
// bins would round differently.
#include "common.hpp"

#include <math.h>

namespace pisa {

constexpr int FISHER_THREADS = 256;
constexpr int FISHER_LDS_BUDGET = 48 * 1024;
// matrix entries (i <= j) and pull components per thread
constexpr int FISHER_ITEMS =
    (PISA_HIP_FISHER_MAX_PARAMS * (PISA_HIP_FISHER_MAX_PARAMS + 1) / 2 + PISA_HIP_FISHER_MAX_PARAMS +
     FISHER_THREADS - 1) / FISHER_THREADS;

struct FisherPairs {
    int32_t lo[PISA_HIP_FISHER_MAX_PARAMS];
    int32_t hi[PISA_HIP_FISHER_MAX_PARAMS];
    double dx[PISA_HIP_FISHER_MAX_PARAMS];
};

// bins per chunk: [n_params] gradients + std dev + truth - fiducial per bin, and a nonempty flag
inline int fisher_chunk(int n_params) {
    int c = FISHER_LDS_BUDGET / (8 * (n_params + 2) + 1);
    c = c / 64 * 64;
    return c > 512 ? 512 : (c < 64 ? 64 : c);
}

inline size_t fisher_lds_bytes(int n_params, int chunk) {
    return (size_t)chunk * (8 * (n_params + 2)) + (size_t)chunk;
}

// the total of point `pt` in bin b: rows added in ascending index order, starting from row 0
// (MapSet.total() / DeviceMapBlock.host_sum)
__device__ __forceinline__ double fisher_total(const double *__restrict__ x, int pt, int n_rows, int64_t n_bins,
                                               int64_t b) {
    const double *p = x + (int64_t)pt * n_rows * n_bins + b;
    double s = p[0];
    for (int r = 1; r < n_rows; r++) s += p[(int64_t)r * n_bins];
    return s;
}

__global__ void __launch_bounds__(FISHER_THREADS)
fisher_kernel(const double *__restrict__ hist, const double *__restrict__ sumw2, int n_points, int n_rows,
              int64_t n_bins, int n_params, FisherPairs pr, int chunk, const double *__restrict__ truth,
              double *__restrict__ grad, double *__restrict__ matrix, double *__restrict__ pull,
              double *__restrict__ totals, double *__restrict__ var0, int64_t *__restrict__ nonempty,
              int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double *s_g = s_lds;                                     // [n_params][chunk]
    double *s_sig = s_lds + (size_t)n_params * chunk;        // [chunk]
    double *s_dm = s_sig + chunk;                            // [chunk]
    unsigned char *s_ne = (unsigned char *)(s_dm + chunk);   // [chunk]
    __shared__ unsigned long long s_count;
    __shared__ int s_bad;
    if (threadIdx.x == 0) {
        s_count = 0;
        s_bad = 0;
    }
    const int n_pairs = n_params * (n_params + 1) / 2;
    const int n_items = n_pairs + (truth ? n_params : 0);
    // item q < n_pairs: entry (i, j), i <= j, row-major over the upper triangle; else pull component q - n_pairs
    int it_a[FISHER_ITEMS], it_b[FISHER_ITEMS];
    double acc[FISHER_ITEMS];
#pragma unroll
    for (int k = 0; k < FISHER_ITEMS; k++) {
        const int q = (int)threadIdx.x + k * FISHER_THREADS;
        acc[k] = 0.0;
        it_a[k] = it_b[k] = -1;
        if (q < n_pairs) {
            int i = 0, r = q;
            while (r >= n_params - i) {
                r -= n_params - i;
                i++;
            }
            it_a[k] = i;
            it_b[k] = i + r;
        } else if (q < n_items) {
            it_a[k] = q - n_pairs;
        }
    }
    unsigned long long count = 0;
    int bad = 0;
    __syncthreads();
    for (int64_t c0 = 0; c0 < n_bins; c0 += chunk) {
        const int nb = (int)(n_bins - c0 < chunk ? n_bins - c0 : chunk);
        for (int t = threadIdx.x; t < nb; t += FISHER_THREADS) {
            const int64_t b = c0 + t;
            const double t0 = fisher_total(hist, 0, n_rows, n_bins, b);
            const double v = fisher_total(sumw2, 0, n_rows, n_bins, b);
            const double sig = sqrt(v);   // Map.std_devs (correctly rounded)
            if (var0) var0[b] = v;
            if (totals) {
                totals[b] = t0;
                for (int pt = 1; pt < n_points; pt++) totals[(int64_t)pt * n_bins + b] = fisher_total(hist, pt, n_rows, n_bins, b);
            }
            for (int p = 0; p < n_params; p++) {
                const double lo = pr.lo[p] == 0 ? t0 : fisher_total(hist, pr.lo[p], n_rows, n_bins, b);
                const double hi = pr.hi[p] == 0 ? t0 : fisher_total(hist, pr.hi[p], n_rows, n_bins, b);
                const double g = (hi - lo) / pr.dx[p];   // get_derivative_map: a true division
                grad[(int64_t)p * n_bins + b] = g;
                s_g[(size_t)p * chunk + t] = g;
            }
            const bool ne = t0 != 0.0;   // np.nonzero of the fiducial total
            s_sig[t] = sig;
            s_ne[t] = ne ? 1 : 0;
            s_dm[t] = truth ? truth[b] - t0 : 0.0;
            if (ne) {
                count++;
                if (sig == 0.0) bad = 1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FISHER_ITEMS; k++) {
            const int q = (int)threadIdx.x + k * FISHER_THREADS;
            if (q >= n_items) continue;
            double a = acc[k];
            const double *gi = s_g + (size_t)it_a[k] * chunk;
            if (q < n_pairs) {
                const double *gj = s_g + (size_t)it_b[k] * chunk;
                // fmatrix += np.outer(g, g) / sigma: the quotients of several bins are independent, the sum is one chain
#pragma unroll 8
                for (int t = 0; t < nb; t++) {
                    const double x = (gi[t] * gj[t]) / s_sig[t];
                    if (s_ne[t]) a += x;
                }
            } else {
                // calculate_pulls: (dm * g) / sigma, summed in bin order
#pragma unroll 8
                for (int t = 0; t < nb; t++) {
                    const double x = (s_dm[t] * gi[t]) / s_sig[t];
                    if (s_ne[t]) a += x;
                }
            }
            acc[k] = a;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < FISHER_ITEMS; k++) {
        const int q = (int)threadIdx.x + k * FISHER_THREADS;
        if (q < n_pairs) {
            matrix[it_a[k] * n_params + it_b[k]] = acc[k];
            matrix[it_b[k] * n_params + it_a[k]] = acc[k];   // exactly symmetric
        } else if (q < n_items) {
            pull[it_a[k]] = acc[k];
        }
    }
    if (count) atomicAdd(&s_count, count);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        nonempty[0] = (int64_t)s_count;
        status[0] = s_bad ? PISA_HIP_FISHER_ZERO_SIGMA : 0;
    }
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_fisher(const double *d_hist, const double *d_sumw2, int32_t n_points, int32_t n_rows,
                             int64_t n_bins, int32_t n_params, const int32_t *h_lo, const int32_t *h_hi,
                             const double *h_dx, const double *d_truth, double *d_grad, double *d_matrix,
                             double *d_pull, double *d_totals, double *d_var0, int64_t *d_nonempty,
                             int32_t *d_status, void *stream) {
    if (!d_hist || !d_sumw2 || !d_grad || !d_matrix || !d_nonempty || !d_status || !h_lo || !h_hi || !h_dx)
        return PISA_HIP_ERR_INVALID;
    if ((d_truth == nullptr) != (d_pull == nullptr)) return PISA_HIP_ERR_INVALID;
    if (n_points < 1 || n_rows < 1 || n_bins < 1 || n_bins > 0x7FFFFFFF) return PISA_HIP_ERR_INVALID;
    if ((int64_t)n_points * n_rows > ((int64_t)1 << 62) / n_bins) return PISA_HIP_ERR_INVALID;
    if (n_params < 1 || n_params > PISA_HIP_FISHER_MAX_PARAMS) return PISA_HIP_ERR_INVALID;
    FisherPairs pr;
    for (int p = 0; p < n_params; p++) {
        if (h_lo[p] < 0 || h_lo[p] >= n_points || h_hi[p] < 0 || h_hi[p] >= n_points) return PISA_HIP_ERR_INVALID;
        if (h_dx[p] == 0.0 || !isfinite(h_dx[p])) return PISA_HIP_ERR_INVALID;
        pr.lo[p] = h_lo[p];
        pr.hi[p] = h_hi[p];
        pr.dx[p] = h_dx[p];
    }
    for (int p = n_params; p < PISA_HIP_FISHER_MAX_PARAMS; p++) {
        pr.lo[p] = pr.hi[p] = 0;
        pr.dx[p] = 1.0;
    }
    const int chunk = fisher_chunk(n_params);
    hipLaunchKernelGGL(fisher_kernel, dim3(1), dim3(FISHER_THREADS), fisher_lds_bytes(n_params, chunk),
                       as_stream(stream), d_hist, d_sumw2, (int)n_points, (int)n_rows, n_bins, (int)n_params, pr,
                       chunk, d_truth, d_grad, d_matrix, d_pull, d_totals, d_var0, d_nonempty, d_status);
    PISA_CHECK_LAUNCH("fisher_kernel");
    return PISA_HIP_OK;
}
