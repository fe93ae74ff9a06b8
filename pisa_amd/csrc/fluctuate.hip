// fluctuate.hip -- pseudo-data of a trial ensemble drawn on the device: out[t][b] ~ Poisson(mu[b]) for n_trials
// trials of one template row, from a counter-based generator (Philox4x32-10, Salmon et al., SC'11), and the other
// methods of `Map.fluctuate` (pisa/core/map.py:1118-1254): gauss, gauss+poisson and scaled_poisson, which also read
// the row's standard deviations (their definition: the head of fluctuate_device.hpp; a normal deviate per entry from
// the block (b, trial, stream, 0xFFFFFFFF) through AS 241, independent of the Poisson blocks).
// The reference draws `Map.fluctuate("poisson")` from a `RandomState` stream (pisa/core/map.py:1098-1254), which no
// counter-based generator reproduces; this is a generator of its own, defined here and in DESIGN.md §4, restated draw
// for draw in tests/fluctuate_cases.py and validated statistically (tests/test_host_fluctuate.py).
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (bin b, first_trial + t, stream, attempt j)
// so the value of entry (trial, bin) depends on (seed, stream, trial number, bin, mu[bin]) alone: not on the number of
// trials, on how they are split over calls (`first_trial`) or on the launch geometry -- the placement property of the
// metric kernels of ensemble.hip.  One Philox block is four words = two doubles in [0, 1):
//   u = ((w_a >> 5) * 2^26 + (w_b >> 6)) * 2^-53        from the pairs (w0, w1) and (w2, w3).
// Sampler, exact in distribution:
//   mu == 0 -> 0; NaN -> NaN, nothing drawn;
//   0 < mu < 10   inversion by sequential search on the first double of attempt 0:
//                 p = exp(-mu), cdf = p, k = 0; while (u >= cdf && k < 255) { k += 1; p *= mu / k; cdf += p; }
//                 (the cap: the rounded cdf can plateau below the largest u);
//   mu >= 10      Hoermann's transformed rejection PTRS (Insurance: Mathematics and Economics 12 (1993) 39-45, the
//                 algorithm numpy uses from 10 upwards), one Philox block per attempt, j = 0, 1, ... until accepted;
//   mu < 0, mu = +inf or mu > 2^52 -> NaN and PISA_HIP_ERR_NEGATIVE in the status word.
// One lane owns one entry; consecutive lanes take consecutive bins of a trial (coalesced stores, the mu row comes from
// L2).  The two sampler branches and the rejection loop are lane-dependent and there is no cross-lane operation
// anywhere in the kernel.  A workgroup takes 256 consecutive entries and strides over the rest, so neither n_trials
// nor n_bins is a grid dimension.  No -ffp-contract here (the Makefile's default): sqrt, division, multiplication and
// addition round as numpy's do, so only exp, log and lgamma can differ from the restatement.  The generator itself is
// in fluctuate_device.hpp (it also compiles for the host); the kernel and the entry point are here.
#include "common.hpp"
#include "fluctuate_device.hpp"

namespace pisa {

constexpr int FL_THREADS = 256;
constexpr int FL_MAX_BLOCKS = 2048;      // 2 workgroups per CU are resident (fluct_kernel: 2 wavefronts per SIMD)

// entry i = t n_bins + b; lane i0 of the grid takes the entries i0, i0 + step, ... with step = step_t n_bins + step_b
// (the number of lanes of the grid, split on the host), carried as (t, b) so that no 64-bit division runs here.
// One instantiation per method: `fl_fluctuate` folds to the method's own branch, and the Poisson one reads no sigma.
template <int METHOD>
__global__ void __launch_bounds__(FL_THREADS)
fluct_kernel(const double *__restrict__ mu, const double *__restrict__ sigma, uint32_t B, int64_t T, uint32_t k0,
             uint32_t k1, uint32_t stream, uint32_t first_trial, int64_t step_t, uint32_t step_b,
             double *__restrict__ out, int32_t *__restrict__ status) {
    const uint32_t i0 = blockIdx.x * (uint32_t)FL_THREADS + threadIdx.x;   // < FL_MAX_BLOCKS * FL_THREADS
    uint32_t b = i0 % B;
    int64_t t = (int64_t)(i0 / B);
    bool bad = false;
    while (t < T) {
        // first_trial + n_trials <= 2^32: the trial number fits the counter word
        const double sg = METHOD == FL_POISSON ? 0.0 : sigma[b];
        out[t * (int64_t)B + b] = fl_fluctuate(METHOD, mu[b], sg, b, first_trial + (uint32_t)t, stream, k0, k1, bad);
        b += step_b;   // (< 2 B <= 2^32 - 2)
        t += step_t;
        if (b >= B) {
            b -= B;
            t++;
        }
    }
    if (bad) status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
}

static_assert(FL_POISSON == PISA_HIP_FLUCT_POISSON && FL_SCALED_POISSON == PISA_HIP_FLUCT_SCALED_POISSON &&
                  FL_GAUSS == PISA_HIP_FLUCT_GAUSS && FL_GAUSS_POISSON == PISA_HIP_FLUCT_GAUSS_POISSON,
              "fluctuate_device.hpp and pisa_hip.h number the methods alike");

template <int METHOD>
static int fluct_launch(const double *d_mu, const double *d_sigma, int64_t n_bins, int64_t n_trials, uint64_t seed,
                        uint32_t stream_id, uint32_t first_trial, double *d_out, int32_t *d_status, void *stream) {
    // (with the limits of fluct_check n_trials * n_bins does not overflow int64)
    const int64_t entries = n_trials * n_bins;
    const int64_t want = (entries + FL_THREADS - 1) / FL_THREADS;
    const int64_t blocks = want < FL_MAX_BLOCKS ? want : FL_MAX_BLOCKS;
    const int64_t step = blocks * FL_THREADS;
    hipLaunchKernelGGL(fluct_kernel<METHOD>, dim3((unsigned)blocks), dim3(FL_THREADS), 0, as_stream(stream), d_mu,
                       d_sigma, (uint32_t)n_bins, n_trials, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                       stream_id, first_trial, step / n_bins, (uint32_t)(step % n_bins), d_out, d_status);
    PISA_CHECK_LAUNCH("fluct_kernel");
    return PISA_HIP_OK;
}

static bool fluct_check(const double *d_mu, const double *d_sigma, int32_t method, int64_t n_bins, int64_t n_trials,
                        uint32_t first_trial, const double *d_out, const int32_t *d_status) {
    if (!d_mu || !d_out || !d_status) return false;
    if (n_bins < 1 || n_trials < 1 || n_bins > 0x7FFFFFFF || n_trials > 0x7FFFFFFF) return false;
    if ((int64_t)first_trial + n_trials > ((int64_t)1 << 32)) return false;
    if (method < FL_POISSON || method > FL_GAUSS_POISSON) return false;
    return method == FL_POISSON || d_sigma;
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_fluctuate(const double *d_mu, const double *d_sigma, int32_t method, int64_t n_bins,
                                int64_t n_trials, uint64_t seed, uint32_t stream_id, uint32_t first_trial,
                                double *d_out, int32_t *d_status, void *stream) {
    if (!fluct_check(d_mu, d_sigma, method, n_bins, n_trials, first_trial, d_out, d_status))
        return PISA_HIP_ERR_INVALID;
    return dispatch_int<FL_POISSON, FL_SCALED_POISSON, FL_GAUSS, FL_GAUSS_POISSON>(method, [&](auto m) {
        return fluct_launch<decltype(m)::value>(d_mu, d_sigma, n_bins, n_trials, seed, stream_id, first_trial, d_out,
                                                d_status, stream);
    });
}

PISA_API int pisa_hip_poisson_fluctuate(const double *d_mu, int64_t n_bins, int64_t n_trials, uint64_t seed,
                                        uint32_t stream_id, uint32_t first_trial, double *d_out, int32_t *d_status,
                                        void *stream) {
    return pisa_hip_fluctuate(d_mu, nullptr, FL_POISSON, n_bins, n_trials, seed, stream_id, first_trial, d_out,
                              d_status, stream);
}
