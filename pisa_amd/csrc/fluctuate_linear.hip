// fluctuate_linear.hip -- pseudo-data of a trial ensemble whose nuisance parameters fluctuate: the template of the
// true point is linearised in J <= 8 parameters, mu(eta) = mu0 + sum_j R[j] eta_j (the template the profiled fit of
// profile.hip works with), every trial draws its own truths eta from the parameters' priors -- a normal of the
// parameter's scale about its shift, truncated to the parameter's box --, and the trial's data are drawn from
// mu(eta) by the poisson, gauss or gauss+poisson method of fluctuate.hip: the prior-predictive (Cousins-Highland)
// ensemble.  The definition: the two functions at the end of fluctuate_device.hpp, DESIGN.md §4 ("pseudo-data with
// drawn nuisance truths"), restated draw for draw in tests/truth_cases.py.
//   truth   eta[t][j] = fl_truth: the first of shift_j + scale_j z_r inside [lower_j, upper_j], z_r from the block
//           (0x80000000 + j, first_trial + t, stream, r); scale_j == 0 gives shift_j and draws nothing
//   mean    mu_t[b] = mu0[b] + R[0][b] eta[t][0] + ... in ascending j, every step rounded; negative -> 0, counted
//   entry   fl_fluctuate(method, mu_t[b], sigma[b], b, first_trial + t, stream, key): the blocks of fluctuate.hip
// so entry (t, b) depends on (seed, stream, trial number, bin, the inputs) alone, as there.  scaled_poisson has no
// such form: its row rules compare a row's variance with its mean, and the mean moves per trial.
// Two launches on the caller's stream.  truth_kernel: one lane per (t, j), the parameters' four numbers in the
// kernel's arguments.  linear_kernel has the shape of fluct_kernel (one lane per entry, consecutive lanes on
// consecutive bins, a workgroup strides over the entries): a lane reads its trial's J truths (one address per
// wavefront unless the wavefront crosses a row's end) and its bin's J responses (coalesced, from L2), and there is
// no cross-lane operation.  The number of clipped means is the one thing the lanes share: a lane that clipped adds
// its own count to the word with ONE atomic after its last entry -- integer addition, so the word does not depend on
// the order --, and a lane that clipped nothing (every lane of an ordinary call) touches nothing.
// pisa_hip_fluctuate_linear_mvn is the same call with CORRELATED truths, those of a fit to an observed map: eta[t] ~
// N(mean, cov) inside the box by rejection of the whole vector (fl_truth_factor, fl_truth_mvn; DESIGN.md §4,
// "pseudo-data at nuisances fitted to the observed data"; tests/observed_cases.py).  truth_mvn_kernel, one lane per
// trial, takes the place of truth_kernel; linear_kernel runs unchanged on its truths.
// pisa_hip_fluctuate_linear_at has no truth launch at all: the truths are an input [n_trials][J] on the device (rows
// of a posterior sample of posterior.hip, for one), and linear_kernel runs unchanged on them.
#include "common.hpp"
#include "fluctuate_device.hpp"

namespace pisa {

constexpr int FLL_THREADS = 256;
constexpr int FLL_MAX_BLOCKS = 2048;
constexpr int FLL_MAX_PARAMS = PISA_HIP_PROFILE_MAX_PARAMS;

struct TruthPriors {
    double scale[FLL_MAX_PARAMS], shift[FLL_MAX_PARAMS], lower[FLL_MAX_PARAMS], upper[FLL_MAX_PARAMS];
};

// pair i = t J + j; lane i0 takes the pairs i0, i0 + lanes of the grid, ...
__global__ void __launch_bounds__(FLL_THREADS)
truth_kernel(TruthPriors p, uint32_t J, int64_t pairs, uint32_t k0, uint32_t k1, uint32_t stream,
             uint32_t first_trial, double *__restrict__ eta, int32_t *__restrict__ status) {
    bool exhausted = false;
    const int64_t step = (int64_t)gridDim.x * FLL_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * FLL_THREADS + threadIdx.x; i < pairs; i += step) {
        const uint32_t j = (uint32_t)(i % J);
        const uint32_t t = (uint32_t)(i / J);   // (< n_trials <= 2^31 - 1)
        eta[i] = fl_truth(j, first_trial + t, stream, k0, k1, p.scale[j], p.shift[j], p.lower[j], p.upper[j],
                          exhausted);
    }
    if (exhausted) status[0] = PISA_HIP_FLUCT_TRUTH_EXHAUSTED;   // (every writer stores the same word)
}

// the entries as fluct_kernel deals them: entry i = t B + b, carried as (t, b)
template <int METHOD>
__global__ void __launch_bounds__(FLL_THREADS)
linear_kernel(const double *__restrict__ mu0, const double *__restrict__ sigma, const double *__restrict__ R,
              const double *__restrict__ eta, int J, uint32_t B, int64_t T, uint32_t k0, uint32_t k1,
              uint32_t stream, uint32_t first_trial, int64_t step_t, uint32_t step_b, double *__restrict__ out,
              int32_t *__restrict__ status) {
    const uint32_t i0 = blockIdx.x * (uint32_t)FLL_THREADS + threadIdx.x;   // < FLL_MAX_BLOCKS * FLL_THREADS
    uint32_t b = i0 % B;
    int64_t t = (int64_t)(i0 / B);
    bool bad = false;
    uint32_t n_clipped = 0;
    while (t < T) {
        bool clipped;
        const double mu = fl_linear_mean(mu0[b], R + b, (int64_t)B, eta + t * J, J, clipped);
        n_clipped += clipped;
        const double sg = METHOD == FL_POISSON ? 0.0 : sigma[b];
        out[t * (int64_t)B + b] = fl_fluctuate(METHOD, mu, sg, b, first_trial + (uint32_t)t, stream, k0, k1, bad);
        b += step_b;   // (< 2 B <= 2^32 - 2)
        t += step_t;
        if (b >= B) {
            b -= B;
            t++;
        }
    }
    if (bad) status[0] = PISA_HIP_ERR_NEGATIVE;   // (after truth_kernel on the stream: the error code wins)
    if (n_clipped) atomicAdd((unsigned int *)(status + 1), n_clipped);
}

template <int METHOD>
static int linear_launch(const double *d_mu, const double *d_sigma, const double *d_response, int32_t n_params,
                         int64_t n_bins, int64_t n_trials, uint64_t seed, uint32_t stream_id, uint32_t first_trial,
                         double *d_out, const double *d_eta, int32_t *d_status, void *stream) {
    const int64_t entries = n_trials * n_bins;
    const int64_t want = (entries + FLL_THREADS - 1) / FLL_THREADS;
    const int64_t blocks = want < FLL_MAX_BLOCKS ? want : FLL_MAX_BLOCKS;
    const int64_t step = blocks * FLL_THREADS;
    hipLaunchKernelGGL(linear_kernel<METHOD>, dim3((unsigned)blocks), dim3(FLL_THREADS), 0, as_stream(stream), d_mu,
                       d_sigma, d_response, d_eta, (int)n_params, (uint32_t)n_bins, n_trials,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), stream_id, first_trial, step / n_bins,
                       (uint32_t)(step % n_bins), d_out, d_status);
    PISA_CHECK_LAUNCH("linear_kernel");
    return PISA_HIP_OK;
}

// the parameters' numbers checked and copied: scale finite and >= 0, shift finite, lower <= upper (no NaN)
static bool truth_priors(int32_t n_params, const double *h_scale, const double *h_shift, const double *h_lower,
                         const double *h_upper, TruthPriors &p) {
    if (n_params < 1 || n_params > FLL_MAX_PARAMS || !h_scale || !h_shift) return false;
    for (int j = 0; j < FLL_MAX_PARAMS; j++) {
        const bool live = j < n_params;
        p.scale[j] = live ? h_scale[j] : 0.0;
        p.shift[j] = live ? h_shift[j] : 0.0;
        p.lower[j] = live && h_lower ? h_lower[j] : -INFINITY;
        p.upper[j] = live && h_upper ? h_upper[j] : INFINITY;
        if (!(p.scale[j] >= 0.0 && p.scale[j] <= 1.7976931348623157e308)) return false;
        if (!(fabs(p.shift[j]) <= 1.7976931348623157e308)) return false;
        if (!(p.lower[j] <= p.upper[j])) return false;
    }
    return true;
}

// ---- truths from a fit's Gaussian: pisa_hip_fluctuate_linear_mvn ----
// The truths of a trial are correlated, so a lane takes a whole trial: J Philox blocks and a J x J triangle of
// multiply-adds per attempt, everything in registers, nothing shared between lanes.  The mean, the box and the factor
// L (computed once per launch on the host by fl_truth_factor) are the kernel's arguments.
struct TruthMvn {
    double mean[FL_MVN_MAX], lower[FL_MVN_MAX], upper[FL_MVN_MAX], L[FL_MVN_MAX * FL_MVN_MAX];
};

static_assert(FL_MVN_MAX == FLL_MAX_PARAMS, "one limit on the number of parameters");

// lane i0 takes the trials i0, i0 + lanes of the grid, ...
__global__ void __launch_bounds__(FLL_THREADS)
truth_mvn_kernel(TruthMvn p, int J, int64_t T, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t first_trial,
                 double *__restrict__ eta, int32_t *__restrict__ status) {
    bool exhausted = false;
    const int64_t step = (int64_t)gridDim.x * FLL_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * FLL_THREADS + threadIdx.x; t < T; t += step) {
        double x[FL_MVN_MAX];
        fl_truth_mvn(first_trial + (uint32_t)t, stream, k0, k1, p.mean, p.L, J, p.lower, p.upper, x, exhausted);
#pragma unroll
        for (int j = 0; j < FL_MVN_MAX; j++)
            if (j < J) eta[t * J + j] = x[j];
    }
    if (exhausted) status[0] = PISA_HIP_FLUCT_TRUTH_EXHAUSTED;   // (every writer stores the same word)
}

// the fit's numbers checked and copied: the mean finite and inside its box, lower <= upper (no NaN), a factor of cov
static bool truth_mvn(int32_t n_params, const double *h_mean, const double *h_cov, const double *h_lower,
                      const double *h_upper, TruthMvn &p) {
    if (n_params < 1 || n_params > FLL_MAX_PARAMS || !h_mean || !h_cov) return false;
    for (int j = 0; j < FL_MVN_MAX; j++) {
        const bool live = j < n_params;
        p.mean[j] = live ? h_mean[j] : 0.0;
        p.lower[j] = live && h_lower ? h_lower[j] : -INFINITY;
        p.upper[j] = live && h_upper ? h_upper[j] : INFINITY;
        if (!(fabs(p.mean[j]) <= 1.7976931348623157e308)) return false;
        if (!(p.lower[j] <= p.mean[j] && p.mean[j] <= p.upper[j])) return false;
    }
    return fl_truth_factor(h_cov, n_params, p.L);
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_fluctuate_linear(const double *d_mu, const double *d_sigma, const double *d_response,
                                       int32_t n_params, const double *h_scale, const double *h_shift,
                                       const double *h_lower, const double *h_upper, int32_t method, int64_t n_bins,
                                       int64_t n_trials, uint64_t seed, uint32_t stream_id, uint32_t first_trial,
                                       double *d_out, double *d_eta_true, int32_t *d_status, void *stream) {
    if (!d_mu || !d_response || !d_out || !d_eta_true || !d_status) return PISA_HIP_ERR_INVALID;
    if (n_bins < 1 || n_trials < 1 || n_bins > 0x7FFFFFFF || n_trials > 0x7FFFFFFF) return PISA_HIP_ERR_INVALID;
    if ((int64_t)first_trial + n_trials > ((int64_t)1 << 32)) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && method != FL_GAUSS && method != FL_GAUSS_POISSON) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && !d_sigma) return PISA_HIP_ERR_INVALID;
    TruthPriors p;
    if (!truth_priors(n_params, h_scale, h_shift, h_lower, h_upper, p)) return PISA_HIP_ERR_INVALID;

    const int64_t pairs = n_trials * n_params;
    const int64_t want = (pairs + FLL_THREADS - 1) / FLL_THREADS;
    const int64_t blocks = want < FLL_MAX_BLOCKS ? want : FLL_MAX_BLOCKS;
    hipLaunchKernelGGL(truth_kernel, dim3((unsigned)blocks), dim3(FLL_THREADS), 0, as_stream(stream), p,
                       (uint32_t)n_params, pairs, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), stream_id,
                       first_trial, d_eta_true, d_status);
    PISA_CHECK_LAUNCH("truth_kernel");
    return dispatch_int<FL_POISSON, FL_GAUSS, FL_GAUSS_POISSON>(method, [&](auto m) {
        return linear_launch<decltype(m)::value>(d_mu, d_sigma, d_response, n_params, n_bins, n_trials, seed,
                                                 stream_id, first_trial, d_out, d_eta_true, d_status, stream);
    });
}

// the call above without the truth launch: the truths are the caller's, d_eta [n_trials][J] on the device
PISA_API int pisa_hip_fluctuate_linear_at(const double *d_mu, const double *d_sigma, const double *d_response,
                                          int32_t n_params, const double *d_eta, int32_t method, int64_t n_bins,
                                          int64_t n_trials, uint64_t seed, uint32_t stream_id, uint32_t first_trial,
                                          double *d_out, int32_t *d_status, void *stream) {
    if (!d_mu || !d_response || !d_out || !d_eta || !d_status) return PISA_HIP_ERR_INVALID;
    if (n_params < 1 || n_params > FLL_MAX_PARAMS) return PISA_HIP_ERR_INVALID;
    if (n_bins < 1 || n_trials < 1 || n_bins > 0x7FFFFFFF || n_trials > 0x7FFFFFFF) return PISA_HIP_ERR_INVALID;
    if ((int64_t)first_trial + n_trials > ((int64_t)1 << 32)) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && method != FL_GAUSS && method != FL_GAUSS_POISSON) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && !d_sigma) return PISA_HIP_ERR_INVALID;
    return dispatch_int<FL_POISSON, FL_GAUSS, FL_GAUSS_POISSON>(method, [&](auto m) {
        return linear_launch<decltype(m)::value>(d_mu, d_sigma, d_response, n_params, n_bins, n_trials, seed,
                                                 stream_id, first_trial, d_out, d_eta, d_status, stream);
    });
}

PISA_API int pisa_hip_fluctuate_linear_mvn(const double *d_mu, const double *d_sigma, const double *d_response,
                                           int32_t n_params, const double *h_mean, const double *h_cov,
                                           const double *h_lower, const double *h_upper, int32_t method,
                                           int64_t n_bins, int64_t n_trials, uint64_t seed, uint32_t stream_id,
                                           uint32_t first_trial, double *d_out, double *d_eta_true, int32_t *d_status,
                                           void *stream) {
    if (!d_mu || !d_response || !d_out || !d_eta_true || !d_status) return PISA_HIP_ERR_INVALID;
    if (n_bins < 1 || n_trials < 1 || n_bins > 0x7FFFFFFF || n_trials > 0x7FFFFFFF) return PISA_HIP_ERR_INVALID;
    if ((int64_t)first_trial + n_trials > ((int64_t)1 << 32)) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && method != FL_GAUSS && method != FL_GAUSS_POISSON) return PISA_HIP_ERR_INVALID;
    if (method != FL_POISSON && !d_sigma) return PISA_HIP_ERR_INVALID;
    TruthMvn p;
    if (!truth_mvn(n_params, h_mean, h_cov, h_lower, h_upper, p)) return PISA_HIP_ERR_INVALID;

    const int64_t want = (n_trials + FLL_THREADS - 1) / FLL_THREADS;
    const int64_t blocks = want < FLL_MAX_BLOCKS ? want : FLL_MAX_BLOCKS;
    hipLaunchKernelGGL(truth_mvn_kernel, dim3((unsigned)blocks), dim3(FLL_THREADS), 0, as_stream(stream), p,
                       (int)n_params, n_trials, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), stream_id,
                       first_trial, d_eta_true, d_status);
    PISA_CHECK_LAUNCH("truth_mvn_kernel");
    return dispatch_int<FL_POISSON, FL_GAUSS, FL_GAUSS_POISSON>(method, [&](auto m) {
        return linear_launch<decltype(m)::value>(d_mu, d_sigma, d_response, n_params, n_bins, n_trials, seed,
                                                 stream_id, first_trial, d_out, d_eta_true, d_status, stream);
    });
}
