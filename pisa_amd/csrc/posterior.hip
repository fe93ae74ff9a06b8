// posterior.hip -- samples of the posterior of the linearised nuisance displacements, p(eta | data row, template
// row): a Goodman-Weare stretch-move ensemble sampler, one chain ensemble per problem, all problems and all steps in
// ONE launch.  The definition -- log-density, counters, move, acceptance, what is kept -- is posterior_device.hpp
// ("Trial ensembles: the nuisance posterior"; restated in tests/posterior_cases.py).
//
// Mapping.  One lane per proposal: the H = W / 2 walkers of the half that moves.  A workgroup is 128 lanes and holds
// min(128 / H, 32) problems side by side (lane = problem * H + walker), so that W = 128 fills a wavefront per problem,
// W = 256 spans both wavefronts and small ensembles share them.  Walker positions and their lp live in LDS; a lane
// writes its own two walkers (h and H + h) and reads a partner of the half that stands still, and a workgroup barrier
// separates the two halves of a step and the steps.  No loop that holds a barrier depends on data: n_steps is one
// argument, and a problem that is refused at its start (or has no row) idles through the barriers.
// Rows.  A proposal's log-density is one sequential sweep over the bins by its lane (so Phi has the solver's bits).
// Where the rows of all problems of a workgroup -- data, expectation, sigma2 for mod_chi2, J responses -- fit the
// LDS stage of PS_STAGE doubles they are copied there once, before the first step, and every sweep reads LDS (all
// lanes of a problem read one address: a broadcast).  Larger rows are streamed from global memory / L2 by every
// sweep; the lanes of a problem still read one address per load.  The arithmetic is the same expression either way.
#include "common.hpp"
#include "ensemble_device.hpp"
#include "posterior_device.hpp"

namespace pisa {

static_assert(PF_MAX_PARAMS == PISA_HIP_PROFILE_MAX_PARAMS && PF_START_OUTSIDE == PISA_HIP_PROFILE_START_OUTSIDE &&
                  PF_BAD_BOUNDS == PISA_HIP_PROFILE_BAD_BOUNDS && PS_MAX_WALKERS == PISA_HIP_POSTERIOR_MAX_WALKERS,
              "posterior_device.hpp and pisa_hip.h disagree");

constexpr int PS_THREADS = 128;    // two wavefronts
constexpr int PS_MAX_NP = 32;      // problems of a workgroup at most (their centres and boxes are kept in LDS)
constexpr int PS_STAGE = 4096;     // doubles of the LDS stage (32 KiB)
static_assert(2 * PS_THREADS == PS_MAX_WALKERS, "a lane owns two walkers");

struct PsArgs {
    const double *D, *E, *S2, *R, *ips, *center, *lower, *upper, *x0;
    const int32_t *t_of, *k_of;
    const uint32_t *chain_id;
    int64_t r_stride_k, b_stride_k, B, P, n_steps, first_step, keep_from, thin, n_keep;
    int T, K, W, np_blk, staged;
    uint32_t k0, k1, stream_id;
    double *chain, *logp, *x_end;
    int32_t *accepted, *problem_status, *status;
};

// lp at eta: one sweep over the bins of rows d, e, s2 and r[j * r_row + b]
template <int KIND, int J>
__device__ __forceinline__ double ps_logp(const double *d, const double *e, const double *s2, const double *r,
                                          int64_t r_row, int64_t B, const double *eta, const double *ips,
                                          const double *c, const double *lo, const double *hi) {
    PsSweep sw;
    ps_begin(sw);
    // (four bins in flight: their loads and logs are independent, only the compensated chain is sequential, and a
    // workgroup has one wavefront per SIMD, so nothing else hides the latencies)
#pragma unroll 4
    for (int64_t b = 0; b < B; b++) {
        double rb[J];
#pragma unroll
        for (int j = 0; j < J; j++) rb[j] = r[j * r_row + b];
        ps_bin<KIND, J>(sw, eta, d[b], e[b], KIND == PF_MOD_CHI2 ? s2[b] : 0.0, rb);
    }
    return ps_end<KIND, J>(sw, eta, ips, c, lo, hi);
}

template <int KIND, int J>
__global__ void __launch_bounds__(PS_THREADS)
posterior_kernel(const PsArgs a) {
    constexpr bool WITH_S2 = KIND == PF_MOD_CHI2;
    constexpr int ROWS = J + 2 + (WITH_S2 ? 1 : 0);
    __shared__ double sX[PS_MAX_WALKERS * J];
    __shared__ double sLp[PS_MAX_WALKERS];
    __shared__ double sStage[PS_STAGE];
    __shared__ double sIps[J];
    __shared__ double sPar[PS_MAX_NP * 3 * J];   // per problem: centre, lower, upper [J] each
    __shared__ int sT[PS_MAX_NP], sK[PS_MAX_NP], sFlag[PS_MAX_NP];
    const int lane = (int)threadIdx.x, W = a.W, H = W / 2, np = a.np_blk;
    const int pl = lane / H, h = lane - pl * H;
    const int64_t p = (int64_t)blockIdx.x * np + pl;
    const bool mine = pl < np && p < a.P;
    const int64_t B = a.B;

    // ---- the rows of the workgroup's problems
    if (lane < np) {
        const int64_t q = (int64_t)blockIdx.x * np + lane;
        int t = -1, k = -1, flag = -1;
        if (q < a.P) {
            const int64_t tq = a.t_of ? (int64_t)a.t_of[q] : q, kq = a.k_of ? (int64_t)a.k_of[q] : q;
            if (tq >= 0 && tq < a.T && kq >= 0 && kq < a.K) {
                t = (int)tq;
                k = (int)kq;
                flag = 0;
            } else {
                a.status[0] = PISA_HIP_ERR_INVALID;   // (no row to read: the call is refused, the problem is NaN)
            }
        }
        sT[lane] = t;
        sK[lane] = k;
        sFlag[lane] = flag;
    }
    if (lane < J) sIps[lane] = a.ips ? a.ips[lane] : 0.0;
    __syncthreads();
    for (int idx = lane; idx < np * J; idx += PS_THREADS) {
        const int q = idx / J, j = idx - q * J;
        const int64_t k = sK[q];
        double c = 0.0, lo = -INFINITY, hi = INFINITY;
        if (k >= 0) {
            if (a.center) c = a.center[k * J + j];
            if (a.lower) lo = a.lower[k * a.b_stride_k + j];
            if (a.upper) hi = a.upper[k * a.b_stride_k + j];
        }
        sPar[(q * 3 + 0) * J + j] = c;
        sPar[(q * 3 + 1) * J + j] = lo;
        sPar[(q * 3 + 2) * J + j] = hi;
    }
    if (a.staged) {
        const int nb = (int)B, per = ROWS * nb;   // (np * per <= PS_STAGE)
        for (int idx = lane; idx < np * per; idx += PS_THREADS) {
            const int q = idx / per, rem = idx - q * per, row = rem / nb, b = rem - row * nb;
            const int64_t t = sT[q], k = sK[q];
            double v = 0.0;
            if (k >= 0) {
                if (row == 0)
                    v = a.D[t * B + b];
                else if (row == 1)
                    v = a.E[k * B + b];
                else if (WITH_S2 && row == 2)
                    v = a.S2[k * B + b];
                else
                    v = a.R[k * a.r_stride_k + (int64_t)(row - (ROWS - J)) * B + b];
            }
            sStage[idx] = v;
        }
    }
    __syncthreads();

    // ---- this lane's problem
    const int slot = pl * W;   // of the problem's walker 0 in sX / sLp (read where `mine`)
    const double *const cen = sPar + (pl * 3 + 0) * J, *const lo = sPar + (pl * 3 + 1) * J,
                 *const hi = sPar + (pl * 3 + 2) * J;
    const int64_t t_p = mine ? sT[pl] : -1, k_p = mine ? sK[pl] : -1;
    const bool has_rows = mine && k_p >= 0;
    const double *const gD = a.D + (has_rows ? t_p * B : 0), *const gE = a.E + (has_rows ? k_p * B : 0);
    const double *const gS2 = WITH_S2 ? a.S2 + (has_rows ? k_p * B : 0) : nullptr;
    const double *const gR = a.R + (has_rows ? k_p * a.r_stride_k : 0);
    const double *const lD = sStage + (int64_t)pl * ROWS * B, *const lE = lD + B, *const lS2 = lE + B,
                 *const lR = lD + (int64_t)(ROWS - J) * B;
    auto logp_at = [&](const double *eta) {
        return a.staged ? ps_logp<KIND, J>(lD, lE, lS2, lR, B, B, eta, sIps, cen, lo, hi)
                        : ps_logp<KIND, J>(gD, gE, gS2, gR, B, B, eta, sIps, cen, lo, hi);
    };
    int n_free = 0;
    if (has_rows) {
        const bool box_ok = ps_box<J>(lo, hi, n_free);
        if (!box_ok) {
            atomicOr(&sFlag[pl], PF_BAD_BOUNDS);
        } else {
            if (h == 0) {
                bool negative = false;
                for (int64_t b = 0; b < B; b++)
                    if (gD[b] < 0.0 || gE[b] < 0.0) negative = true;   // (a NaN compares false)
                if (negative) a.status[0] = PISA_HIP_ERR_NEGATIVE;     // (every writer stores the same word)
            }
#pragma unroll 1
            for (int half = 0; half < 2; half++) {
                const int w = half * H + h;
                double x[J];
#pragma unroll
                for (int j = 0; j < J; j++) {
                    x[j] = a.x0[(p * W + w) * J + j];
                    sX[(slot + w) * J + j] = x[j];
                }
                const double lp = logp_at(x);
                sLp[slot + w] = lp;
                if (lp != lp || lp == -INFINITY) atomicOr(&sFlag[pl], PF_START_OUTSIDE);
            }
        }
    }
    __syncthreads();
    const bool alive = has_rows && sFlag[pl] == 0;
    const uint32_t chain = mine ? (a.chain_id ? a.chain_id[p] : (uint32_t)p) : 0u;
    int32_t n_acc[2] = {0, 0};
    int64_t i_keep = 0;

    // ---- the steps
    for (int64_t i = 0; i < a.n_steps; i++) {
        const int64_t s = a.first_step + i;
#pragma unroll 1
        for (int half = 0; half < 2; half++) {
            if (alive) {
                const int w = half * H + h;
                double u_z, u_p, u_a;
                ps_uniforms((uint32_t)w, (uint32_t)s, a.stream_id, chain, a.k0, a.k1, u_z, u_p, u_a);
                const double z = ps_stretch(u_z);
                const int partner = (1 - half) * H + ps_partner(u_p, H);
                double x[J], c[J], y[J];
#pragma unroll
                for (int j = 0; j < J; j++) {
                    x[j] = sX[(slot + w) * J + j];
                    c[j] = sX[(slot + partner) * J + j];
                }
                ps_propose<J>(x, c, z, y);
                const double lp_y = logp_at(y);
                if (ps_accept(u_a, z, n_free, lp_y, sLp[slot + w])) {
#pragma unroll
                    for (int j = 0; j < J; j++) sX[(slot + w) * J + j] = y[j];
                    sLp[slot + w] = lp_y;
                    n_acc[half]++;
                }
            }
            __syncthreads();   // the half that moved is the half that stands still next
        }
        if (ps_kept(s, a.keep_from, a.thin)) {
            if (mine) {
#pragma unroll 1
                for (int half = 0; half < 2; half++) {
                    const int w = half * H + h;   // (this lane's own walkers: it wrote them itself)
                    const int64_t o = (p * a.n_keep + i_keep) * W + w;
#pragma unroll
                    for (int j = 0; j < J; j++) a.chain[o * J + j] = alive ? sX[(slot + w) * J + j] : NAN;
                    a.logp[o] = alive ? sLp[slot + w] : NAN;
                }
            }
            i_keep++;
        }
    }
    if (!mine) return;
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
        const int w = half * H + h;
        a.accepted[p * W + w] = n_acc[half];
        if (a.x_end) {
#pragma unroll
            for (int j = 0; j < J; j++) a.x_end[(p * W + w) * J + j] = alive ? sX[(slot + w) * J + j] : NAN;
        }
    }
    if (h == 0) a.problem_status[p] = sFlag[pl];
}

template <int KIND, int J>
static int posterior_launch(PsArgs a, hipStream_t stream) {
    const int rows = J + 2 + (KIND == PF_MOD_CHI2 ? 1 : 0);
    a.staged = (int64_t)a.np_blk * rows * a.B <= PS_STAGE ? 1 : 0;
    const int64_t blocks = (a.P + a.np_blk - 1) / a.np_blk;
    hipLaunchKernelGGL((posterior_kernel<KIND, J>), dim3((unsigned)blocks), dim3(PS_THREADS), 0, stream, a);
    PISA_CHECK_LAUNCH("posterior_kernel");
    return PISA_HIP_OK;
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_posterior_sample(int32_t kind, const double *d_data, const double *d_expected,
                                       const double *d_sigma2, const double *d_response, int64_t response_stride_k,
                                       const double *d_inv_prior_sigma, const double *d_center, const double *d_lower,
                                       const double *d_upper, int64_t bound_stride_k, int32_t n_params,
                                       int64_t n_data, int64_t n_templates, int64_t n_bins, int64_t n_problems,
                                       const int32_t *d_t_of_problem, const int32_t *d_k_of_problem,
                                       const uint32_t *d_chain_id, int32_t n_walkers, const double *d_x0,
                                       uint64_t seed, uint32_t stream_id, int64_t first_step, int64_t n_steps,
                                       int64_t keep_from, int64_t thin, int64_t n_keep, double *d_chain,
                                       double *d_logp, int32_t *d_accepted, double *d_x_end,
                                       int32_t *d_problem_status, int32_t *d_status, void *stream) {
    if (kind < PISA_HIP_METRIC_LLH || kind > PISA_HIP_METRIC_MOD_CHI2) return PISA_HIP_ERR_INVALID;
    if (n_params < 1 || n_params > PISA_HIP_PROFILE_MAX_PARAMS) return PISA_HIP_ERR_INVALID;
    if (n_walkers < 2 || n_walkers > PS_MAX_WALKERS || (n_walkers & 1) || n_walkers < 2 * n_params)
        return PISA_HIP_ERR_INVALID;
    if (!ens_check_sizes(n_data, n_templates, n_bins) || !ens_check_sizes(n_problems, n_steps, 1))
        return PISA_HIP_ERR_INVALID;
    if (thin < 1 || first_step < 0 || keep_from < 0 || first_step > ((int64_t)1 << 32) ||
        first_step + n_steps > ((int64_t)1 << 32))
        return PISA_HIP_ERR_INVALID;
    if (n_keep != ps_n_keep(first_step, n_steps, keep_from, thin)) return PISA_HIP_ERR_INVALID;
    // the chain is the largest output: at most 2^40 bytes (n_keep <= n_steps < 2^31, a row is at most 2^14 bytes)
    const int64_t row_bytes = (int64_t)n_walkers * n_params * 8;
    if (n_keep > 0 && n_problems > (((int64_t)1 << 40) / row_bytes) / n_keep) return PISA_HIP_ERR_INVALID;
    if (!d_data || !d_expected || !d_response || !d_x0 || !d_accepted || !d_problem_status || !d_status)
        return PISA_HIP_ERR_INVALID;
    if (n_keep > 0 && (!d_chain || !d_logp)) return PISA_HIP_ERR_INVALID;
    if (kind == PISA_HIP_METRIC_MOD_CHI2 && !d_sigma2) return PISA_HIP_ERR_INVALID;
    if (response_stride_k != 0 && response_stride_k < (int64_t)n_params * n_bins) return PISA_HIP_ERR_INVALID;
    if ((d_lower || d_upper) && bound_stride_k != 0 && bound_stride_k < (int64_t)n_params) return PISA_HIP_ERR_INVALID;
    if (!d_t_of_problem && n_problems > n_data) return PISA_HIP_ERR_INVALID;
    if (!d_k_of_problem && n_problems > n_templates) return PISA_HIP_ERR_INVALID;
    PsArgs a{};
    a.D = d_data;
    a.E = d_expected;
    a.S2 = d_sigma2;
    a.R = d_response;
    a.ips = d_inv_prior_sigma;
    a.center = d_center;
    a.lower = d_lower;
    a.upper = d_upper;
    a.x0 = d_x0;
    a.t_of = d_t_of_problem;
    a.k_of = d_k_of_problem;
    a.chain_id = d_chain_id;
    a.r_stride_k = response_stride_k;
    a.b_stride_k = bound_stride_k;
    a.B = n_bins;
    a.P = n_problems;
    a.n_steps = n_steps;
    a.first_step = first_step;
    a.keep_from = keep_from;
    a.thin = thin;
    a.n_keep = n_keep;
    a.T = (int)n_data;
    a.K = (int)n_templates;
    a.W = n_walkers;
    const int per = PS_THREADS / (n_walkers / 2);
    a.np_blk = per < PS_MAX_NP ? per : PS_MAX_NP;
    a.k0 = (uint32_t)(seed & 0xffffffffu);
    a.k1 = (uint32_t)(seed >> 32);
    a.stream_id = stream_id;
    a.chain = d_chain;
    a.logp = d_logp;
    a.x_end = d_x_end;
    a.accepted = d_accepted;
    a.problem_status = d_problem_status;
    a.status = d_status;
    hipStream_t st = as_stream(stream);
    return dispatch_int<PF_LLH, PF_POISSON_LLH, PF_CHI2, PF_MOD_CHI2>(kind, [&](auto c) {
        return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(n_params, [&](auto j) {
            return posterior_launch<decltype(c)::value, decltype(j)::value>(a, st);
        });
    });
}
