// ensemble.hip -- the metric of MANY data maps against MANY templates: M[t][k] = Map.metric_total of data map t
// against template k (pisa/core/map.py:1572-1604 + np.nansum, pisa/utils/stats.py) for llh, poisson_llh, chi2 and
// mod_chi2, as a [n_trials][n_templates] matrix or reduced per trial to (best, arg, value at a given column).
//   ens_direct_kernel    every kind: one lane owns one (t, k) pair and walks the bins in ascending order through
//                        `metric_bin` (metric_device.hpp), rows of D / E / S2 staged in LDS in bin chunks.  The lane sees
//                        every bin of its pair, so chi2's whole-map rule (stats.py:160-163) is kept.
//   ens_prep_kernel +    llh, poisson_llh: the matrix is a dense contraction,
//   ens_product_kernel       poisson_llh  M = (sum_b d ln mu  -  sum_b mu)  -  sum_b lgamma(d + 1)
//                            llh          M = sum_b (d ln mu - [d > 0] mu)  -  sum_{b: d > 0} (d ln d - d)
//                        (mu clipped to SMALL_POS; a bin without data is dropped with its -mu, stats.py:243-253 under
//                        np.nansum).  The preparation writes L = ln mu and -mu per template, zero-padded to a multiple
//                        of 4 bins, and the constants s_k = sum_b mu, c_t; the contraction runs on
//                        v_mfma_f64_16x16x4_f64, for llh with the two products [d . L] and [(d > 0) . (-mu)] of a group
//                        of 4 bins issued back to back into the same accumulator.
// What both forms guarantee: the bits of entry (t, k) depend on row t of D and row k of E / S2 only -- not on the
// number of rows, their position, or how a caller splits them over launches.  Every sum over bins is ONE chain in
// ascending bin order (per lane in the direct form, per accumulator element in the MFMA: groups of 4 bins in ascending
// order, the same groups whatever the tile), there is no atomic and no split over the bins.
// Every chain keeps its rounding errors (`ens_two_sum`): the lane's sum of the direct form, the constants s_k and c_t
// (stored as (hi, lo) pairs), and in the product form the entry's running sum, which the matrix core's accumulator
// joins every EP_FLUSH = 16 bins before it restarts from zero; the epilogue (sum - s_k) - c_t carries its rounding
// errors to one last addition.  A plain chain over 130 bins misses the bound the numpy restatements are held to
// (tests/ensemble_cases.py: 12 eps of the scale against 2).
// The reduced form keeps, per lane, the best value of its column class over the template tiles in ascending order
// (strict comparison: the smallest k wins a tie) and joins the 16 columns across lanes at the end; max / min do not
// round, so the three outputs are those of the same reduction over the full matrix.
#include "common.hpp"
#include "ensemble_device.hpp"
#include "metric_device.hpp"

#include <math.h>

namespace pisa {

typedef double ens_d4 __attribute__((ext_vector_type(4)));

constexpr int ENS_THREADS = 256;
// direct form: 16 trials x 16 templates per workgroup, 64 bins per chunk; rows 65 doubles apart (an odd stride: the 16
// template rows a wavefront reads at one bin fall into different LDS banks, the trial row is a broadcast)
constexpr int ED_TILE = 16;
constexpr int ED_BK = 64;
constexpr int ED_LD = ED_BK + 1;
// product form: 64 trials x 64 templates per workgroup (a wavefront: 16 trials x 64 templates = 4 accumulator
// tiles, one A fragment feeds 4 MFMAs), 32 bins per chunk
constexpr int EP_TILE = 64;
constexpr int EP_BK = 32;
constexpr int EP_LD = EP_BK + 4;
constexpr int EP_FLUSH = 16;
// preparation: 64 rows per workgroup, 32 bins per chunk
constexpr int EPREP_ROWS = 64;
constexpr int EPREP_BK = 32;
constexpr int EPREP_LD = EPREP_BK + 1;

template <int KIND>
struct EnsKind {
    static constexpr bool is_llh = KIND == PISA_HIP_METRIC_LLH || KIND == PISA_HIP_METRIC_POISSON_LLH;
};

// ----------------------------------------------------------------------------------------------- direct form
// grid.x: strips of 16 trials; FULL: grid.y = tiles of 16 templates, REDUCE: the workgroup walks all of them
template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(ENS_THREADS)
ens_direct_kernel(const double *__restrict__ D, const double *__restrict__ E, const double *__restrict__ S2,
                  const double *__restrict__ offset, int k0, int T, int K, int64_t B, double *__restrict__ out,
                  double *__restrict__ best, int32_t *__restrict__ arg, double *__restrict__ at,
                  int32_t *__restrict__ status) {
    constexpr bool WITH_S2 = KIND == PISA_HIP_METRIC_MOD_CHI2;
    constexpr bool MAXIMISE = EnsKind<KIND>::is_llh;
    __shared__ double sD[ED_TILE * ED_LD];
    __shared__ double sE[ED_TILE * ED_LD];
    __shared__ double sS[WITH_S2 ? ED_TILE * ED_LD : 8];
    const int tid = (int)threadIdx.x, ti = tid >> 4, ki = tid & 15;
    const int64_t t0 = (int64_t)blockIdx.x * ED_TILE;
    const int64_t t = t0 + ti;
    const int n_kt = ens_tiles(K, ED_TILE);
    const int kt_begin = REDUCE ? 0 : (int)blockIdx.y, kt_end = REDUCE ? n_kt : (int)blockIdx.y + 1;
    const bool use_s2 = WITH_S2 && S2 != nullptr;
    EnsOut<MAXIMISE, REDUCE> res;
    bool negative = false;
    for (int kt = kt_begin; kt < kt_end; kt++) {
        const int64_t k = (int64_t)kt * ED_TILE + ki;
        double sum = 0.0, comp = 0.0;
        bool differs = false;   // chi2: some |d - mu| >= 5 eps
        for (int64_t c0 = 0; c0 < B; c0 += ED_BK) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < ED_TILE * ED_BK / ENS_THREADS; i++) {
                const int idx = tid + ENS_THREADS * i, r = idx / ED_BK, cc = idx % ED_BK;
                const int64_t b = c0 + cc, tt = t0 + r, kk = (int64_t)kt * ED_TILE + r;
                const bool in_b = b < B;
                sD[r * ED_LD + cc] = (in_b && tt < T) ? D[tt * B + b] : 0.0;
                sE[r * ED_LD + cc] = (in_b && kk < K) ? E[kk * B + b] : 0.0;
                if (WITH_S2) sS[r * ED_LD + cc] = (use_s2 && in_b && kk < K) ? S2[kk * B + b] : 0.0;
            }
            __syncthreads();
            const int nb = (int)(B - c0 < ED_BK ? B - c0 : ED_BK);
            const double *pd = sD + ti * ED_LD, *pe = sE + ki * ED_LD, *ps = sS + (WITH_S2 ? ki * ED_LD : 0);
            for (int cc = 0; cc < nb; cc++) {
                const double d = pd[cc], lam = pe[cc], s2 = WITH_S2 ? ps[cc] : 0.0;
                // as metric_kernel (metric_flux.hip): a non-finite input is a NaN bin, which np.nansum drops
                const bool finite = (d == d) && (lam == lam) && !isinf(d) && !isinf(lam);
                if (!finite) continue;
                if (d < 0.0 || lam < 0.0) negative = true;
                if (KIND == PISA_HIP_METRIC_CHI2) {
                    const double lc = lam < SMALL_POS ? SMALL_POS : lam;
                    if (!(fabs(d - lc) < 5 * FTYPE_PREC)) differs = true;
                }
                const double v = metric_bin(KIND, d, lam, s2);
                if (v == v) ens_two_sum(sum, comp, v);   // np.nansum
            }
        }
        double acc = sum + comp;
        if (KIND == PISA_HIP_METRIC_CHI2 && !differs) acc = 0.0;   // stats.py:160-161
        if (t < T && k < K) res.entry(acc, t, k, K, offset, k0, out);
    }
    res.finish(t, T, ki, k0, best, arg, at);
    if (negative) status[0] = PISA_HIP_ERR_NEGATIVE;   // (every writer stores the same word)
}

// ---------------------------------------------------------------------------------------------- product form
// Per template row k (blocks [0, ceil(K / 64))):  Lp[k][b] = ln(max(E, SMALL_POS)), NLp[k][b] = -max(E, SMALL_POS)
// (llh only), both zero for B <= b < Bp, s[k] = sum_b max(E, SMALL_POS) (poisson_llh only); per trial row t (the
// blocks after them):  c[t] = sum_b lgamma(d + 1) (poisson_llh) or sum_{b: d > 0} (d ln d - d) (llh).
// Every thread forms the terms of some elements of the chunk, then thread r < 64 adds the terms of row r in
// ascending bin order: one compensated chain per row (`ens_two_sum`), carried in registers from chunk to chunk and
// stored as a (hi, lo) pair.
template <int KIND>
__global__ void __launch_bounds__(ENS_THREADS)
ens_prep_kernel(const double *__restrict__ D, const double *__restrict__ E, int T, int K, int64_t B, int64_t Bp,
                double *__restrict__ Lp, double *__restrict__ NLp, double2 *__restrict__ s, double2 *__restrict__ c,
                int32_t *__restrict__ status) {
    __shared__ double sh[EPREP_ROWS * EPREP_LD];
    const int tid = (int)threadIdx.x;
    const int n_kb = ens_tiles(K, EPREP_ROWS);
    const bool templates = (int)blockIdx.x < n_kb;
    const int64_t r0 = (int64_t)(templates ? blockIdx.x : blockIdx.x - n_kb) * EPREP_ROWS;
    const int64_t n_rows = templates ? K : T;
    double sum = 0.0, comp = 0.0;
    bool negative = false;
    for (int64_t c0 = 0; c0 < Bp; c0 += EPREP_BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < EPREP_ROWS * EPREP_BK / ENS_THREADS; i++) {
            const int idx = tid + ENS_THREADS * i, r = idx / EPREP_BK, cc = idx % EPREP_BK;
            const int64_t b = c0 + cc, row = r0 + r;
            double term = 0.0;
            if (row < n_rows && b < Bp) {
                if (templates) {
                    double l = 0.0, nl = 0.0;
                    if (b < B) {
                        const double e = E[row * B + b];
                        if (e < 0.0) negative = true;
                        const double lc = e < SMALL_POS ? SMALL_POS : e;
                        l = log(lc);
                        nl = -lc;
                        term = lc;
                    }
                    Lp[row * Bp + b] = l;
                    if (KIND == PISA_HIP_METRIC_LLH) NLp[row * Bp + b] = nl;
                } else if (b < B) {
                    const double d = D[row * B + b];
                    if (d < 0.0) negative = true;
                    if (KIND == PISA_HIP_METRIC_POISSON_LLH)
                        term = lgamma(d + 1);
                    else
                        term = d > 0.0 ? d * log(d) - d : 0.0;
                }
            }
            sh[r * EPREP_LD + cc] = term;
        }
        __syncthreads();
        if (tid < EPREP_ROWS) {
            const int nb = (int)(B - c0 < EPREP_BK ? (B - c0 > 0 ? B - c0 : 0) : EPREP_BK);
            const double *p = sh + tid * EPREP_LD;
            for (int cc = 0; cc < nb; cc++) ens_two_sum(sum, comp, p[cc]);
        }
    }
    if (tid < EPREP_ROWS && r0 + tid < n_rows) {
        // the constant as an unevaluated pair: hi = fl(sum + comp), lo = the rest
        const double hi = sum + comp;
        const double2 pair = make_double2(hi, (sum - hi) + comp);
        if (!templates)
            c[r0 + tid] = pair;
        else if (KIND == PISA_HIP_METRIC_POISSON_LLH)
            s[r0 + tid] = pair;
    }
    if (negative) status[0] = PISA_HIP_ERR_NEGATIVE;
}

// grid.x: strips of 64 trials; FULL: grid.y = tiles of 64 templates, REDUCE: the workgroup walks all of them.
// Wavefront w owns trials 16 w .. 16 w + 15 of the strip and the tile's 64 templates: acc[j] is the 16 x 16 block of
// templates 16 j .. 16 j + 15.  Operands of v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15]; result register r of lane l is C[row (l >> 4) + 4 r][col l & 15].
template <int KIND, bool REDUCE>
__global__ void __launch_bounds__(ENS_THREADS)
ens_product_kernel(const double *__restrict__ D, const double *__restrict__ Lp, const double *__restrict__ NLp,
                   const double2 *__restrict__ s, const double2 *__restrict__ c, const double *__restrict__ offset,
                   int k0, int T, int K, int64_t B, int64_t Bp, double *__restrict__ out,
                   double *__restrict__ best, int32_t *__restrict__ arg, double *__restrict__ at) {
    constexpr bool LLH = KIND == PISA_HIP_METRIC_LLH;
    __shared__ double sD[EP_TILE * EP_LD];
    __shared__ double sL[EP_TILE * EP_LD];
    __shared__ double sN[LLH ? EP_TILE * EP_LD : 8];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * EP_TILE;
    const int n_kt = ens_tiles(K, EP_TILE);
    const int kt_begin = REDUCE ? 0 : (int)blockIdx.y, kt_end = REDUCE ? n_kt : (int)blockIdx.y + 1;
    // (`EnsOut` in its four-row form, spelled out: four instances of the struct change the kernel's code, EXPERIMENTS.md)
    double best_v[4] = {0.0, 0.0, 0.0, 0.0}, at_v[4] = {0.0, 0.0, 0.0, 0.0};
    int best_k[4] = {-1, -1, -1, -1};
    double2 c_t[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t t = t0 + 16 * wave + lk + 4 * r;
        c_t[r] = t < T ? c[t] : make_double2(0.0, 0.0);
    }
    for (int kt = kt_begin; kt < kt_end; kt++) {
        const int64_t kbase = (int64_t)kt * EP_TILE;
        // the matrix core's accumulator runs over EP_FLUSH bins, then joins the entry's running sum through
        // `ens_two_sum` and starts again from zero: the same bins whatever the tile (c0 is a multiple of EP_BK)
        ens_d4 acc[4], sum[4], comp[4];
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = sum[j] = comp[j] = (ens_d4){0.0, 0.0, 0.0, 0.0};
        for (int64_t c0 = 0; c0 < Bp; c0 += EP_BK) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EP_TILE * EP_BK / ENS_THREADS; i++) {
                const int idx = tid + ENS_THREADS * i, r = idx / EP_BK, cc = idx % EP_BK;
                const int64_t b = c0 + cc, tt = t0 + r, kk = kbase + r;
                sD[r * EP_LD + cc] = (b < B && tt < T) ? D[tt * B + b] : 0.0;
                const bool in_k = b < Bp && kk < K;
                sL[r * EP_LD + cc] = in_k ? Lp[kk * Bp + b] : 0.0;
                if (LLH) sN[r * EP_LD + cc] = in_k ? NLp[kk * Bp + b] : 0.0;
            }
            __syncthreads();
            const int n_steps = (int)(Bp - c0 < EP_BK ? (Bp - c0) / 4 : EP_BK / 4);
            const double *pa = sD + (16 * wave + li) * EP_LD + lk;
            for (int st = 0; st < n_steps; st++) {
                const double a = pa[4 * st];
                const double ai = a > 0.0 ? 1.0 : 0.0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int o = (16 * j + li) * EP_LD + 4 * st + lk;
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sL[o], acc[j], 0, 0, 0);
                    if (LLH) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, sN[o], acc[j], 0, 0, 0);
                }
                if ((st + 1) % (EP_FLUSH / 4) == 0 || st + 1 == n_steps) {
#pragma unroll
                    for (int j = 0; j < 4; j++) {
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            double sv = sum[j][r], cv = comp[j][r];
                            ens_two_sum(sv, cv, acc[j][r]);
                            sum[j][r] = sv;
                            comp[j][r] = cv;
                        }
                        acc[j] = (ens_d4){0.0, 0.0, 0.0, 0.0};
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t k = kbase + 16 * j + li;
            if (k >= K) continue;
            const double2 s_k = LLH ? make_double2(0.0, 0.0) : s[k];
            const double off = (REDUCE && offset) ? offset[k] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int64_t t = t0 + 16 * wave + lk + 4 * r;
                if (t >= T) continue;
                // (sum - s_k) - c_t in that order, every rounding error kept and added at the end
                double m = sum[j][r], e = comp[j][r];
                if (!LLH) {
                    ens_two_sum(m, e, -s_k.x);
                    e -= s_k.y;
                }
                ens_two_sum(m, e, -c_t[r].x);
                e -= c_t[r].y;
                m += e;
                if (REDUCE) {
                    const double v = offset ? m + off : m;
                    if (ens_better<true>(v, (int)k, best_v[r], best_k[r])) {
                        best_v[r] = v;
                        best_k[r] = (int)k;
                    }
                    if ((int)k == k0) at_v[r] = v;
                } else {
                    out[t * K + k] = m;
                }
            }
        }
    }
    if (REDUCE) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            ens_join16<true>(best_v[r], best_k[r]);
            const int64_t t = t0 + 16 * wave + lk + 4 * r;
            if (t < T) {
                if (li == 0) {
                    best[t] = best_v[r];
                    arg[t] = best_k[r];
                }
                if (li == (k0 & 15)) at[t] = at_v[r];
            }
        }
    }
}



// preparation buffers of the product form
static DeviceScratch g_ens_work;

template <int KIND, bool REDUCE>
static int ens_launch_direct(const EnsArgs &a) {
    const int T = (int)a.T, K = (int)a.K;
    const dim3 grid((unsigned)ens_tiles(T, ED_TILE), REDUCE ? 1u : (unsigned)ens_tiles(K, ED_TILE));
    hipLaunchKernelGGL((ens_direct_kernel<KIND, REDUCE>), grid, dim3(ENS_THREADS), 0, as_stream(a.stream), a.D, a.E,
                       a.S2, a.offset, a.k0, T, K, a.B, a.out, a.best, a.arg, a.at, a.status);
    PISA_CHECK_LAUNCH("ens_direct_kernel");
    return PISA_HIP_OK;
}

template <int KIND, bool REDUCE>
static int ens_launch_product(const EnsArgs &a) {
    constexpr bool LLH = KIND == PISA_HIP_METRIC_LLH;
    const int T = (int)a.T, K = (int)a.K;
    const int64_t B = a.B, Bp = (B + 3) / 4 * 4;
    hipStream_t stream = as_stream(a.stream);
    double *w;
    const int rc = g_ens_work.reserve((int64_t)K * Bp * (LLH ? 2 : 1) + 2 * ((int64_t)K + T), &w);
    if (rc != PISA_HIP_OK) return rc;
    double *Lp = w, *NLp = LLH ? Lp + (int64_t)K * Bp : nullptr;
    double2 *s = reinterpret_cast<double2 *>(w + (int64_t)K * Bp * (LLH ? 2 : 1)), *c = s + K;   // (16-byte aligned: Bp is a multiple of 4)
    const unsigned n_prep = (unsigned)(ens_tiles(K, EPREP_ROWS) + ens_tiles(T, EPREP_ROWS));
    hipLaunchKernelGGL((ens_prep_kernel<KIND>), dim3(n_prep), dim3(ENS_THREADS), 0, stream, a.D, a.E, T, K, B, Bp, Lp,
                       NLp, s, c, a.status);
    PISA_CHECK_LAUNCH("ens_prep_kernel");
    const dim3 grid((unsigned)ens_tiles(T, EP_TILE), REDUCE ? 1u : (unsigned)ens_tiles(K, EP_TILE));
    hipLaunchKernelGGL((ens_product_kernel<KIND, REDUCE>), grid, dim3(ENS_THREADS), 0, stream, a.D, Lp, NLp, s, c,
                       a.offset, a.k0, T, K, B, Bp, a.out, a.best, a.arg, a.at);
    PISA_CHECK_LAUNCH("ens_product_kernel");
    return PISA_HIP_OK;
}

template <bool REDUCE>
static int ens_run(int32_t kind, int32_t form, const EnsArgs &a) {
    if (kind < PISA_HIP_METRIC_LLH || kind > PISA_HIP_METRIC_MOD_CHI2) return PISA_HIP_ERR_INVALID;
    if (form < PISA_HIP_ENSEMBLE_AUTO || form > PISA_HIP_ENSEMBLE_PRODUCT) return PISA_HIP_ERR_INVALID;
    const bool llh_kind = kind <= PISA_HIP_METRIC_POISSON_LLH;
    if (form == PISA_HIP_ENSEMBLE_PRODUCT && !llh_kind) return PISA_HIP_ERR_INVALID;
    if (!ens_check_matrix<REDUCE>(a, ED_TILE)) return PISA_HIP_ERR_INVALID;
    if (llh_kind && form != PISA_HIP_ENSEMBLE_DIRECT)
        return dispatch_int<PISA_HIP_METRIC_LLH, PISA_HIP_METRIC_POISSON_LLH>(
            kind, [&](auto c) { return ens_launch_product<decltype(c)::value, REDUCE>(a); });
    return dispatch_int<PISA_HIP_METRIC_LLH, PISA_HIP_METRIC_POISSON_LLH, PISA_HIP_METRIC_CHI2,
                        PISA_HIP_METRIC_MOD_CHI2>(
        kind, [&](auto c) { return ens_launch_direct<decltype(c)::value, REDUCE>(a); });
}

}  // namespace pisa

using namespace pisa;

PISA_API int pisa_hip_metric_matrix(int32_t kind, int32_t form, const double *d_data, const double *d_expected,
                                    const double *d_sigma2, int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                    double *d_out, int32_t *d_status, void *stream) {
    return ens_run<false>(kind, form, {d_data, d_expected, d_sigma2, nullptr, 0, n_trials, n_templates, n_bins, d_out,
                                       nullptr, nullptr, nullptr, d_status, stream});
}

PISA_API int pisa_hip_metric_matrix_best(int32_t kind, int32_t form, const double *d_data, const double *d_expected,
                                         const double *d_sigma2, const double *d_offset, int32_t k0,
                                         int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_best,
                                         int32_t *d_arg, double *d_at, int32_t *d_status, void *stream) {
    return ens_run<true>(kind, form, {d_data, d_expected, d_sigma2, d_offset, k0, n_trials, n_templates, n_bins,
                                      nullptr, d_best, d_arg, d_at, d_status, stream});
}
