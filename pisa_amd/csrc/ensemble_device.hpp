// ensemble_device.hpp -- what the trial-ensemble files share (ensemble.hip, ensemble_mc.hip, profile.hip).  Device
// side: the count of tiles, the compensated chain every sum over bins is carried in, the reduced form's comparison,
// its join over the 16 lanes of a column class and the bookkeeping of a lane's entry (`EnsOut`).  Host side: the
// launch arguments of the matrix entry points and the checks of sizes and outputs they share with profile.hip.
#pragma once
#include "common.hpp"

namespace pisa {

// tiles of `tile` rows that cover n rows, counted in 64 bits: n may be within a tile of 2^31 - 1
__host__ __device__ __forceinline__ int ens_tiles(int64_t n, int tile) { return (int)((n + tile - 1) / tile); }

// s + c += x with the rounding error of the addition kept in c (Knuth's TwoSum: exact for any magnitudes, no branch).
// A sum carried this way is still ONE chain over the bins in ascending order; its error no longer grows with their
// number (a plain chain of 130 chi2 terms is off by up to 12 eps of the sum, this one by the per-bin errors and one
// final rounding: tests/ensemble_cases.py).
__device__ __forceinline__ void ens_two_sum(double &s, double &c, double x) {
    const double t = s + x;
    const double bb = t - s;
    c += (s - (t - bb)) + (x - bb);
    s = t;
}

// is `v` at column `k` better than (best, arg)?  llh kinds: larger; chi2 kinds: smaller; ties: the smaller column
template <bool MAXIMISE>
__device__ __forceinline__ bool ens_better(double v, int k, double best, int arg) {
    if (k < 0) return false;
    if (arg < 0) return true;
    const bool gt = MAXIMISE ? v > best : v < best;
    return gt || (v == best && k < arg);
}

// joins (best, arg) over the 16 lanes that share lane >> 4
template <bool MAXIMISE>
__device__ __forceinline__ void ens_join16(double &best, int &arg) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
        const double ov = __shfl_xor(best, m, 64);
        const int oa = __shfl_xor(arg, m, 64);
        if (ens_better<MAXIMISE>(ov, oa, best, arg)) {
            best = ov;
            arg = oa;
        }
    }
}

// What a lane does with its entry (t, k).  FULL: it writes out[t][k].  REDUCE: it keeps the best value of its column
// class over the template tiles in ascending order (strict comparison: the smallest k wins a tie) and the value at
// column k0; `finish` joins the 16 column classes of a trial (`ki`: the lane's class) and one lane each writes
// (best, arg) and at.
template <bool MAXIMISE, bool REDUCE>
struct EnsOut {
    double best_v = 0.0, at_v = 0.0;
    int best_k = -1;
    __device__ __forceinline__ void entry(double acc, int64_t t, int64_t k, int K, const double *offset, int k0,
                                          double *out) {
        if (REDUCE) {
            const double v = offset ? acc + offset[k] : acc;
            if (ens_better<MAXIMISE>(v, (int)k, best_v, best_k)) {
                best_v = v;
                best_k = (int)k;
            }
            if ((int)k == k0) at_v = v;
        } else {
            out[t * K + k] = acc;
        }
    }
    __device__ __forceinline__ void finish(int64_t t, int T, int ki, int k0, double *best, int32_t *arg, double *at) {
        if (!REDUCE) return;
        ens_join16<MAXIMISE>(best_v, best_k);
        if (t < T) {
            if (ki == 0) {
                best[t] = best_v;
                arg[t] = best_k;
            }
            if (ki == (k0 & 15)) at[t] = at_v;
        }
    }
};

// ------------------------------------------------------------------------------------------------------ host
// the arguments of a metric_matrix entry point, full (out) or reduced (offset, k0, best, arg, at), as its launches
// take them
struct EnsArgs {
    const double *D, *E, *S2, *offset;
    int32_t k0;
    int64_t T, K, B;
    double *out, *best;
    int32_t *arg;
    double *at;
    int32_t *status;
    void *stream;
};

// every size in [1, 2^31 - 1]: no product of two of them overflows int64
inline bool ens_check_sizes(int64_t T, int64_t K, int64_t B) {
    return T >= 1 && K >= 1 && B >= 1 && T <= 0x7FFFFFFF && K <= 0x7FFFFFFF && B <= 0x7FFFFFFF;
}

// FULL: the matrix; REDUCE: the three vectors and a column k0 of the matrix
template <bool REDUCE>
inline bool ens_check_outputs(const double *out, const double *best, const int32_t *arg, const double *at, int32_t k0,
                              int64_t K) {
    return REDUCE ? (best && arg && at && k0 >= 0 && k0 < K) : out != nullptr;
}

// what the matrix entry points check alike; `tile`: the templates of a workgroup (the full matrix has one workgroup
// row per template tile)
template <bool REDUCE>
inline bool ens_check_matrix(const EnsArgs &a, int tile) {
    return ens_check_sizes(a.T, a.K, a.B) && a.D && a.E && a.status &&
           ens_check_outputs<REDUCE>(a.out, a.best, a.arg, a.at, a.k0, a.K) &&
           (REDUCE || ens_tiles(a.K, tile) <= 65535);
}

}  // namespace pisa
