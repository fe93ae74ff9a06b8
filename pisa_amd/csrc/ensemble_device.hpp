// ensemble_device.hpp -- what the trial-ensemble kernels share (ensemble.hip, ensemble_mc.hip): the count of tiles,
// the compensated chain every sum over bins is carried in, and the reduced form's comparison and its join over the 16
// lanes of a column class.
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

}  // namespace pisa
