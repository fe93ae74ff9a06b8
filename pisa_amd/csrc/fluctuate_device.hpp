// fluctuate_device.hpp -- the counter-based Poisson generator of fluctuate.hip, per entry: Philox4x32-10, the two doubles
// of a block and the sampler (definition: the head of fluctuate.hip).  No HIP type or call, so that the same
// source also compiles for the host with a plain C++ compiler: tests/test_host_fluctuate.py runs it there, under the
// sanitizers, against the numpy restatement of tests/fluctuate_cases.py.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PISA_FL_HD __host__ __device__ __forceinline__
#else
#define PISA_FL_HD inline
#endif

namespace pisa {

constexpr int FL_INVERSION_CAP = 255;
constexpr double FL_PTRS_FROM = 10.0;
constexpr double FL_MU_MAX = 4503599627370496.0;   // 2^52: beyond it a count is not every integer

struct FlWords {
    uint32_t w[4];
};

PISA_FL_HD FlWords fl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return FlWords{{c0, c1, c2, c3}};
}

// 53 bits of two words -> [0, 1); every operation is exact
PISA_FL_HD double fl_unit(uint32_t wa, uint32_t wb) {
    return ((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) * (1.0 / 9007199254740992.0);
}

// one entry: Poisson(mu) from the blocks (b, trial, stream, j); `bad` is set for a mean that has no draw
PISA_FL_HD double fl_draw(double mu, uint32_t b, uint32_t trial, uint32_t stream, uint32_t k0, uint32_t k1,
                          bool &bad) {
    if (mu != mu) return mu;
    if (mu == 0.0) return 0.0;
    if (mu < 0.0 || mu > FL_MU_MAX) {
        bad = true;
        return NAN;
    }
    FlWords w = fl_philox(b, trial, stream, 0u, k0, k1);
    if (mu < FL_PTRS_FROM) {
        const double u = fl_unit(w.w[0], w.w[1]);
        double p = exp(-mu), cdf = p, k = 0.0;
        while (u >= cdf && k < (double)FL_INVERSION_CAP) {
            k += 1.0;
            p *= mu / k;
            cdf += p;
        }
        return k;
    }
    const double slam = sqrt(mu), loglam = log(mu);
    const double bq = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * bq;
    const double invalpha = 1.1239 + 1.1328 / (bq - 3.4);
    const double vr = 0.9277 - 3.6224 / (bq - 2.0);
    for (uint32_t j = 0;;) {
        const double U = fl_unit(w.w[0], w.w[1]) - 0.5, V = fl_unit(w.w[2], w.w[3]);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + bq) * U + mu + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (!(k < 0.0 || (us < 0.013 && V > us))) {
            const double lhs = log(V) + log(invalpha) - log(a / (us * us) + bq);
            const double rhs = -mu + k * loglam - lgamma(k + 1.0);
            if (lhs <= rhs) return k;
        }
        j++;
        w = fl_philox(b, trial, stream, j, k0, k1);
    }
}

}  // namespace pisa
