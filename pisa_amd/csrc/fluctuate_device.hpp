// fluctuate_device.hpp -- the counter-based generator of fluctuate.hip, per entry: Philox4x32-10, the doubles of a block,
// the Poisson sampler, the normal deviate and the four fluctuation methods (definition: the head of fluctuate.hip,
// DESIGN.md §4).  No HIP type or call, so that the same source also compiles for the host with a plain C++ compiler:
// tests/test_host_fluctuate.py and tests/test_host_fluctuate_methods.py run it there, under the sanitizers, against the
// numpy restatements of tests/fluctuate_cases.py and tests/fluctuate_method_cases.py.
//
// The Gaussian block of an entry is the Philox block with the counter (bin, trial number, stream, 0xFFFFFFFF) under
// the same key.  The Poisson sampler's blocks carry the attempt j = 0, 1, ... in that word; PTRS accepts every attempt
// with a probability above 0.8, so the chance of reaching j = 2^32 - 1 is below 0.2^(2^32 - 1): the word is one the
// sampler cannot reach and the normal deviate is independent of every Poisson block.  Only the block's first double is
// used, as the open-interval uniform
//     u = ((double)(w0 >> 6) * 2^26 + (double)(w1 >> 6) + 0.5) * 2^-52
// of 52 random bits: it lies in [2^-53, 1 - 2^-53], its lattice is symmetric about 1/2, and u - 0.5 and 1 - u are exact.
// ((k + 0.5) * 2^-53 on the 53-bit integer of fl_unit would not do: k + 0.5 is no double from 2^52 on and the top of
// that lattice rounds to 1.0.)  The deviate is z = PPND16(u), Wichura's Algorithm AS 241 (Applied Statistics 37 (1988)
// 477-484), with the coefficients of the publication; |z| < 8.2096.  Its central branch (|u - 0.5| <= 0.425, 85 % of
// the draws) is additions, multiplications and one division: built without contraction it has the same bits in the
// kernel, in g++ and in numpy.  The tail branches take r = sqrt(-log(min(u, 1 - u))): log is the one library call that
// may differ between the sides.  The Horner chains run from the highest coefficient down, the numerator first.
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
constexpr uint32_t FL_GAUSS_WORD = 0xFFFFFFFFu;    // the attempt word of the Gaussian block
// the methods (PISA_HIP_FLUCT_* of pisa_hip.h; Map.fluctuate of pisa/core/map.py:1118-1254)
constexpr int FL_POISSON = 0, FL_SCALED_POISSON = 1, FL_GAUSS = 2, FL_GAUSS_POISSON = 3;

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

// 52 bits of two words -> (0, 1), symmetric about 1/2; every operation is exact
PISA_FL_HD double fl_unit_open(uint32_t w0, uint32_t w1) {
    return ((double)(w0 >> 6) * 67108864.0 + (double)(w1 >> 6) + 0.5) * (1.0 / 4503599627370496.0);
}

// PPND16 of AS 241: the standard normal quantile of u in (0, 1)
PISA_FL_HD double fl_normal_quantile(double u) {
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
                                 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                               1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
                                3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                              5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                            4.2313330701600911252e+1) * r + 1.0;
        return num / den;
    }
    double r = sqrt(-log(q <= 0.0 ? u : 1.0 - u));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                  1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
               4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
        den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                  1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
               2.05319162663775882187e+0) * r + 1.0;
    } else {
        r = r - 5.0;
        num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                  2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
               5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
        den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                  7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
               5.99832206555887937690e-1) * r + 1.0;
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// the normal deviate of entry (b, trial, stream): the first double of the Gaussian block
PISA_FL_HD double fl_normal(uint32_t b, uint32_t trial, uint32_t stream, uint32_t k0, uint32_t k1) {
    const FlWords w = fl_philox(b, trial, stream, FL_GAUSS_WORD, k0, k1);
    return fl_normal_quantile(fl_unit_open(w.w[0], w.w[1]));
}

// One entry of `method`.  A NaN mean gives NaN for every method: nothing is drawn and `bad` is not set.  Where sigma
// is read, a NaN, negative or infinite sigma gives NaN and `bad`.  Every product and sum is rounded (no contraction).
//   poisson         fl_draw(mu); sigma is not read.
//   gauss           mu + sigma z, not clipped; sigma == 0 gives mu itself and reads no block; mu == 0 with sigma > 0
//                   does fluctuate, as in the reference.
//   gauss+poisson   g = mu + sigma z; g < 0 becomes 0; then fl_draw(g) with its own blocks j = 0, 1, ...; g > 2^52
//                   gives NaN and `bad`; sigma == 0 is exactly the poisson entry.
//   scaled_poisson  mu == 0 gives 0 (sigma is not read); mu < 0 gives NaN and `bad` (the reference silently returns
//                   negative multiples of a negative scale there: this departs from it); otherwise
//                   s = (sigma sigma) / mu, lam = mu / s, k = fl_draw(lam), result k s.  sigma == 0 with mu != 0 gives
//                   lam = inf, so NaN and `bad` (analysis/ensemble.py applies the reference's row rule before it calls);
//                   so does an s that is not finite (sigma sigma overflowed, or mu = +inf gave s = 0 and lam = inf).
// `method` is a constant where the kernel calls this, so an instantiation holds its own branch only.
PISA_FL_HD double fl_fluctuate(int method, double mu, double sigma, uint32_t b, uint32_t trial, uint32_t stream,
                               uint32_t k0, uint32_t k1, bool &bad) {
    if (method == FL_POISSON) return fl_draw(mu, b, trial, stream, k0, k1, bad);
    if (mu != mu) return mu;
    if (method == FL_SCALED_POISSON && mu == 0.0) return 0.0;
    if (!(sigma >= 0.0 && sigma <= 1.7976931348623157e308)) {
        bad = true;
        return NAN;
    }
    if (method == FL_SCALED_POISSON) {
        if (mu < 0.0) {
            bad = true;
            return NAN;
        }
        const double s = (sigma * sigma) / mu;
        if (!(s <= 1.7976931348623157e308)) {   // (sigma sigma overflowed: lam = 0 would give 0 * inf)
            bad = true;
            return NAN;
        }
        const double lam = mu / s;
        const double k = fl_draw(lam, b, trial, stream, k0, k1, bad);
        return k * s;
    }
    double g = mu;
    if (sigma != 0.0) {
        const double sz = sigma * fl_normal(b, trial, stream, k0, k1);
        g = mu + sz;
        if (method == FL_GAUSS_POISSON && g < 0.0) g = 0.0;
    }
    // (one call site of the sampler for both cases of sigma: one copy of it in the kernel)
    return method == FL_GAUSS ? g : fl_draw(g, b, trial, stream, k0, k1, bad);
}

// ---- pseudo-data of a linearised template with drawn nuisance truths (fluctuate_linear.hip) ----
constexpr uint32_t FL_TRUTH_WORD = 0x80000000u;   // the first counter word of parameter j's blocks is FL_TRUTH_WORD + j
constexpr int FL_TRUTH_ATTEMPTS = 256;            // candidates of one truth before the last one is clamped

// The truth of parameter j in trial number `trial`: shift where scale == 0 (nothing is drawn, the box is not read);
// otherwise the first candidate shift + scale z_r, r = 0, 1, ..., inside [lower, upper], z_r the normal deviate of
// the block (FL_TRUTH_WORD + j, trial, stream, r) -- a normal truncated to the box by rejection.  A bin word is at
// most 2^31 - 2, so no block of an entry's draws (Poisson or Gaussian) has this counter.  After FL_TRUTH_ATTEMPTS
// refused candidates the last one is held inside the box by comparisons and `exhausted` is set.
PISA_FL_HD double fl_truth(uint32_t j, uint32_t trial, uint32_t stream, uint32_t k0, uint32_t k1, double scale,
                           double shift, double lower, double upper, bool &exhausted) {
    if (scale == 0.0) return shift;
    double x = shift;
    for (uint32_t r = 0; r < (uint32_t)FL_TRUTH_ATTEMPTS; r++) {
        const FlWords w = fl_philox(FL_TRUTH_WORD + j, trial, stream, r, k0, k1);
        const double sz = scale * fl_normal_quantile(fl_unit_open(w.w[0], w.w[1]));
        x = shift + sz;
        if (x >= lower && x <= upper) return x;
    }
    exhausted = true;
    return x < lower ? lower : (x > upper ? upper : x);
}

// The mean of bin b at the truths: mu0 + r[0] eta_0 + ... + r[J - 1] eta_(J-1) in ascending j, every product and sum
// rounded -- the expression of pf_mu (profile_device.hpp) --, r[j * stride] the response of parameter j in this bin.
// A NaN stays NaN; a negative mean becomes 0 and `clipped` is set.
PISA_FL_HD double fl_linear_mean(double mu0, const double *r, int64_t stride, const double *eta, int n_params,
                                 bool &clipped) {
    double mu = mu0;
    for (int j = 0; j < n_params; j++) {
        const double t = r[j * stride] * eta[j];
        mu = mu + t;
    }
    clipped = mu < 0.0;
    return clipped ? 0.0 : mu;
}

// ---- truths drawn from a fit's Gaussian N(mean, cov) inside a box (fluctuate_linear.hip; DESIGN.md §4, "pseudo-data
// at nuisances fitted to the observed data") ----
constexpr int FL_MVN_MAX = 8;   // parameters at most; L is kept [FL_MVN_MAX][FL_MVN_MAX] whatever J is

// The factor of cov [J][J] (row-major; its lower triangle is read): L [FL_MVN_MAX][FL_MVN_MAX] lower triangular with
// cov = L L^T, entries outside the leading J x J block 0.  A coordinate with cov[j][j] == 0 is dead: its row and
// column of cov must hold zeros alone (else refused), row and column j of L are 0 and the coordinate is never drawn.
// Over the live coordinates in ascending order plain Cholesky row by row,
//     L[i][j] = (cov[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j],   L[j][j] = sqrt(cov[j][j] - sum_{k<j} L[j][k]^2),
// the sums in ascending k, every product, subtraction, division and the sqrt rounded on its own.  false (refused): a J
// outside [1, FL_MVN_MAX], an entry of cov that is not finite, a dead coordinate with a non-zero entry, a pivot that is
// <= 0 or NaN, an entry of L that is not finite.
PISA_FL_HD bool fl_truth_factor(const double *cov, int J, double *L) {
    for (int i = 0; i < FL_MVN_MAX * FL_MVN_MAX; i++) L[i] = 0.0;
    if (J < 1 || J > FL_MVN_MAX) return false;
    for (int i = 0; i < J * J; i++)
        if (!(fabs(cov[i]) <= 1.7976931348623157e308)) return false;
    for (int j = 0; j < J; j++) {
        if (cov[j * J + j] != 0.0) continue;
        for (int i = 0; i < J; i++)
            if (cov[j * J + i] != 0.0 || cov[i * J + j] != 0.0) return false;
    }
    for (int i = 0; i < J; i++) {
        if (cov[i * J + i] == 0.0) continue;
        for (int j = 0; j <= i; j++) {
            if (cov[j * J + j] == 0.0) continue;
            double s = cov[i * J + j];
            for (int k = 0; k < j; k++) {
                const double t = L[i * FL_MVN_MAX + k] * L[j * FL_MVN_MAX + k];   // (0 for a dead k)
                s = s - t;
            }
            if (j < i) {
                s = s / L[j * FL_MVN_MAX + j];
            } else {
                if (!(s > 0.0)) return false;
                s = sqrt(s);
            }
            if (!(fabs(s) <= 1.7976931348623157e308)) return false;
            L[i * FL_MVN_MAX + j] = s;
        }
    }
    return true;
}

// The truths x [J] of trial number `trial`: for the attempt r = 0, 1, ... the deviates z_k of the blocks (FL_TRUTH_WORD
// + k, trial, stream, r) -- the counters of fl_truth -- for the live k (L[k][k] != 0) alone, and the candidate
//     x_j = mean_j + L[j][0] z_0 + ... + L[j][j] z_j   over the live k in ascending order, every step rounded
// (x_j = mean_j for a dead j).  The first candidate ALL of whose coordinates lie inside [lower_j, upper_j] is the
// truth: rejection of the whole vector, which is what samples the normal truncated to the box.  After
// FL_TRUTH_ATTEMPTS refused candidates the last one is held inside the box coordinate by coordinate and `exhausted`
// is set.  The loops have constant bounds so that z and x stay in registers in the kernel.
PISA_FL_HD void fl_truth_mvn(uint32_t trial, uint32_t stream, uint32_t k0, uint32_t k1, const double *mean,
                             const double *L, int J, const double *lower, const double *upper, double *x,
                             bool &exhausted) {
    double z[FL_MVN_MAX];
    for (uint32_t r = 0; r < (uint32_t)FL_TRUTH_ATTEMPTS; r++) {
        bool inside = true;
#pragma unroll
        for (int j = 0; j < FL_MVN_MAX; j++) {
            if (j < J) {
                double xj = mean[j];
                z[j] = 0.0;
                if (L[j * FL_MVN_MAX + j] != 0.0) {
                    const FlWords w = fl_philox(FL_TRUTH_WORD + (uint32_t)j, trial, stream, r, k0, k1);
                    z[j] = fl_normal_quantile(fl_unit_open(w.w[0], w.w[1]));
#pragma unroll
                    for (int k = 0; k <= j; k++) {
                        if (L[k * FL_MVN_MAX + k] != 0.0) {
                            const double t = L[j * FL_MVN_MAX + k] * z[k];
                            xj = xj + t;
                        }
                    }
                }
                x[j] = xj;
                inside = inside && xj >= lower[j] && xj <= upper[j];
            }
        }
        if (inside) return;
    }
    exhausted = true;
#pragma unroll
    for (int j = 0; j < FL_MVN_MAX; j++)
        if (j < J) x[j] = x[j] < lower[j] ? lower[j] : (x[j] > upper[j] ? upper[j] : x[j]);
}

}  // namespace pisa
