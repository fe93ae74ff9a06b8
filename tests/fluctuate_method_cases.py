"""Shared pieces of the tests of the fluctuation methods of the device generator (csrc/fluctuate_device.hpp:
`fl_fluctuate`; `pisa_hip_fluctuate` through `kernels.fluctuate`; `method=` of pisa_amd/analysis/ensemble.py): the
numpy restatement of the normal deviate and of the methods gauss, gauss+poisson and scaled_poisson, entry for entry,
on top of the restatement of the Poisson sampler in tests/fluctuate_cases.py.  A plain helper module (no fixtures);
tests/test_host_fluctuate_methods.py validates it without a GPU, tests/test_gpu_fluctuate_methods.py holds the kernel
to it.

The definition.  The Gaussian block of entry (bin b, trial number, stream) is the Philox block with the
counter (b, trial number, stream, 0xFFFFFFFF) under the key of the seed; its first two words give
    u = ((w0 >> 6) * 2^26 + (w1 >> 6) + 0.5) * 2^-52      in [2^-53, 1 - 2^-53], symmetric about 1/2,
and z = PPND16(u), Wichura's Algorithm AS 241, with the Horner chains from the highest coefficient down.
    a NaN mean -> NaN for every method; a NaN, negative or infinite sigma where it is read -> NaN (and the status);
    gauss           mu + sigma z (two rounded steps), sigma == 0 -> mu;
    gauss+poisson   g = mu + sigma z, g < 0 -> 0, then the Poisson sampler at g (sigma == 0: at mu);
    scaled_poisson  mu == 0 -> 0; mu < 0 -> NaN; s = (sigma sigma) / mu, not finite -> NaN; lam = mu / s; k s.

What may differ between this restatement and the kernel.  The central branch of AS 241 (|u - 0.5| <= 0.425, 85 % of
the entries) is additions, multiplications and one division, rounded alike on both sides: the same bits.  The tail
branches take t = -log(min(u, 1 - u)), and log is a library call: glibc's and the device library's double log are each
specified to within 1 ulp, so two of them lie within 2 ulps of each other and LOG_ULPS = 4 leaves a factor of 2.  From
t on every step (sqrt, the chains, the division) rounds alike again, so the kernel's z is, bit for bit, the chain's
value at ONE of the doubles within LOG_ULPS of this side's t.  `normal` therefore evaluates the chain at every one of
them (t stepped by `np.nextafter`, 4 down and 4 up) and returns the smallest and the largest result as (z_lo, z_hi):
the chain's rounding noise from one t to the next is of the size of the slope, so the two end points alone need not
bound the values between them.  `normal_candidates` returns all nine, which tells how many ulps of t apart two sides were.
"""
import numpy as np

from tests import fluctuate_cases as fc

LOG_ULPS = 4
GAUSS_WORD = 0xFFFFFFFF
METHODS = ("poisson", "scaled_poisson", "gauss", "gauss+poisson")
FACTORS = (0.0, 0.3, 1.0, 3.0, 1e-8)         # sigma = f sqrt(mu); 5 is coprime to the palette's 13 means

_CENTRAL_NUM = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
_CENTRAL_DEN = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
_NEAR_NUM = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
             3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
_NEAR_DEN = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
             6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
_FAR_NUM = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
            2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
_FAR_DEN = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
            1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def _horner(coeff, r):
    acc = coeff[0] * r + coeff[1]
    for c in coeff[2:]:
        acc = acc * r + c
    return acc


def unit_open(w0, w1):
    """52 bits of two words -> a double in (0, 1), every operation exact"""
    return ((w0 >> np.uint64(6)).astype(np.float64) * 67108864.0 + (w1 >> np.uint64(6)).astype(np.float64) + 0.5) * (
        1.0 / 4503599627370496.0)


def _tail(t, negative):
    """the tail branches of AS 241 from t = -log(min(u, 1 - u)) on"""
    r = np.sqrt(t)
    near = r <= 5.0
    ra, rb = r - 1.6, r - 5.0
    x = np.where(near, _horner(_NEAR_NUM, ra) / _horner(_NEAR_DEN, ra), _horner(_FAR_NUM, rb) / _horner(_FAR_DEN, rb))
    return np.where(negative, -x, x)


def normal_candidates(u):
    """[2 LOG_ULPS + 1, ...]: z of `u` with t stepped by -LOG_ULPS ... +LOG_ULPS ulps in the tail branches (row LOG_ULPS is
    this side's own z); all rows equal in the central branch"""
    u = np.asarray(u, dtype=np.float64)
    q = u - 0.5
    central = np.abs(q) <= 0.425
    r = 0.180625 - q * q
    zc = _horner(_CENTRAL_NUM, r) * q / _horner(_CENTRAL_DEN, r)
    t0 = -np.log(np.where(q <= 0.0, u, 1.0 - u))
    rows = [None] * (2 * LOG_ULPS + 1)
    rows[LOG_ULPS] = t0
    for step, toward in ((-1, 0.0), (1, np.inf)):
        t = t0
        for j in range(1, LOG_ULPS + 1):
            t = np.nextafter(t, toward)
            rows[LOG_ULPS + step * j] = t
    return np.stack([np.where(central, zc, _tail(t, q < 0.0)) for t in rows])


def normal(u):
    """AS 241 in the kernel's operation order -> (z, z_lo, z_hi); z_lo == z == z_hi in the central branch, the smallest
    and largest value over the t within LOG_ULPS ulps in the tails (module docstring)"""
    z = normal_candidates(u)
    return z[LOG_ULPS], z.min(axis=0), z.max(axis=0)


def deviates(trial, b, stream, seed):
    """u of the Gaussian block of the entries: `trial` (the trial NUMBER) and `b` arrays of one shape"""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = fc.philox((np.asarray(b, dtype=np.uint64), np.asarray(trial, dtype=np.uint64),
                   np.uint64(int(stream) & 0xFFFFFFFF), np.uint64(GAUSS_WORD)), key)
    return unit_open(w[0], w[1])


def block(mu_row, sigma_row, method, n_trials, seed, stream=0, first_trial=0):
    """what one call of the kernel addresses: [n_trials, B] entries of the row `mu_row` with the standard deviations
    `sigma_row` (None for "poisson"), trial numbers from `first_trial` -> (values, lo, hi, marginal): the value with
    this side's log; for "gauss" the bounds the kernel's value lies within (== values in the central branch, == values
    for the other methods); for the methods that end in a Poisson draw the entries whose count may differ."""
    assert method in METHODS
    mu_row = np.asarray(mu_row, dtype=np.float64).ravel()
    shape = (int(n_trials), mu_row.size)
    t = np.broadcast_to((np.arange(shape[0], dtype=np.uint64) + np.uint64(first_trial))[:, None], shape)
    b = np.broadcast_to(np.arange(shape[1], dtype=np.uint64)[None, :], shape)
    mu = np.broadcast_to(mu_row[None, :], shape)
    if method == "poisson":
        k, marginal, _ = fc.draws(mu, t, b, stream, seed)
        return k, k, k, marginal
    sigma = np.broadcast_to(np.asarray(sigma_row, dtype=np.float64).ravel()[None, :], shape)
    none = np.zeros(shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        nan_mu = np.isnan(mu)
        good_sigma = (sigma >= 0.0) & np.isfinite(sigma)
        if method == "scaled_poisson":
            zero = mu == 0.0
            s = (sigma * sigma) / mu
            live = ~nan_mu & ~zero & good_sigma & (mu > 0.0) & np.isfinite(s)
            lam = np.where(live, mu / s, np.nan)
            k, marginal, _ = fc.draws(lam, t, b, stream, seed)
            values = np.where(zero, 0.0, k * s)
            values[~live & ~zero] = np.nan
            return values, values, values, marginal & live
        live = ~nan_mu & good_sigma
        flat = live & (sigma == 0.0)
        z, z_lo, z_hi = normal(deviates(t, b, stream, seed))
        g, g_lo, g_hi = (np.where(flat, mu, np.where(live, mu + sigma * x, np.nan)) for x in (z, z_lo, z_hi))
        if method == "gauss":
            return g, g_lo, g_hi, none
        draws = [fc.draws(np.where(x < 0.0, 0.0, x), t, b, stream, seed) for x in (g, g_lo, g_hi)]
        k = draws[0][0]
        marginal = draws[0][1] | draws[1][1] | draws[2][1]
        for other in draws[1:]:
            marginal |= ~((other[0] == k) | (np.isnan(other[0]) & np.isnan(k)))
        return k, k, k, marginal


def palette_rows(n_bins):
    """(means, sigmas) of `n_bins` bins: the means cycle through `fc.PALETTE` (NaN and 0 included), sigma = f sqrt(mu)
    with f cycling through FACTORS, so that from 65 bins on every mean meets every factor"""
    mu = fc.palette_row(n_bins)
    f = np.array([FACTORS[i % len(FACTORS)] for i in range(int(n_bins))])
    with np.errstate(invalid="ignore"):
        return mu, f * np.sqrt(mu)


def wide_window(mu_row, sigma_row, method):
    """Bins of a "scaled_poisson" row whose Poisson mean lam = mu / s lies above the largest mean of `fc.PALETTE` (1e6).
    `fc.draws` marks an entry marginal within 64 eps of the magnitudes compared, and those grow with the mean: at
    lam = 1e13 (the palette's mu = 1e-3 with f = 1e-8, its only such pair: the larger means give lam > 2^52 and NaN) the
    window around an integer is 0.14 wide and the logarithmic test cancels terms of 3e14, so about a quarter of the
    entries are marginal whatever the seed.  Such entries are still compared with `==` wherever they are not marginal;
    the claims "no entry is marginal at this seed" and "the marginal share is at most 1e-5" are made of every other
    entry, as they are made of the Poisson generator up to its palette's largest mean."""
    mu = np.asarray(mu_row, dtype=np.float64)
    if method != "scaled_poisson":
        return np.zeros(mu.shape, dtype=bool)
    sigma = np.asarray(sigma_row, dtype=np.float64)
    with np.errstate(all="ignore"):
        return mu / ((sigma * sigma) / mu) > max(fc.POSITIVE)


class NumpyMethodSolver(fc.NumpyDrawSolver):
    """`fluctuate_cases.NumpyDrawSolver` plus `fluctuate`: the batch evaluator of `generator="device"` with a `method`
    restated in numpy"""

    def fluctuate(self, mu, sigma, method, n_trials, seed, stream, first_trial=0):
        self.calls.append(("fluctuate", method, int(n_trials), int(stream), int(first_trial)))
        return block(mu, sigma, method, n_trials, seed, stream, first_trial)[0]
