"""Shared pieces of the tests of the pseudo-data with drawn nuisance truths (csrc/fluctuate_device.hpp: `fl_truth`,
`fl_linear_mean`; `pisa_hip_fluctuate_linear` through `kernels.fluctuate_linear`; `nuisance="prior"` of
pisa_amd/analysis/ensemble.py): the numpy restatement, draw for draw, on top of tests/fluctuate_cases.py (Philox, the
Poisson sampler) and tests/fluctuate_method_cases.py (the normal deviate, the window of the library's log).  A plain
helper module (no fixtures); tests/test_host_truth.py validates it without a GPU, tests/test_gpu_truth.py holds the
kernels to it.

The definition ("pseudo-data with drawn nuisance truths").  Inputs: the row mu0 [B], optionally sigma [B],
the response R [J, B], and per parameter scale_j >= 0, shift_j, lower_j <= upper_j.
    truth   eta[t, j] = shift_j where scale_j == 0 (nothing is drawn, the box is not read); otherwise the first of the
            candidates x_r = shift_j + scale_j z_r (two rounded steps), r = 0, 1, ..., with lower_j <= x_r <= upper_j,
            z_r = PPND16(unit_open(w0, w1)) of the Philox block with the counter (0x80000000 + j, trial number, stream, r)
            under the key of the seed.  After 256 refused candidates the last one is held inside the box (x < lower ->
            lower, x > upper -> upper) and the call is marked exhausted.
    mean    mu_t[b] = mu0[b] + R[0, b] eta[t, 0] + ... + R[J - 1, b] eta[t, J - 1], ascending j, every product and sum
            rounded; a NaN stays NaN; mu_t[b] < 0 becomes 0 and is counted.
    entry   the entry of tests/fluctuate_method_cases.py for the mean mu_t[b] and sigma[b]: the blocks with the counter
            (b, trial number, stream, attempt) -- b <= 2^31 - 2, so never a truth's block.

What may differ between this restatement and the kernel: the library's log in the tail branches of AS 241, as in
fluctuate_method_cases.  `truths` therefore carries, per candidate, the window [x_lo, x_hi] of the values a log within
LOG_ULPS of numpy's reaches (x is monotone in z: the two ends bound it), and marks a truth `marginal` where some
candidate's acceptance is not the same over its whole window -- a candidate that close to a box edge.  A truth that is
not marginal lies inside [lo, hi], and lo == hi wherever the accepted candidate came from the central branch.  The
data are then compared on the KERNEL's own truths (`block` takes eta), so that a truth from the tails does not blur
the comparison of the counts.
"""
import numpy as np

from tests import fluctuate_cases as fc
from tests import fluctuate_method_cases as fm

TRUTH_WORD = 0x80000000
ATTEMPTS = 256
METHODS = ("poisson", "gauss", "gauss+poisson")
KINDS = ("unbounded", "two-sided", "one-sided", "mixed")
# the shapes of the GPU test and their seed, at which the restatement marks nothing marginal (tests/test_host_truth.py)
SEED, STREAM = 1, 3
TRUTH_SHAPES = tuple((T, J) for T in (1, 63, 64, 65, 257) for J in (1, 3, 8))
DATA_SHAPES = tuple((T, B) for T in (1, 65, 257) for B in (1, 63, 64, 65, 257))


def first_trial_of(T):
    """the T = 65 cases run their trial numbers up to the last one the counter word holds"""
    return 2 ** 32 - T if T == 65 else 0


def data_case(T, B, i):
    """the inputs of data shape number i: (mu0, sigma, R, (scale, shift, lower, upper)); J and the kind of box cycle"""
    J = (1, 3, 8)[i % 3]
    mu0, sigma = fm.palette_rows(B)
    return mu0, sigma, responses(J, B, mu0), priors(J, KINDS[i % len(KINDS)])


def truth_deviates(trial, j, stream, seed, r):
    """u of the r-th candidate block of the truths: `trial` (the trial NUMBER) and `j` arrays of one shape"""
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = fc.philox((np.asarray(j, dtype=np.uint64) + np.uint64(TRUTH_WORD), np.asarray(trial, dtype=np.uint64),
                   np.uint64(int(stream) & 0xFFFFFFFF), np.uint64(r)), key)
    return fm.unit_open(w[0], w[1])


def truths(scale, shift, lower, upper, n_trials, seed, stream=0, first_trial=0, attempts=ATTEMPTS):
    """[n_trials, J] truths -> dict(eta, lo, hi: the window the kernel's truth lies in, marginal [n_trials, J] bool,
    tries [n_trials, J]: candidates used (0 where nothing is drawn), exhausted: bool)"""
    scale, shift = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
    J = scale.size
    lower = np.full(J, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
    upper = np.full(J, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
    T = int(n_trials)
    shape = (T, J)
    eta = np.broadcast_to(shift[None, :], shape).copy()
    lo, hi = eta.copy(), eta.copy()
    marginal = np.zeros(shape, dtype=bool)
    tries = np.zeros(shape, dtype=np.int64)
    tt, jj = np.nonzero(np.broadcast_to((scale != 0.0)[None, :], shape))
    exhausted = False
    for r in range(int(attempts)):
        if not tt.size:
            break
        z, z_lo, z_hi = fm.normal(truth_deviates(tt.astype(np.uint64) + np.uint64(first_trial), jj, stream, seed, r))
        x, x_lo, x_hi = (shift[jj] + scale[jj] * v for v in (z, z_lo, z_hi))
        inside, in_lo, in_hi = ((lower[jj] <= v) & (v <= upper[jj]) for v in (x, x_lo, x_hi))
        marginal[tt, jj] |= (in_lo != inside) | (in_hi != inside)
        tries[tt, jj] = r + 1
        eta[tt, jj], lo[tt, jj], hi[tt, jj] = x, x_lo, x_hi
        if r == int(attempts) - 1 and not inside.all():
            exhausted = True
            for a in (eta, lo, hi):
                a[tt[~inside], jj[~inside]] = np.clip(a[tt[~inside], jj[~inside]], lower[jj[~inside]],
                                                      upper[jj[~inside]])
        tt, jj = tt[~inside], jj[~inside]
    return dict(eta=eta, lo=lo, hi=hi, marginal=marginal, tries=tries, exhausted=exhausted)


def means(mu0, R, eta):
    """[T, B]: mu0 + R[0] eta[:, 0] + ... in ascending j, every step rounded -> (mu_t with the negative means taken as
    0, clipped [T, B] bool)"""
    mu0, R, eta = (np.asarray(a, dtype=np.float64) for a in (mu0, R, eta))
    mu = np.broadcast_to(mu0[None, :], (eta.shape[0], mu0.size)).copy()
    for j in range(R.shape[0]):
        mu = mu + R[j][None, :] * eta[:, j, None]
    with np.errstate(invalid="ignore"):
        clipped = mu < 0.0
    return np.where(clipped, 0.0, mu), clipped


def entries(mu, sigma_row, method, seed, stream=0, first_trial=0):
    """the entries of `fluctuate_method_cases.block` for means that differ per trial: mu [T, B] -> (values, lo, hi,
    marginal); the methods are "poisson", "gauss" and "gauss+poisson" alone"""
    assert method in METHODS
    mu = np.asarray(mu, dtype=np.float64)
    shape = mu.shape
    t = np.broadcast_to((np.arange(shape[0], dtype=np.uint64) + np.uint64(first_trial))[:, None], shape)
    b = np.broadcast_to(np.arange(shape[1], dtype=np.uint64)[None, :], shape)
    if method == "poisson":
        k, marginal, _ = fc.draws(mu, t, b, stream, seed)
        return k, k, k, marginal
    sigma = np.broadcast_to(np.asarray(sigma_row, dtype=np.float64).ravel()[None, :], shape)
    with np.errstate(invalid="ignore", over="ignore"):
        live = ~np.isnan(mu) & (sigma >= 0.0) & np.isfinite(sigma)
        flat = live & (sigma == 0.0)
        z, z_lo, z_hi = fm.normal(fm.deviates(t, b, stream, seed))
        g, g_lo, g_hi = (np.where(flat, mu, np.where(live, mu + sigma * x, np.nan)) for x in (z, z_lo, z_hi))
        if method == "gauss":
            return g, g_lo, g_hi, np.zeros(shape, dtype=bool)
        draws = [fc.draws(np.where(x < 0.0, 0.0, x), t, b, stream, seed) for x in (g, g_lo, g_hi)]
    k = draws[0][0]
    marginal = draws[0][1] | draws[1][1] | draws[2][1]
    for other in draws[1:]:
        marginal |= ~((other[0] == k) | (np.isnan(other[0]) & np.isnan(k)))
    return k, k, k, marginal


def block(mu0, sigma_row, R, eta, method, seed, stream=0, first_trial=0):
    """what one call addresses, on GIVEN truths eta [T, J] -> (values, lo, hi, marginal, clipped: the count)"""
    mu, clipped = means(mu0, R, eta)
    return entries(mu, sigma_row, method, seed, stream, first_trial) + (int(clipped.sum()),)


def linear(mu0, sigma_row, R, scale, shift, lower, upper, method, n_trials, seed, stream=0, first_trial=0):
    """the whole call restated -> dict(data, eta, clipped, truths: the dict of `truths`, block: the tuple of `block`)"""
    tr = truths(scale, shift, lower, upper, n_trials, seed, stream, first_trial)
    blk = block(mu0, sigma_row, R, tr["eta"], method, seed, stream, first_trial)
    return dict(data=blk[0], eta=tr["eta"], clipped=blk[4], truths=tr, block=blk)


def responses(n_params, n_bins, mu0, size=0.05):
    """[J, B] responses of the size of `size` of the mean per unit of the parameter, NaN and 0 means given a response
    of their own so that every bin moves"""
    b = (np.arange(n_bins) + 0.5) / n_bins
    base = np.where(np.isnan(mu0) | (mu0 == 0.0), 1.0, mu0)
    return size * np.cos((np.arange(n_params)[:, None] + 1) * np.pi * b[None, :]) * base[None, :]


def priors(n_params, kind):
    """(scale, shift, lower, upper) of J parameters: "unbounded", "two-sided" (a box of a little more than +-1 sigma
    about the shift, off centre), "one-sided" (lower bounds alone, below the shift), "mixed" (cycling through those
    and scale == 0)"""
    j = np.arange(n_params)
    scale, shift = 0.5 + 0.25 * j, 0.1 * (j - 1.0)
    lower, upper = np.full(n_params, -np.inf), np.full(n_params, np.inf)
    if kind == "two-sided":
        lower, upper = shift - 1.0 * scale, shift + 1.25 * scale
    elif kind == "one-sided":
        lower = shift - 0.5 * scale
    elif kind == "mixed":
        form = j % 4
        lower = np.where(form == 1, shift - 1.0 * scale, np.where(form == 2, shift - 0.5 * scale, lower))
        upper = np.where(form == 1, shift + 1.25 * scale, upper)
        scale = np.where(form == 3, 0.0, scale)
    else:
        assert kind == "unbounded"
    return scale, shift, lower, upper


class NumpyTruthSolver(fm.NumpyMethodSolver):
    """`fluctuate_method_cases.NumpyMethodSolver` plus `draw_linear`: the batch evaluator of `generator="device"` with
    `nuisance="prior"` restated in numpy.  (The profiled methods a `response` needs come from a subclass in the test
    that uses them: tests/profile_cases.py.)"""

    def draw_linear(self, mu, response, sigma, method, n_trials, seed, stream, scale, shift, lower=None, upper=None,
                    first_trial=0):
        self.calls.append(("draw_linear", method, int(n_trials), int(stream), int(first_trial)))
        out = linear(np.asarray(mu, dtype=np.float64).ravel(), sigma, np.asarray(response, dtype=np.float64), scale,
                     shift, lower, upper, method, n_trials, seed, stream, first_trial)
        return dict(data=out["data"], eta=out["eta"], clipped=out["clipped"])
