"""Shared pieces of the tests of the device Poisson generator (csrc/fluctuate.hip: `pisa_hip_poisson_fluctuate` through
`kernels.poisson_fluctuate`, `generator="device"` of pisa_amd/analysis/ensemble.py): the numpy restatement of the
generator, draw for draw, the palette of means and a batch evaluator that draws.  A plain helper module (no fixtures);
`tests/test_host_fluctuate.py` validates the restatement statistically without a GPU, `tests/test_gpu_fluctuate.py`
holds the kernel to it with `==`.

The generator: Philox4x32-10 with
    key     = (seed & 0xffffffff, seed >> 32)
    counter = (bin b, trial number, stream, attempt j)
two doubles per block, u = ((w_a >> 5) * 2^26 + (w_b >> 6)) * 2^-53 from (w0, w1) and (w2, w3);
    mu == 0 -> 0, NaN -> NaN;
    0 < mu < 10  inversion on the first double of attempt 0: p = exp(-mu), cdf = p, k = 0;
                 while u >= cdf and k < 255: k += 1; p *= mu / k; cdf += p
    mu >= 10     Hoermann's PTRS, one block per attempt, j = 0, 1, ... until accepted.
An entry depends on (seed, stream, trial number, bin, mu) alone, so `draws` takes those as arrays of one shape.

What may differ between this restatement and the kernel.  Square root, division, multiplication and addition round the
same way on both sides (the kernel is built without contraction), so every quantity but exp(-mu), ln and lgamma has
the same bits, and a draw can come out differently only where a decision that involves one of those sat at the edge.
`draws` marks such entries (`marginal`): any decision within MARGIN_EPS = 64 eps of the magnitudes compared --
    inversion  |u - cdf| <= 64 eps max(u, cdf) at the stopping step or at the step before it (the cdf is a sum of
               positive terms: its magnitude is its own);
    PTRS       the floor's argument x = (2 a / us + b) U + mu + 0.43 within 64 eps (|(2 a / us + b) U| + mu + 0.43) of
               the nearest integer, in any attempt;
               |lhs - rhs| <= 64 eps (|ln V| + |ln(1 / alpha)| + |ln(a / us^2 + b)| + mu + |k ln mu| + |lgamma(k + 1)|)
               in any attempt that reached the logarithmic test.
The libraries' exp, ln and lgamma are good to a few eps of their values, so 64 eps of the terms covers them with room.
"""
import numpy as np
from scipy.special import gammaln

from tests import ensemble_cases as ec

EPS = float(np.finfo(np.float64).eps)
MARGIN_EPS = 64.0
INVERSION_CAP = 255
PTRS_FROM = 10.0
MU_MAX = 2.0 ** 52

# the means of the tests: the edges of both samplers and of the switch between them, small and large
POSITIVE = (1e-300, 1e-3, 0.5, 1.0, 9.999, float(np.nextafter(10.0, 0.0)), 10.0, 10.001, 37.5, 1e3, 1e6)
PALETTE = (0.0,) + POSITIVE + (float("nan"),)

_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox(counter, key):
    """Philox4x32-10: `counter` four and `key` two arrays (or numbers) of 32-bit words, held in uint64 -> four arrays"""
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def unit(wa, wb):
    """53 bits of two words -> a double in [0, 1), every operation exact"""
    return ((wa >> np.uint64(5)).astype(np.float64) * 67108864.0 + (wb >> np.uint64(6)).astype(np.float64)) * (
        1.0 / 9007199254740992.0)


def _near(x, y, scale):
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & np.isfinite(y) & (np.abs(x - y) <= MARGIN_EPS * EPS * scale)


def draws(mu, trial, b, stream, seed):
    """The generator on entries: `mu`, `trial` (the trial NUMBER: first_trial + t) and `b` arrays of one shape,
    `stream` and `seed` numbers -> (counts float64, marginal bool, attempts: the largest number of blocks an entry
    used).  A mean without a draw (negative, +inf, above 2^52) gives NaN."""
    mu = np.asarray(mu, dtype=np.float64)
    shape = mu.shape
    mu = mu.ravel()
    trial = np.broadcast_to(np.asarray(trial, dtype=np.uint64), shape).ravel()
    b = np.broadcast_to(np.asarray(b, dtype=np.uint64), shape).ravel()
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    stream = np.uint64(int(stream) & 0xFFFFFFFF)
    out = np.full(mu.shape, np.nan)
    marginal = np.zeros(mu.shape, dtype=bool)
    attempts = 0
    with np.errstate(invalid="ignore"):
        out[mu == 0.0] = 0.0
        small = np.nonzero((mu > 0.0) & (mu < PTRS_FROM))[0]
        big = np.nonzero((mu >= PTRS_FROM) & (mu <= MU_MAX))[0]
    if small.size:
        attempts = 1
        m = mu[small]
        w = philox((b[small], trial[small], stream, 0), key)
        u = unit(w[0], w[1])
        p = np.exp(-m)
        cdf = p.copy()
        prev = np.full(m.shape, np.inf)        # the cdf of the step before (none before the first)
        k = np.zeros(m.shape)
        act = u >= cdf
        while act.any():
            i = np.nonzero(act)[0]
            prev[i] = cdf[i]
            k[i] += 1.0
            p[i] *= m[i] / k[i]
            cdf[i] += p[i]
            act[i] = (u[i] >= cdf[i]) & (k[i] < INVERSION_CAP)
        out[small] = k
        marginal[small] = _near(u, cdf, np.maximum(u, cdf)) | _near(u, prev, np.maximum(u, prev))
    if big.size:
        lam = mu[big]
        slam, loglam = np.sqrt(lam), np.log(lam)
        bq = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * bq
        invalpha = 1.1239 + 1.1328 / (bq - 3.4)
        vr = 0.9277 - 3.6224 / (bq - 2.0)
        res = np.full(lam.shape, np.nan)
        flag = np.zeros(lam.shape, dtype=bool)
        todo = np.arange(lam.size)
        j = 0
        while todo.size:
            i = todo
            w = philox((b[big][i], trial[big][i], stream, j), key)
            U, V = unit(w[0], w[1]) - 0.5, unit(w[2], w[3])
            us = 0.5 - np.abs(U)
            with np.errstate(divide="ignore", invalid="ignore"):
                lead = (2.0 * a[i] / us + bq[i]) * U
                x = lead + lam[i] + 0.43
                k = np.floor(x)
                flag[i] |= _near(x, np.rint(x), np.abs(lead) + lam[i] + 0.43)
                acc1 = (us >= 0.07) & (V <= vr[i])
                rej = (k < 0.0) | ((us < 0.013) & (V > us))
                t1, t2, t3 = np.log(V), np.log(invalpha[i]), np.log(a[i] / (us * us) + bq[i])
                t5, t6 = k * loglam[i], gammaln(k + 1.0)
                lhs, rhs = t1 + t2 - t3, -lam[i] + t5 - t6
                tested = ~acc1 & ~rej
                flag[i] |= tested & _near(lhs, rhs, np.abs(t1) + np.abs(t2) + np.abs(t3) + lam[i] + np.abs(t5) + np.abs(t6))
                acc = acc1 | (tested & (lhs <= rhs))
            res[i[acc]] = k[acc]
            todo = i[~acc]
            j += 1
        attempts = max(attempts, j)
        out[big] = res
        marginal[big] = flag
    return out.reshape(shape), marginal.reshape(shape), attempts


def block(mu_row, n_trials, seed, stream=0, first_trial=0):
    """what one call of the kernel addresses: [n_trials, B] entries of the row `mu_row`, trial numbers from
    `first_trial` -> (counts, marginal)"""
    mu_row = np.asarray(mu_row, dtype=np.float64).ravel()
    t = (np.arange(int(n_trials), dtype=np.uint64) + np.uint64(first_trial))[:, None]
    b = np.arange(mu_row.size, dtype=np.uint64)[None, :]
    shape = (int(n_trials), mu_row.size)
    out, marginal, _ = draws(np.broadcast_to(mu_row[None, :], shape), np.broadcast_to(t, shape),
                             np.broadcast_to(b, shape), stream, seed)
    return out, marginal


def palette_row(n_bins):
    """a row of `n_bins` means cycling through the palette, NaN included"""
    return np.array([PALETTE[i % len(PALETTE)] for i in range(int(n_bins))], dtype=np.float64)


class NumpyDrawSolver(ec.NumpySolver):
    """`ensemble_cases.NumpySolver` plus `draw`: the batch evaluator of `generator="device"` restated in numpy"""

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        self.calls.append(("draw", int(n_trials), int(stream), int(first_trial)))
        return block(mu, n_trials, seed, stream, first_trial)[0]
