"""Shared pieces of the tests of the pseudo-data at nuisances fitted to the observed data (csrc/fluctuate_device.hpp:
`fl_truth_factor`, `fl_truth_mvn`; `pisa_hip_fluctuate_linear_mvn` through `kernels.fluctuate_linear_mvn`;
`fit_observed` and `nuisance="profiled"` / `"fitted"` of pisa_amd/analysis/ensemble.py): the numpy restatement, draw for
draw, on top of tests/truth_cases.py (the truths' counters, the mean, the entries), the case families and a numpy batch
evaluator.  A plain helper module (no fixtures); tests/test_host_observed.py validates it without a GPU,
tests/test_gpu_observed.py holds the kernel to it.

The definition ("pseudo-data at nuisances fitted to the observed data").  Inputs: the fitted
displacements mean [J], their covariance cov [J, J] and the box lower <= mean <= upper.
    factor  a coordinate with cov[j, j] == 0 is dead: its row and column must be zero (else refused), row and column j
            of L are 0.  Over the live coordinates in ascending order plain Cholesky row by row,
                L[i, j] = (cov[i, j] - sum_{k<j} L[i, k] L[j, k]) / L[j, j],
                L[j, j] = sqrt(cov[j, j] - sum_{k<j} L[j, k]^2),
            the sums in ascending k, every operation rounded on its own.  Refused: an entry of cov that is not finite, a
            pivot <= 0 or NaN, an entry of L that is not finite.
    truth   for the attempt r = 0, 1, ...: z_k = PPND16(unit_open(w0, w1)) of the Philox block with the counter
            (0x80000000 + k, trial number, stream, r) for the live k; x_j = mean_j + L[j, 0] z_0 + ... + L[j, j] z_j over
            the live k in ascending order, every product and sum rounded; a dead j has x_j = mean_j.  The first
            candidate with EVERY coordinate inside [lower_j, upper_j] is the trial's truth.  After 256 refused
            candidates the last one is held inside the box coordinate by coordinate and the call is marked exhausted.
    mean, entry  those of tests/truth_cases.py on these truths.

What may differ between this restatement and the kernel is the library's log in the tail branches of AS 241, as in
tests/truth_cases.py: a deviate from the central branch is exact, one from a tail branch lies in the window [z_lo, z_hi]
of `fluctuate_method_cases.normal` (a log within LOG_ULPS of numpy's).  The window goes through the sum by interval
arithmetic: a rounded product L z is monotone in z and a rounded sum is monotone in both terms, so the chain evaluated
on the lower ends of its terms (min(L z_lo, L z_hi)) bounds x_j from below and the one on the upper ends from above,
rounding included.  `truths_mvn` returns that window [lo, hi] per truth -- lo == hi wherever every live deviate up to
j came from the central branch -- and marks a trial `marginal` where some candidate has a coordinate whose place
(inside or outside its box) is not the same over its whole window: a candidate that close to a box edge.

The factor has no library call but sqrt (correctly rounded everywhere): it is compared bit for bit.  Its accuracy is
gated against np.longdouble, |L L^T - cov| <= G_FACTOR eps kappa max|cov| with the product in longdouble and kappa the
2-norm condition number of the live block scaled to a unit diagonal.  G_FACTOR is measured on this restatement over
the families below with J = 1 ... 8 by tests/test_host_observed.py (numpy 2.2: 0.224, at J = 4 with the correlation
0.5 and coordinate 0 dead) and held there; it is not taken from the device.
"""
import numpy as np

from tests import fluctuate_method_cases as fm
from tests import hesse_cases as hc
from tests import truth_cases as tc

ATTEMPTS = tc.ATTEMPTS
METHODS = tc.METHODS
EPS = float(np.finfo(np.float64).eps)
G_FACTOR = 0.23             # worst |L L^T - cov| / (eps kappa max|cov|) of the restatement (module docstring)

COV_KINDS = ("diagonal", "dense", "tight", "one-dead", "all-dead")     # "dense": correlation 0.5, "tight": 0.99
BOX_KINDS = ("none", "one-sided", "two-sided", "held")
# the shapes of the GPU test and their seed, at which the restatement marks nothing marginal and exhausts nothing
# (tests/test_host_observed.py)
SEED, STREAM = 2, 3
TRUTH_SHAPES = tc.TRUTH_SHAPES
DATA_SHAPES = tuple((T, B) for T in (1, 65, 257) for B in (1, 64, 65))
first_trial_of = tc.first_trial_of


def truth_factor(cov, dtype=np.float64):
    """`fl_truth_factor`: L [J, J] in `dtype`, or None where the factor is refused"""
    cov = np.asarray(cov, dtype=dtype)
    J = cov.shape[0]
    L = np.zeros((J, J), dtype=dtype)
    if cov.shape != (J, J) or not 1 <= J <= 8 or not np.isfinite(cov).all():
        return None
    dead = np.diagonal(cov) == 0
    if np.any(cov[dead, :] != 0) or np.any(cov[:, dead] != 0):
        return None
    with np.errstate(all="ignore"):
        for i in range(J):
            if dead[i]:
                continue
            for j in range(i + 1):
                if dead[j]:
                    continue
                s = cov[i, j]
                for k in range(j):
                    t = L[i, k] * L[j, k]
                    s = s - t
                if j < i:
                    s = s / L[j, j]
                else:
                    if not s > 0:
                        return None
                    s = np.sqrt(s)
                if not np.isfinite(s):
                    return None
                L[i, j] = s
    return L


def factor_ratio(cov):
    """|L L^T - cov| of the float64 factor, the product in longdouble, in units of eps kappa max|cov| (0 where no
    coordinate is live)"""
    cov = np.asarray(cov, dtype=np.float64)
    L = truth_factor(cov)
    live = np.diagonal(cov) != 0
    if not live.any():
        return 0.0
    Lx = L.astype(np.longdouble)
    resid = np.abs(Lx @ Lx.T - cov.astype(np.longdouble)).max()
    block = cov[np.ix_(live, live)]
    d = 1.0 / np.sqrt(np.diagonal(block))
    kappa = np.linalg.cond(block * d[:, None] * d[None, :])
    return float(resid / (EPS * kappa * np.abs(cov).max()))


def truths_mvn(mean, L, lower, upper, n_trials, seed, stream=0, first_trial=0, attempts=ATTEMPTS):
    """[n_trials, J] truths -> dict(eta, lo, hi [n_trials, J]: the window the kernel's truth lies in; marginal
    [n_trials] bool; tries [n_trials]: candidates used (0 where no coordinate is live); exhausted: bool)"""
    mean, L = np.asarray(mean, dtype=np.float64), np.asarray(L, dtype=np.float64)
    J, T = mean.size, int(n_trials)
    lower = np.full(J, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
    upper = np.full(J, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
    live = np.nonzero(np.diagonal(L) != 0.0)[0]
    eta = np.broadcast_to(mean[None, :], (T, J)).copy()
    lo, hi = eta.copy(), eta.copy()
    marginal = np.zeros(T, dtype=bool)
    tries = np.zeros(T, dtype=np.int64)
    exhausted = False
    pending = np.arange(T) if live.size else np.arange(0)
    for r in range(int(attempts)):
        if not pending.size:
            break
        trial = pending.astype(np.uint64) + np.uint64(first_trial)
        z = {k: fm.normal(tc.truth_deviates(trial, np.full(pending.size, k), stream, seed, r)) for k in live}
        x = [np.broadcast_to(mean[None, :], (pending.size, J)).copy() for _ in range(3)]        # value, low end, high end
        for j in live:
            for k in live[live <= j]:
                terms = [L[j, k] * v for v in z[k]]
                x[0][:, j] = x[0][:, j] + terms[0]
                x[1][:, j] = x[1][:, j] + np.minimum(terms[1], terms[2])
                x[2][:, j] = x[2][:, j] + np.maximum(terms[1], terms[2])
        inside, in_lo, in_hi = ((lower[None, :] <= v) & (v <= upper[None, :]) for v in x)
        marginal[pending] |= ((in_lo != inside) | (in_hi != inside)).any(axis=1)
        accepted = inside.all(axis=1)
        tries[pending] = r + 1
        if r == int(attempts) - 1 and not accepted.all():
            exhausted = True
            for v in x:
                v[~accepted] = np.clip(v[~accepted], lower[None, :], upper[None, :])
        eta[pending], lo[pending], hi[pending] = x
        pending = pending[~accepted]
    return dict(eta=eta, lo=lo, hi=hi, marginal=marginal, tries=tries, exhausted=exhausted)


def linear_mvn(mu0, sigma_row, R, mean, cov, lower, upper, method, n_trials, seed, stream=0, first_trial=0):
    """the whole call restated -> dict(data, eta, clipped, truths: the dict of `truths_mvn`, block: the tuple of
    `truth_cases.block`); ValueError for a refused factor"""
    L = truth_factor(cov)
    if L is None:
        raise ValueError("linear_mvn: the covariance has no factor")
    tr = truths_mvn(mean, L, lower, upper, n_trials, seed, stream, first_trial)
    blk = tc.block(mu0, sigma_row, R, tr["eta"], method, seed, stream, first_trial)
    return dict(data=blk[0], eta=tr["eta"], clipped=blk[4], truths=tr, block=blk)


# ----------------------------------------------------------------------------------------------- the families
def stddevs(n_params):
    return 0.5 + 0.25 * np.arange(n_params)


def covariance(n_params, kind):
    """[J, J] of one of COV_KINDS: standard deviations 0.5, 0.75, ... and one correlation between all pairs (0, 0.5 or
    0.99); "one-dead": the dense one with the row and column of coordinate J // 2 zero; "all-dead": zeros"""
    assert kind in COV_KINDS
    sd = stddevs(n_params)
    rho = {"diagonal": 0.0, "dense": 0.5, "tight": 0.99, "one-dead": 0.5, "all-dead": 0.0}[kind]
    cov = rho * sd[:, None] * sd[None, :]
    cov[np.diag_indices(n_params)] = sd * sd
    if kind == "one-dead":
        cov[n_params // 2, :] = 0.0
        cov[:, n_params // 2] = 0.0
    elif kind == "all-dead":
        cov[:] = 0.0
    return cov


def case(n_params, cov_kind, box_kind):
    """(mean, cov, lower, upper) [J] / [J, J]: the box in units of the marginal standard deviations about the mean --
    "none"; "one-sided": lower bounds alone, one sigma below the mean; "two-sided": -2 and +2.25 sigma; "held": the
    two-sided box with coordinate 0 dead (its row and column of cov zeroed) and its mean ON its lower bound, what a
    fit that ends on a bound hands over"""
    assert box_kind in BOX_KINDS
    mean = 0.1 * (np.arange(n_params) - 1.0)
    cov = covariance(n_params, cov_kind)
    if box_kind == "held":
        cov[0, :] = 0.0
        cov[:, 0] = 0.0
    sd = np.sqrt(np.diagonal(cov))
    lower, upper = np.full(n_params, -np.inf), np.full(n_params, np.inf)
    if box_kind == "one-sided":
        lower = mean - 1.0 * sd
    elif box_kind in ("two-sided", "held"):
        lower, upper = mean - 2.0 * sd, mean + 2.25 * sd
        if box_kind == "held":
            upper[0] = mean[0] + 1.0
    return mean, cov, lower, upper


def cases(n_params):
    """every covariance kind x every box kind -> ((cov_kind, box_kind), (mean, cov, lower, upper))"""
    return [((c, b), case(n_params, c, b)) for c in COV_KINDS for b in BOX_KINDS]


def exhausting_case(n_params=3):
    """the one family built to show the status word.  The entry point refuses a mean outside its box, so no box can lie
    sigmas away from the mean; the box that no candidate enters is, in coordinate 1, the sliver [mean, mean + 1e-9
    sigma], which holds 4e-10 of the marginal's mass: all 256 candidates of every trial are refused, the last one is held
    inside the box and the call is marked exhausted"""
    mean, cov, lower, upper = case(n_params, "dense", "two-sided")
    lower[1], upper[1] = mean[1], mean[1] + 1e-9 * np.sqrt(cov[1, 1])
    return mean, cov, lower, upper


def data_case(T, B, i):
    """the inputs of data shape number i: (mu0, sigma, R, (mean, cov, lower, upper)); J, the covariance kind and the box
    kind cycle"""
    J = (1, 3, 8)[i % 3]
    mu0, sigma = fm.palette_rows(B)
    return mu0, sigma, tc.responses(J, B, mu0), case(J, COV_KINDS[i % len(COV_KINDS)], BOX_KINDS[i % len(BOX_KINDS)])


def closure_case():
    """T = 4096 truths of J = 3 parameters with the correlation 0.5 and no box -> (mean, cov, T, seed, stream)"""
    mean, cov, _, _ = case(3, "dense", "none")
    return mean, cov, 4096, 11, 2


def closure_limits(cov, T):
    """five standard errors of the sample mean and the sample covariance of T draws from N(., cov): sqrt(cov_jj / T)
    and sqrt((cov_ii cov_jj + cov_ij^2) / T) (the variance of a product of jointly normal deviates, Isserlis)"""
    var = np.diagonal(cov)
    return 5.0 * np.sqrt(var / T), 5.0 * np.sqrt((var[:, None] * var[None, :] + cov * cov) / T)


def check_closure(eta, mean, cov):
    """the gates of the closure test on truths [T, J]: `closure_limits`, asserted"""
    T = eta.shape[0]
    lim_mean, lim_cov = closure_limits(cov, T)
    d_mean = np.abs(eta.mean(axis=0) - mean)
    d_cov = np.abs(np.cov(eta, rowvar=False, ddof=1) - cov)
    print("closure: |mean - m| / limit %s, worst |C - cov| / limit %.2f" % (np.round(d_mean / lim_mean, 2),
                                                                            float(np.max(d_cov / lim_cov))))
    assert np.all(d_mean <= lim_mean) and np.all(d_cov <= lim_cov)


class NumpySolver(tc.NumpyTruthSolver, hc.NumpyHesseSolver):
    """draws through tests/truth_cases.py and this module (`draw_linear_mvn`), fits through
    tests/profile_bounded_cases.py, covariances through tests/hesse_cases.py: the batch evaluator of every mode of
    `nuisance=` restated in numpy"""

    def draw_linear_mvn(self, mu, response, sigma, method, n_trials, seed, stream, mean, cov, lower=None, upper=None,
                        first_trial=0):
        self.calls.append(("draw_linear_mvn", method, int(n_trials), int(stream), int(first_trial)))
        out = linear_mvn(np.asarray(mu, dtype=np.float64).ravel(), sigma, np.asarray(response, dtype=np.float64), mean,
                         cov, lower, upper, method, n_trials, seed, stream, first_trial)
        if out["truths"]["exhausted"]:
            raise ValueError("draw_linear_mvn: a trial found no candidate inside the box")
        return dict(data=out["data"], eta=out["eta"], clipped=out["clipped"])
