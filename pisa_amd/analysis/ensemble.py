"""Trial ensembles on a grid of hypotheses: the metric of MANY pseudo-data maps against MANY templates, and what
frequentist analyses build on it (sensitivity bands, goodness of fit, Feldman-Cousins intervals).

The reference has no such module: an analysis loops `Map.fluctuate` + `Map.metric_total` (pisa/core/map.py:1098-1254,
1572-1604) over trials and hypotheses.  Here the templates of a grid are made once (`TemplateGrid.from_maker`: one
sweep of the events per `MAX_POINTS` points where the pipeline allows it), the pseudo-data of a true point are drawn
(`pseudo_data`), and the T x K metric values come from one launch (`kernels.metric_matrix`), or never exist at all
(`kernels.metric_matrix_best`: best, arg and the value at the true point per trial).  `METRICS` are llh, poisson_llh,
chi2 and mod_chi2 and the four metrics that account for finite MC statistics, correct_chi2, mcllh_mean, mcllh_eff and
conv_llh (csrc/ensemble_mc.hip: they read the templates' `sumw2`, and `response=` is refused with them).

Two generators draw the pseudo-data.  `generator="host"` (the default) is the reference's `RandomState` stream: trial
t is the t-th `Map.fluctuate("poisson")`, drawn by scipy on the host and uploaded.  `generator="device"` is the
counter-based generator of csrc/fluctuate.hip (`kernels.poisson_fluctuate`: Philox4x32-10, inversion below a mean of
10 and Hoermann's PTRS from there on): the draws are made where the metric kernels read them and never visit the
host.  It cannot reproduce the reference's stream, so it has its own definition, restated draw for draw
in tests/fluctuate_cases.py and validated statistically there.  Its entry (trial, bin) depends on (seed, stream = index
of the true point, trial number, bin, mean) alone, so the result of `feldman_cousins` does not depend on how the
trials are chunked.

Both generators draw by any of `FLUCTUATE_METHODS` (`method=`, default "poisson"), the methods of `Map.fluctuate`
(pisa/core/map.py:1118-1254): "gauss" and "gauss+poisson" also carry the template's MC-statistical error sqrt(sumw2)
-- the pseudo-data a calibration of the MC-uncertainty metrics needs --, "scaled_poisson" is Bohm & Zech's scaled
Poisson process with the template's mean and variance.  The host generator is the loop over `Map.fluctuate(method)`
on one `RandomState`, trial by trial (the Gaussian and the Poisson draws alternate in the stream).  The device
generator draws through `solver.fluctuate` (`kernels.fluctuate`, `pisa_hip_fluctuate`): a normal deviate per entry
from a Philox block of its own through AS 241, defined in csrc/fluctuate_device.hpp and DESIGN.md §4 and restated in
tests/fluctuate_method_cases.py.  The row rules of "scaled_poisson" (errors missing: their Poisson expectation;
variance equal to the mean: the plain Poisson call) are applied per template row on the host before the launch.

Nuisance parameters are profiled in two ways.  A dimension of the grid is profiled by `delta_metric` taking the best
value over the grid's points.  A free parameter that is NOT a dimension of the grid is fitted per (trial, point) pair
where a `NuisanceResponse` is passed (`response=`): the template of point k is linearised in those parameters around
the point, mu = hist[k] + sum_j response[k, j] eta_j with the binwise gradients of `DistributionMaker._fisher_templates`
(`NuisanceResponse.from_maker`), and the displacements eta are fitted by the damped Newton iteration of
csrc/profile.hip (`kernels.profiled_metric_matrix`, at most 8 parameters, or 32 in the wide form a response asks for
with `wide=True`; Gaussian priors included; DESIGN.md §4, "Profiled trial ensembles") -- T x K small convex fits in one launch, no minimiser on the host.  The fit is exact for
a parameter the template is linear in (aeff_scale) and a first-order profile otherwise.  A response with bounds
(`NuisanceResponse(..., lower=, upper=)`, `from_maker(..., bounded=True)`: the parameters' ranges as displacements
from the point's values) fits every eta inside them, as a host minimiser working in the rescaled box [0, 1] would
(csrc/profile_bounded.hip; DESIGN.md §4, "Profiled trial ensembles: bounds"): a fitted coordinate on a bound equals
the bound, and a response without bounds is fitted as before.  Without `response` a parameter that is not a dimension
of the grid stays at the value it had when the grid was made, and every call gives what it gave before the argument
existed.

The batch evaluator is an argument (`solver=`, default `DeviceSolver`): an object with
    matrix(kind, data, expected, sigma2) -> [T, K]
    best(kind, data, expected, sigma2, offset, k0) -> (best [T], arg [T], at [T])
and, for `generator="device"`,
    draw(mu [B], n_trials, seed, stream, first_trial=0) -> [n_trials, B]
and, for `generator="device"` with another method than "poisson",
    fluctuate(mu [B], sigma [B], method, n_trials, seed, stream, first_trial=0) -> [n_trials, B]
and, for `response=`,
    profiled_matrix(kind, data, expected, response, sigma2, inv_prior_sigma, center, max_iter)
        -> dict(value [T, K], eta [T, K, J], n_iter [T, K], status [T, K])
    profiled_best(kind, data, expected, response, sigma2, inv_prior_sigma, center, offset, k0, max_iter)
        -> dict(best [T], arg [T], at [T], eta_best [T, J], eta_at [T, J], status [T])
and, for a `response` that has bounds, the same two methods with the keywords
    lower=, upper=  ([J] or [K, J] host arrays of displacements, -inf / +inf for no bound)
which the drivers pass ONLY for such a response: a solver that knows nothing of bounds keeps working with responses
that have none, and a bounded response on it is refused,
and, for a wide `response` (`NuisanceResponse(..., wide=True)`: up to 32 parameters), the same two methods with
    wide=True
(csrc/profile_wide.hip, `kernels.profiled_metric_matrix_wide`: one wavefront per pair, the bits of the narrow fit up to 8
parameters), passed ONLY for such a response in the same way; what reads a kernel that stays limited to 8 parameters --
`hesse`, `posterior`, `draw_linear`, `draw_linear_mvn`, `draw_linear_at` -- is refused for a response with more,
and, for a log-linear `response` (`NuisanceResponse(..., form="loglinear")`: templates hist * exp(rho . eta), 1 to 32
parameters, always fitted by the wide form), the same two methods with
    form="loglinear"
(csrc/profile_loglinear.hip, `kernels.profiled_metric_matrix_wide(..., form=)`), passed ONLY for such a response; the
host generator forms its means by the response's form, and what reads a linear kernel -- `hesse`, `posterior`,
`draw_linear`, `draw_linear_mvn`, `draw_linear_at` -- is refused for it by a ValueError that says "log-linear",
and, for `generator="device"` with `nuisance="prior"`,
    draw_linear(mu [B], response [J, B], sigma [B] or None, method, n_trials, seed, stream, scale, shift, lower, upper
                ([J] host arrays; lower / upper may be None), first_trial=0)
        -> dict(data [n_trials, B], eta [n_trials, J], clipped)
(`nuisance="profiled"` draws through it as well, with every scale 0), and, for `generator="device"` with
`nuisance="fitted"`,
    draw_linear_mvn(mu [B], response [J, B], sigma [B] or None, method, n_trials, seed, stream, mean [J], cov [J, J],
                    lower, upper ([J] host arrays; either may be None), first_trial=0)
        -> dict(data [n_trials, B], eta [n_trials, J], clipped)
and, for `covariance=True`, `pulls` and `nuisance="fitted"`,
    hesse(kind, data, expected, response, eta [T, J], k (an int or [T] ints), sigma2, inv_prior_sigma, center,
          lower=, upper=) -> dict(cov [T, J, J], sigma [T, J], status [T])
and, for `posterior_sample`,
    posterior(kind, data, expected, response, x0 [P, W, J], n_steps, seed, t_of, k_of ([P] ints or None), sigma2,
              inv_prior_sigma, center, lower, upper, stream, chain_id ([P] ints or None), first_step, keep_from, thin)
        -> dict(chain [P, n_keep, W, J], logp [P, n_keep, W], accepted [P, W], end [P, W, J], status [P])
and, for `generator="device"` with `truths=`,
    draw_linear_at(mu [B], response [J, B], sigma [B] or None, method, eta [n_trials, J], seed, stream, first_trial=0)
        -> dict(data [n_trials, B], eta [n_trials, J], clipped)
so that everything around the kernels can run with a numpy restatement (tests/ensemble_cases.py,
tests/fluctuate_cases.py, tests/fluctuate_method_cases.py, tests/profile_cases.py, tests/truth_cases.py,
tests/hesse_cases.py, tests/observed_cases.py, tests/posterior_cases.py).

`nuisance="prior"` (`pseudo_data`, `feldman_cousins`; needs `response=`) makes pseudo-experiments with the systematics
fluctuated: every trial draws the truths of the response's parameters from their priors and its data from the
linearised template at those truths (csrc/fluctuate_linear.hip; DESIGN.md §4, "pseudo-data with drawn nuisance
truths"), where the default `nuisance="fixed"` leaves them at the point's values.  `delta_metric(..., covariance=True)`
returns the covariance of the fitted displacements (csrc/profile_hesse.hip; "covariance and pulls") and `pulls` the
distribution (eta_hat - eta_true) / sigma_hat an analyst checks a profiled ensemble with.

Once a data map exists, two more modes generate at the nuisance values that map prefers (`observed=`, with
`response=`; DESIGN.md §4, "pseudo-data at nuisances fitted to the observed data").  `fit_observed` fits the observed
map at every point of the grid in one launch: eta_obs [K, J], and with `covariance=True` the fit's covariance cov_obs
[K, J, J].  `nuisance="profiled"` is the profile construction of a Feldman-Cousins analysis with systematics: the
pseudo-data of true point k are drawn from hist[k] + sum_j response[k, j] eta_obs[k, j], the same truths in every
trial -- the generator of "prior" with every scale 0 and the shift eta_obs[k].  `nuisance="fitted"` draws every
trial's truths from the fit's Gaussian N(eta_obs[k], cov_obs[k]) truncated to the response's box: the truths are
CORRELATED, so the whole vector is drawn and rejected at once (`fl_truth_factor`, `fl_truth_mvn` of
csrc/fluctuate_device.hpp; `kernels.fluctuate_linear_mvn`), and a coordinate the fit holds on a bound (a zero row and
column of cov_obs[k]) stays on it.

The true posterior of the displacements -- skewed at few counts, flat inside a box, free to move where the fit sits on
a bound, none of which the fit's Gaussian can be -- is sampled by `posterior_sample`: a Goodman-Weare stretch-move
ensemble sampler, one chain ensemble per grid point and every step of every point in ONE launch (csrc/posterior.hip,
`kernels.posterior_sample`; DESIGN.md §4, "Trial ensembles: the nuisance posterior") -> a `PosteriorSample` with the
samples, their integrated autocorrelation time (`autocorr_time`) and credible intervals.  Pseudo-experiments at such
samples enter through `truths=` of `pseudo_data` and `feldman_cousins` (a `PosteriorSample`, or rows of displacements
of the caller's own): trial number n is generated at row n of the true point's truths, the posterior-predictive
ensemble.  `nuisance="posterior"` stays an unknown name: the posterior lives in `posterior_sample` and `truths=`, and
the reference's full-model `MCMC_sampling` (analysis/bayesian_analysis.py: templates re-made per walker) is not this.
"""
import math

import numpy as np

from pisa_amd.core.map import FLUCTUATE_METHODS
from pisa_amd.utils.comparisons import ALLCLOSE_KW

__all__ = ["METRICS", "GENERATORS", "FLUCTUATE_METHODS", "DeviceSolver", "TemplateGrid", "NuisanceResponse", "grid_points", "pseudo_data",
           "metric_matrix", "delta_metric", "pulls", "critical_values", "feldman_cousins", "accepted", "NUISANCE", "fit_observed",
           "posterior_sample", "PosteriorSample", "autocorr_time"]

# kernels.METRIC_KIND, then kernels.ENSEMBLE_MC_KINDS: the metrics that account for finite MC statistics, which read
# the templates' sumw2 and have no profiled form
METRICS = ("llh", "poisson_llh", "chi2", "mod_chi2", "correct_chi2", "mcllh_mean", "mcllh_eff", "conv_llh")
_MC_METRICS = METRICS[4:]
_MAXIMISED = ("llh", "poisson_llh", "mcllh_mean", "mcllh_eff", "conv_llh")


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError("ensemble: metric '%s' not among %s" % (metric, list(METRICS)))


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


class DeviceSolver:
    """the default batch evaluator: `kernels.metric_matrix` / `metric_matrix_best`.  Host arrays are uploaded, device
    tensors are used as they are; device tensors come back."""

    def __init__(self, form="auto"):
        self.form = form

    def _up(self, a):
        import torch

        from pisa_amd import kernels as K

        if a is None or isinstance(a, torch.Tensor):
            return a
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(K.device())

    def _run(self, fn, kind, arrays, **kw):
        return fn(kind, *[self._up(a) for a in arrays], form=self.form, **kw)

    def matrix(self, kind, data, expected, sigma2=None):
        from pisa_amd import kernels as K

        return self._run(K.metric_matrix, kind, (data, expected, sigma2))

    def best(self, kind, data, expected, sigma2=None, offset=None, k0=0):
        from pisa_amd import kernels as K

        return self._run(K.metric_matrix_best, kind, (data, expected, sigma2, offset), k0=int(k0))

    def profiled_matrix(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                        max_iter=32, lower=None, upper=None, wide=False, form="linear"):
        """wide=True: the wide form (`kernels.profiled_metric_matrix_wide`, up to 32 parameters), whatever J.
        form: "linear", or "loglinear" (`response` holds rho, the template is expected * exp(rho . eta)); any other
        form than "linear" runs the wide kernels"""
        from pisa_amd import kernels as K

        data, expected, response, sigma2, ips, center, lower, upper = [self._up(a) for a in (
            data, expected, response, sigma2, inv_prior_sigma, center, lower, upper)]
        if form != "linear":
            return K.profiled_metric_matrix_wide(kind, data, expected, response, sigma2, ips, center,
                                                 max_iter=max_iter, lower=lower, upper=upper, form=form)
        fn = K.profiled_metric_matrix_wide if wide else K.profiled_metric_matrix
        return fn(kind, data, expected, response, sigma2, ips, center, max_iter=max_iter, lower=lower, upper=upper)

    def profiled_best(self, kind, data, expected, response, sigma2=None, inv_prior_sigma=None, center=None,
                      offset=None, k0=0, max_iter=32, lower=None, upper=None, wide=False, form="linear"):
        from pisa_amd import kernels as K

        data, expected, response, sigma2, ips, center, offset, lower, upper = [self._up(a) for a in (
            data, expected, response, sigma2, inv_prior_sigma, center, offset, lower, upper)]
        if form != "linear":
            return K.profiled_metric_matrix_best_wide(kind, data, expected, response, sigma2, ips, center, offset,
                                                      int(k0), max_iter=max_iter, lower=lower, upper=upper, form=form)
        fn = K.profiled_metric_matrix_best_wide if wide else K.profiled_metric_matrix_best
        return fn(kind, data, expected, response, sigma2, ips, center, offset, int(k0), max_iter=max_iter, lower=lower,
                  upper=upper)

    def hesse(self, kind, data, expected, response, eta, k, sigma2=None, inv_prior_sigma=None, center=None, lower=None,
              upper=None):
        """dict(cov [T, J, J], sigma [T, J], status [T]): the covariance of the displacements eta [T, J] fitted at the
        template k (one int, or [T] ints: the fit's `arg`) of every trial (`kernels.profiled_hesse`)"""
        import torch

        from pisa_amd import kernels as K

        data, expected, response, eta, sigma2, ips, center, lower, upper = [self._up(a) for a in (
            data, expected, response, eta, sigma2, inv_prior_sigma, center, lower, upper)]
        if not isinstance(k, (int, np.integer)):
            k = k if isinstance(k, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(k, dtype=np.int32))
            k = k.to(device=data.device, dtype=torch.int32)
        return K.profiled_hesse(kind, data, expected, response, eta, k, sigma2, ips, center, lower, upper)

    def draw(self, mu, n_trials, seed, stream, first_trial=0):
        """[n_trials, B] Poisson draws of the row `mu` on the device (`kernels.poisson_fluctuate`)"""
        from pisa_amd import kernels as K

        return K.poisson_fluctuate(self._up(mu).reshape(-1), n_trials, seed, stream=stream, first_trial=first_trial)

    def fluctuate(self, mu, sigma, method, n_trials, seed, stream, first_trial=0):
        """[n_trials, B] draws of the row `mu` with the standard deviations `sigma` by `method` on the device
        (`kernels.fluctuate`)"""
        from pisa_amd import kernels as K

        return K.fluctuate(self._up(mu).reshape(-1), n_trials, seed, method=method, sigma=self._up(sigma).reshape(-1),
                           stream=stream, first_trial=first_trial)

    def draw_linear(self, mu, response, sigma, method, n_trials, seed, stream, scale, shift, lower=None, upper=None,
                    first_trial=0):
        """dict(data [n_trials, B], eta [n_trials, J], clipped): every trial's nuisance truths drawn from N(shift,
        scale) inside [lower, upper] and its data by `method` from mu + sum_j response[j] eta_j on the device
        (`kernels.fluctuate_linear`); for "poisson" sigma is None"""
        from pisa_amd import kernels as K

        sigma = None if sigma is None else self._up(sigma).reshape(-1)
        return K.fluctuate_linear(self._up(mu).reshape(-1), self._up(response), n_trials, seed, scale, shift, lower,
                                  upper, method=method, sigma=sigma, stream=stream, first_trial=first_trial)

    def draw_linear_mvn(self, mu, response, sigma, method, n_trials, seed, stream, mean, cov, lower=None, upper=None,
                        first_trial=0):
        """`draw_linear` with every trial's truths drawn from N(mean [J], cov [J, J]) inside [lower, upper], the whole
        vector rejected (`kernels.fluctuate_linear_mvn`)"""
        from pisa_amd import kernels as K

        sigma = None if sigma is None else self._up(sigma).reshape(-1)
        return K.fluctuate_linear_mvn(self._up(mu).reshape(-1), self._up(response), n_trials, seed, mean, cov, lower,
                                      upper, method=method, sigma=sigma, stream=stream, first_trial=first_trial)

    def draw_linear_at(self, mu, response, sigma, method, eta, seed, stream, first_trial=0):
        """`draw_linear` at given truths: eta [n_trials, J], row t the truths of trial number first_trial + t; nothing
        is drawn for them (`kernels.fluctuate_linear_at`) -> dict(data [n_trials, B], eta, clipped)"""
        from pisa_amd import kernels as K

        sigma = None if sigma is None else self._up(sigma).reshape(-1)
        return K.fluctuate_linear_at(self._up(mu).reshape(-1), self._up(response), self._up(eta), seed, method=method,
                                     sigma=sigma, stream=stream, first_trial=first_trial)

    def posterior(self, kind, data, expected, response, x0, n_steps, seed, t_of=None, k_of=None, sigma2=None,
                  inv_prior_sigma=None, center=None, lower=None, upper=None, stream=0, chain_id=None, first_step=0,
                  keep_from=0, thin=1):
        """dict(chain [P, n_keep, W, J], logp [P, n_keep, W], accepted [P, W], end [P, W, J], status [P]): the
        stretch-move chains of P problems from the starts x0 [P, W, J] (`kernels.posterior_sample`); t_of, k_of and
        chain_id: [P] ints or None"""
        import torch

        from pisa_amd import kernels as K

        data, expected, response, x0, sigma2, ips, center, lower, upper = [self._up(a) for a in (
            data, expected, response, x0, sigma2, inv_prior_sigma, center, lower, upper)]

        def ints(a, dtype):
            if a is None or isinstance(a, torch.Tensor):
                return a
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device=data.device, dtype=dtype)

        return K.posterior_sample(kind, data, expected, response, x0, n_steps, seed, ints(t_of, torch.int32),
                                  ints(k_of, torch.int32), sigma2, ips, center, lower, upper, stream,
                                  ints(chain_id, torch.int64), first_step, keep_from, thin)


def _rescaled(param, value):
    """the [0, 1]-rescaled value `param` would have at `value` (param.py:358-377) without moving it"""
    if param._range is None:
        raise ValueError("Cannot rescale without a range specified for parameter %s" % param.name)
    v = value.m_as(param._units) if hasattr(value, "m_as") else float(value)
    r0, r1 = param._range[0].m_as(param._units), param._range[1].m_as(param._units)
    if param.scales_as_log:
        if r0 < 0:
            r0, r1, v = -r0, -r1, -v
        r = (np.log(v) - np.log(r0)) / (np.log(r1) - np.log(r0))
    else:
        r = (v - r0) / (r1 - r0)
    if not -1e-12 <= r <= 1 + 1e-12:
        raise ValueError("%s: %s is outside the parameter's range" % (param.name, value))
    return float(min(max(r, 0.0), 1.0))


def grid_points(hypo_maker, axes):
    """The cartesian product of `axes` = {name of a free parameter: values (numbers in the parameter's units, or
    quantities)} as [K, n_free] values of the free parameters rescaled to [0, 1], in the order of
    `hypo_maker.params.free`; the LAST name of `axes` runs fastest.  Free parameters that are not named stay at
    their current value."""
    free = hypo_maker.params.free
    names = list(free.names)
    base = np.array([float(p._rescaled_value) for p in free], dtype=np.float64)
    cols, vals = [], []
    for name, values in axes.items():
        if name not in names:
            raise ValueError("grid_points: '%s' is not a free parameter (%s)" % (name, names))
        if hasattr(values, "m_as"):                 # a quantity holding an array: numbers in the parameter's units
            values = values.m_as(free[name]._units)
        seq = list(values) if isinstance(values, (list, tuple)) else list(np.atleast_1d(values))
        v = [_rescaled(free[name], x) for x in seq]
        if not v:
            raise ValueError("grid_points: no values for '%s'" % name)
        cols.append(names.index(name))
        vals.append(np.asarray(v, dtype=np.float64))
    if len(set(cols)) != len(cols):
        raise ValueError("grid_points: a parameter is named twice")
    n = int(np.prod([v.size for v in vals])) if vals else 1
    pts = np.tile(base, (n, 1))
    if vals:
        mesh = np.meshgrid(*vals, indexing="ij")
        for c, m in zip(cols, mesh):
            pts[:, c] = m.ravel()
    return pts


class TemplateGrid:
    """The templates of K points of the free parameters: `hist` and `sumw2` [K, B] (device tensors from
    `from_maker`; any arrays the solver takes otherwise), `points` [K, n_free] rescaled, the output `binning` and
    `penalty` [K] = params.priors_penalty(metric) at each point."""

    def __init__(self, hist, sumw2, points, binning=None, penalty=None, metric=None, sweeps=0):
        self.hist, self.sumw2 = hist, sumw2
        self.points = np.atleast_2d(np.asarray(points, dtype=np.float64))
        self.binning = binning
        n = int(self.hist.shape[0])
        self.penalty = np.zeros(n) if penalty is None else np.asarray(penalty, dtype=np.float64)
        self.metric = metric
        self.sweeps = sweeps
        self._host = {}
        if self.sumw2 is not None and tuple(self.sumw2.shape) != tuple(self.hist.shape):
            raise ValueError("TemplateGrid: sumw2 has the shape of hist")
        if self.penalty.shape != (n,) or self.points.shape[0] != n:
            raise ValueError("TemplateGrid: one point and one penalty per template")

    def __len__(self):
        return int(self.hist.shape[0])

    n_bins = property(lambda self: int(self.hist.shape[1]))

    def host(self, which="hist"):
        """`hist` / `sumw2` as a host array (fetched once)"""
        if which not in self._host:
            self._host[which] = _host(getattr(self, which))
        return self._host[which]

    def sigma2_for(self, metric):
        return self.sumw2 if metric == "mod_chi2" or metric in _MC_METRICS else None

    @classmethod
    def from_maker(cls, hypo_maker, rescaled_points, metric):
        """The templates of `hypo_maker` at `rescaled_points` [K, n_free].  One pipeline of the replayable shape
        whose moving parameters belong to osc.prob3 / aeff.aeff takes the points through `FastPlan.maps_many` (one
        sweep of the events per MAX_POINTS points) and the containers are added in ascending row order; anything
        else (a flux, KDE or post-histogram stage moving, several pipelines) takes one
        `get_outputs(return_sum=True)` per point.  Either way row k of `hist` is, bit for bit,
        `get_outputs(return_sum=True)["total"].nominal_values` at point k and row k of `sumw2` its variances (zeros
        where the maps carry no errors).  On return the free parameters hold the values they had at entry."""
        from pisa_amd import kernels as K

        _check_metric(metric)
        pts = np.clip(np.atleast_2d(np.asarray(rescaled_points, dtype=np.float64)), 0.0, 1.0)
        n_free = len(hypo_maker.params.free)
        if pts.ndim != 2 or pts.shape[1] != n_free or pts.shape[0] < 1:
            raise ValueError("TemplateGrid: points are [K, %d] rescaled values of the free parameters" % n_free)
        n = pts.shape[0]
        saved = [p.value for p in hypo_maker.params.free]
        pens = np.zeros(n)

        def set_point(i):
            hypo_maker._set_rescaled_free_params(pts[i])
            pens[i] = hypo_maker.params.priors_penalty(metric=metric)

        pipes = hypo_maker._pipelines
        try:
            first = hypo_maker.get_outputs(return_sum=True)      # (also builds the replay plan)
            if isinstance(first, list):
                raise NotImplementedError("TemplateGrid of a pipeline with a variable binning (one MapSet per "
                                          "selection)")
            binning = first["total"].binning
            n_bins = int(np.asarray(first["total"].nominal_values).size)
            hist = var = None
            sweeps = 0
            if len(pipes) == 1 and pipes[0].fast_path and pipes[0]._plan is not None and n >= 2:
                pipe, plan = pipes[0], pipes[0]._plan
                try:
                    maps = plan.maps_many(set_point, n)
                except BaseException:
                    pipe._plan = None
                    plan.invalidate()
                    raise
                if maps is not None:
                    # MapSet.total(): the containers' rows added in ascending order, starting from row 0
                    h, v = maps["hist"].cpu().numpy(), maps["sumw2"].cpu().numpy()
                    hist, var = h[:, 0].copy(), v[:, 0].copy()
                    for r in range(1, h.shape[1]):
                        hist += h[:, r]
                        var += v[:, r]
                    sweeps = maps["sweeps"]
            if hist is None:
                hist, var = np.empty((n, n_bins)), np.empty((n, n_bins))
                for i in range(n):
                    set_point(i)
                    out = hypo_maker.get_outputs(return_sum=True)
                    if isinstance(out, list):
                        raise NotImplementedError("TemplateGrid of a pipeline with a variable binning")
                    m = out["total"]
                    hist[i] = np.asarray(m.nominal_values, dtype=np.float64).ravel()
                    var[i] = np.asarray(m.variances, dtype=np.float64).ravel()
        finally:
            hypo_maker.set_free_params(saved)
        grid = cls(K.to_device(hist), K.to_device(var), pts, binning, pens, metric, sweeps)
        grid._host = {"hist": hist, "sumw2": var}
        return grid


class NuisanceResponse:
    """The linear response of the templates of a grid to J <= 8 (`wide=True`: J <= 32) nuisance parameters that are not
    dimensions of the grid: `names` [J]; `response` [K, J, B] (or [J, B], shared by all points) the change of the template per unit of
    the parameter (its magnitude in the parameter's units); `inv_prior_sigma` [J] = 1 / stddev of a Gaussian prior,
    0 without one; `center` [K, J] the parameter's value at point k minus its prior mean; `prior_at_point` [K] the
    named parameters' share of `priors_penalty` at point k, which the drivers take out of `grid.penalty` (the fit
    adds the prior at the FITTED value: no prior is counted twice); `values` [K, J] the parameters' values at the
    points, to which a fitted displacement eta is added; `lower` / `upper` [J] or [K, J] host arrays (either may be
    None): the box lower <= eta <= upper every displacement is fitted in, -inf / +inf for no bound (a NaN, or lower >
    upper, raises ValueError).  Arrays of whatever kind the solver takes.  `wide=True` takes 1 to 32 parameters and has
    the drivers fit them with the wide form of the solver (`wide=True` of `profiled_matrix` / `profiled_best`;
    csrc/profile_wide.hip), whatever J; what goes through a kernel limited to 8 parameters (covariances, pulls,
    nuisance="fitted", `posterior_sample`, the device generator's nuisance draws) is then refused above 8.
    `form="loglinear"`: the multiplicative response mu_kb(eta) = hist_kb exp(sum_j rho_kjb eta_j), with rho held in
    `response` ([K, J, B] or [J, B]); the template stays positive and keeps the cross terms of a product of factors
    (csrc/profile_loglinear.hip; DESIGN.md §4, "Profiled trial ensembles: the log-linear response").  A log-linear
    response is wide whatever `wide=` says: it takes 1 to 32 names and is fitted by the wide form of the solver, which
    gets form="loglinear".  What reads a kernel that is linear -- covariances, pulls, nuisance="fitted",
    `posterior_sample`, the device generator with drawn or given truths -- is refused for it, whatever J."""

    def __init__(self, names, response, inv_prior_sigma=None, center=None, prior_at_point=None, values=None,
                 max_iter=32, lower=None, upper=None, wide=False, form="linear"):
        if form not in FORMS:
            raise ValueError("NuisanceResponse: form '%s' is not one of %s" % (form, list(FORMS)))
        self.names = tuple(names)
        self.form = form
        self.wide = bool(wide) or form != "linear"
        self.response = response
        n_j = len(self.names)
        if len(response.shape) not in (2, 3) or int(response.shape[-2]) != n_j:
            raise ValueError("NuisanceResponse: response is [K, %d, B] or [%d, B] for %d names" % (n_j, n_j, n_j))
        if self.wide and not 1 <= n_j <= WIDE_MAX_PARAMS:
            raise ValueError("NuisanceResponse: 1 to %d parameters with wide=True, got %d" % (WIDE_MAX_PARAMS, n_j))
        if not self.wide and not 1 <= n_j <= MAX_PARAMS:
            raise ValueError("NuisanceResponse: 1 to 8 parameters, got %d" % n_j)
        self.inv_prior_sigma = np.zeros(n_j) if inv_prior_sigma is None else np.asarray(inv_prior_sigma, np.float64)
        self.center = None if center is None else np.asarray(center, dtype=np.float64)
        self.prior_at_point = None if prior_at_point is None else np.asarray(prior_at_point, dtype=np.float64)
        self.values = None if values is None else np.asarray(values, dtype=np.float64)
        self.max_iter = int(max_iter)
        if self.inv_prior_sigma.shape != (n_j,) or np.any(self.inv_prior_sigma < 0):
            raise ValueError("NuisanceResponse: inv_prior_sigma holds one value >= 0 per parameter")
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64)
        shapes = [(n_j,)] + ([(int(response.shape[0]), n_j)] if len(response.shape) == 3 else [])
        for name, b in (("lower", self.lower), ("upper", self.upper)):
            if b is None:
                continue
            if b.ndim == 2 and len(shapes) == 1:
                shapes.append((b.shape[0], n_j))        # (a shared response: K is the bounds' own)
            if b.shape not in shapes:
                raise ValueError("NuisanceResponse: %s is [%d] or [K, %d], got %s" % (name, n_j, n_j, b.shape))
            if np.isnan(b).any():
                raise ValueError("NuisanceResponse: %s holds a NaN" % name)
        if self.lower is not None and self.upper is not None:
            if self.lower.ndim != self.upper.ndim:         # one form for both: the kernels take one stride
                n_k = (self.lower if self.lower.ndim == 2 else self.upper).shape[0]
                self.lower = np.ascontiguousarray(np.broadcast_to(self.lower, (n_k, n_j)))
                self.upper = np.ascontiguousarray(np.broadcast_to(self.upper, (n_k, n_j)))
            if self.lower.shape != self.upper.shape:
                raise ValueError("NuisanceResponse: lower %s and upper %s do not fit" % (self.lower.shape,
                                                                                         self.upper.shape))
            if np.any(self.lower > self.upper):
                raise ValueError("NuisanceResponse: lower > upper")

    bounded = property(lambda self: self.lower is not None or self.upper is not None)

    def bounds(self):
        """the keywords a driver passes to the solver's profiled methods: none for a response without bounds"""
        return dict(lower=self.lower, upper=self.upper) if self.bounded else {}

    def fit_keywords(self):
        """the keywords a driver passes to `profiled_matrix` and `profiled_best`: the bounds of a response that has
        some, wide=True for a wide response, form= for a response that is not linear, nothing otherwise"""
        kw = dict(self.bounds(), wide=True) if self.wide else self.bounds()
        return dict(kw, form=self.form) if self.form != "linear" else kw

    def offset(self, grid):
        """grid.penalty without the named parameters' share, or None if that is zero everywhere"""
        off = grid.penalty if self.prior_at_point is None else grid.penalty - self.prior_at_point
        return off if np.any(off != 0.0) else None

    @classmethod
    def from_maker(cls, hypo_maker, grid, names, test_vals, max_iter=32, bounded=False, wide=False, form="linear"):
        """The response of `grid`'s templates to the free parameters `names` of `hypo_maker`: at every point of
        `grid.points` the gradients (T_hi - T_lo) / (hi - lo) of `hypo_maker._fisher_templates` (one call per
        parameter, every other parameter at the point's own value; one sweep of the events each where the pipeline
        has the replayable shape) between the point's own value + test_vals[name][0] and + test_vals[name][1]
        (displacements: numbers in the parameter's units, or quantities).  1 / sigma and
        the mean are read from a Gaussian prior; a uniform prior (or none) gives 0; any other kind raises
        ValueError.  bounded=True: every displacement is fitted inside the parameter's `range`, lower[k, j] =
        range_j[0] - values[k, j] and upper[k, j] = range_j[1] - values[k, j] in the parameter's units (-inf / +inf
        for a parameter without a range).  wide=True: as in the constructor, up to 32 names.  form="loglinear": the
        response holds rho[k, j, b] = grad[k, j, b] / hist[k, b] where the point's own template hist[k, b] > 0 and 0
        elsewhere (the same gradients, read as logarithmic derivatives), and is wide.  On return the free
        parameters hold the values they had at entry."""
        from pisa_amd import kernels as K

        if form not in FORMS:
            raise ValueError("NuisanceResponse: form '%s' is not one of %s" % (form, list(FORMS)))
        names = list(names)
        wide = bool(wide) or form != "linear"
        most = WIDE_MAX_PARAMS if wide else MAX_PARAMS
        if not 1 <= len(names) <= most:      # (before any template is made)
            raise ValueError("NuisanceResponse: 1 to %d parameters%s, got %d"
                             % (most, " with wide=True" if wide else "", len(names)))
        free = hypo_maker.params.free
        for name in names:
            if name not in free.names:
                raise ValueError("NuisanceResponse: '%s' is not a free parameter (%s)" % (name, list(free.names)))
        if len(set(names)) != len(names):
            raise ValueError("NuisanceResponse: a parameter is named twice")
        ips, means = np.zeros(len(names)), np.zeros(len(names))
        for j, name in enumerate(names):
            prm = free[name]
            kind = "uniform" if prm.prior is None else prm.prior.kind
            if kind == "gaussian":
                ips[j] = 1.0 / float(prm.prior.stddev.to(prm._units).magnitude)
                means[j] = float(prm.prior.mean.to(prm._units).magnitude)
            elif kind != "uniform":
                raise ValueError("NuisanceResponse: the %s prior of '%s' is not quadratic; only Gaussian and uniform "
                                 "priors can be profiled" % (kind, name))
        n = len(grid)
        saved = [p.value for p in free]
        resp = np.empty((n, len(names), grid.n_bins))
        values, at_point = np.zeros((n, len(names))), np.zeros(n)
        pipes = hypo_maker._pipelines
        try:
            for k in range(n):
                hypo_maker._set_rescaled_free_params(grid.points[k])
                tv = {}
                for j, name in enumerate(names):
                    prm = hypo_maker.params[name]
                    at_point[k] += prm.prior_penalty(grid.metric)
                    here = prm.value
                    values[k, j] = float(here.m_as(prm._units))
                    tv[name] = [here + (d if hasattr(d, "m_as") else d * here.units) for d in test_vals[name]]
                    lo, hi = (t.m_as(prm._units) for t in tv[name])
                    if not lo != hi:
                        raise ValueError("NuisanceResponse: the two test values of '%s' coincide" % name)
                    tv[name] = [t.to(prm._units) for t in tv[name]]
                for j, name in enumerate(names):
                    # one parameter at a time from the point itself: `_fisher_templates` leaves a parameter at its
                    # last test value while it moves the later ones, which would shift their gradients
                    hypo_maker._set_rescaled_free_params(grid.points[k])
                    resp[k, j] = hypo_maker._fisher_templates([name], {name: tv[name]})["grad"].reshape(-1)
        except BaseException:
            if len(pipes) == 1 and getattr(pipes[0], "_plan", None) is not None:
                plan, pipes[0]._plan = pipes[0]._plan, None
                plan.invalidate()
            raise
        finally:
            hypo_maker.set_free_params(saved)
        center = np.where(ips[None, :] > 0, values - means[None, :], 0.0)
        if form == "loglinear":
            hist = np.asarray(grid.host("hist"), dtype=np.float64).reshape(n, 1, grid.n_bins)
            with np.errstate(invalid="ignore"):
                has = hist > 0.0
            resp = np.where(has, resp / np.where(has, hist, 1.0), 0.0)
        lower = upper = None
        if bounded:
            lower, upper = np.full(values.shape, -np.inf), np.full(values.shape, np.inf)
            for j, name in enumerate(names):
                prm = free[name]
                if prm._range is not None:
                    lower[:, j] = float(prm._range[0].m_as(prm._units)) - values[:, j]
                    upper[:, j] = float(prm._range[1].m_as(prm._units)) - values[:, j]
        return cls(names, K.to_device(resp), ips, center, at_point, values, max_iter, lower, upper, wide, form)


def _takes_bounds(method):
    import inspect

    params = inspect.signature(method).parameters
    return ("lower" in params and "upper" in params) or any(
        p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _takes_wide(method):
    import inspect

    params = inspect.signature(method).parameters
    return "wide" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _takes_form(method):
    import inspect

    params = inspect.signature(method).parameters
    return "form" in params or any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params.values())


def _check_linear(response, what, needs):
    """what reads a kernel whose template is linear in the displacements"""
    if response is not None and getattr(response, "form", "linear") != "linear":
        raise ValueError("%s: %s is not available for a log-linear response (it reads a kernel that is linear in the "
                         "displacements; the fits alone take the form)" % (what, needs))


def _check_narrow(response, what, needs):
    """what goes through a kernel that fits, draws or samples at most 8 parameters"""
    if response is not None and len(response.names) > MAX_PARAMS:
        raise ValueError("%s: %s is limited to %d nuisance parameters; this response has %d (the wide form fits up to "
                         "%d, and fits alone)" % (what, needs, MAX_PARAMS, len(response.names), WIDE_MAX_PARAMS))


def _check_response(response, grid, solver, what, metric=None):
    if metric in _MC_METRICS:
        raise ValueError("%s: response= is not available for '%s' (no profiled form of the MC-uncertainty metrics)"
                         % (what, metric))
    if not hasattr(solver, "profiled_matrix") or not hasattr(solver, "profiled_best"):
        raise ValueError("ensemble: response= needs a solver with profiled_matrix and profiled_best; %s has none"
                         % type(solver).__name__)
    if response.bounded and not (_takes_bounds(solver.profiled_matrix) and _takes_bounds(solver.profiled_best)):
        raise ValueError("ensemble: a response with bounds needs a solver whose profiled_matrix and profiled_best "
                         "take lower= and upper=; those of %s do not" % type(solver).__name__)
    if getattr(response, "wide", False) and not (_takes_wide(solver.profiled_matrix)
                                                 and _takes_wide(solver.profiled_best)):
        raise ValueError("ensemble: a wide response needs a solver whose profiled_matrix and profiled_best take "
                         "wide=; those of %s do not" % type(solver).__name__)
    if getattr(response, "form", "linear") != "linear" and not (_takes_form(solver.profiled_matrix)
                                                                and _takes_form(solver.profiled_best)):
        raise ValueError("ensemble: a log-linear response needs a solver whose profiled_matrix and profiled_best take "
                         "form=; those of %s do not" % type(solver).__name__)
    shape = tuple(response.response.shape)
    if shape[-1] != grid.n_bins or (len(shape) == 3 and shape[0] != len(grid)):
        raise ValueError("%s: the response does not belong to this grid (%s against %d points, %d bins)"
                         % (what, shape, len(grid), grid.n_bins))
    for b in (response.lower, response.upper):
        if b is not None and b.ndim == 2 and b.shape[0] != len(grid):
            raise ValueError("%s: the response's bounds do not belong to this grid (%s against %d points)"
                             % (what, b.shape, len(grid)))


GENERATORS = ("host", "device")
FORMS = ("linear", "loglinear")  # kernels.RESPONSE_FORM: how the templates respond to the displacements
MAX_PARAMS = 8                 # _lib.PROFILE_MAX_PARAMS: the narrow fit, the covariance, the draws and the sampler
WIDE_MAX_PARAMS = 32           # _lib.PROFILE_WIDE_MAX_PARAMS: the wide fit
CHUNK_BYTES = 1 << 30          # pseudo-data of the device generator alive at a time


def _check_generator(generator, solver, method="poisson"):
    if generator not in GENERATORS:
        raise ValueError("ensemble: generator '%s' not among %s" % (generator, list(GENERATORS)))
    if generator == "device" and not hasattr(solver, "draw"):
        raise ValueError("ensemble: generator='device' needs a solver with draw(mu, n_trials, seed, stream, "
                         "first_trial); %s has none" % type(solver).__name__)
    if generator == "device" and method != "poisson" and not hasattr(solver, "fluctuate"):
        raise ValueError("ensemble: generator='device' with method='%s' needs a solver with fluctuate(mu, sigma, "
                         "method, n_trials, seed, stream, first_trial); %s has none" % (method, type(solver).__name__))


def _check_method(method, grid):
    """the method's name as `Map.fluctuate` normalises it (its ValueError for an unknown one)"""
    name = str(method).strip().lower().replace(" ", "")
    if name not in FLUCTUATE_METHODS:
        raise ValueError('Map fluctuation method "%s" not recognized! Valid choices are: %s.'
                         % (name, FLUCTUATE_METHODS))
    if name in ("gauss", "gauss+poisson") and grid.sumw2 is None:
        raise ValueError("ensemble: method='%s' needs the templates' sumw2; this grid has none" % name)
    return name


def _sigma_row(grid, k, method):
    """The standard deviations of template k as `method` reads them: sqrt(sumw2[k]) on the host, after the row rules
    of "scaled_poisson" (map.py:1180-1193): a non-NaN, non-zero bin without an error sets every valid bin's error to
    its Poisson expectation (one warning); a row whose variances equal its means to `ALLCLOSE_KW` has the scale 1
    exactly.  None where the draw is the plain Poisson draw (method "poisson", or that scale of 1)."""
    if method == "poisson":
        return None
    mu = np.asarray(grid.host("hist")[k], dtype=np.float64).ravel()
    with np.errstate(invalid="ignore"):
        sigma = np.zeros(mu.size) if grid.sumw2 is None else np.sqrt(
            np.asarray(grid.host("sumw2")[k], dtype=np.float64).ravel())
        if method == "scaled_poisson":
            ok = ~np.isnan(mu)
            if np.any(sigma[ok & (mu != 0.0)] == 0.0):
                from pisa_amd.utils.log import logging

                logging.warning("Some bins have non-zero counts but no associated error! All errors will be set to "
                                "their Poisson expectation now.")
                sigma = np.where(ok, np.sqrt(mu), sigma)
            if np.allclose(sigma[ok] ** 2, mu[ok], **ALLCLOSE_KW):
                return None
    return sigma


def _host_fluctuate(mu, sigma, method, rs):
    """one `Map.fluctuate(method, random_state=rs)` of the row `mu` with the standard deviations `sigma` (the
    post-rule row of `_sigma_row`; None: the scale 1 of "scaled_poisson"): the same scipy calls on the non-NaN bins
    in the same order (map.py:1171-1251)"""
    from scipy.stats import norm, poisson

    ok = ~np.isnan(mu)
    out = np.full(mu.size, np.nan)
    with np.errstate(invalid="ignore"):
        if method == "scaled_poisson":
            scale = 1.0 if sigma is None else sigma[ok] ** 2 / mu[ok]
            out[ok] = poisson.rvs(mu[ok] / scale, random_state=rs)
            out[ok] *= scale
            out[mu == 0.0] = 0.0
        elif method == "gauss+poisson":
            g = np.clip(norm.rvs(loc=mu[ok], scale=sigma[ok], random_state=rs), 0, None)
            out[ok] = poisson.rvs(g, random_state=rs)
        else:
            out[ok] = norm.rvs(loc=mu[ok], scale=sigma[ok], random_state=rs)
    return out


def _device_draw(solver, grid, k, sigma, method, n_trials, seed, first_trial=0):
    if sigma is None:
        return solver.draw(grid.hist[k], n_trials, seed, stream=k, first_trial=first_trial)
    return solver.fluctuate(grid.hist[k], sigma, method, n_trials, seed, stream=k, first_trial=first_trial)


NUISANCE = ("fixed", "prior", "profiled", "fitted")
_OBSERVED = NUISANCE[2:]       # the modes that read an observed map
TRUTH_ATTEMPTS = 256           # candidates of one trial's truths before the draw gives up (FL_TRUTH_ATTEMPTS)
_PROFILE_HELD = 32             # PISA_HIP_PROFILE_HELD: a coordinate held on a bound; the one flag that is no failure
TRUTH_MIN_MASS = 0.25          # the least share of a prior's mass a parameter's box may hold (kernels.TRUTH_MIN_MASS)


def _check_nuisance(nuisance, response, grid, solver, generator, method, metric, what, observed=None):
    """every mode but "fixed" needs a response of this grid, a metric with a profiled form, a method whose mean may
    move per trial and, for the device generator, a solver that draws such data; "profiled" and "fitted" need the
    observed map, which the other two refuse"""
    if nuisance not in NUISANCE:
        raise ValueError("ensemble: nuisance '%s' not among %s" % (nuisance, list(NUISANCE)))
    if generator not in GENERATORS:
        raise ValueError("ensemble: generator '%s' not among %s" % (generator, list(GENERATORS)))
    if observed is not None and nuisance not in _OBSERVED:
        raise ValueError("%s: observed= belongs to nuisance='profiled' and 'fitted'; nuisance='%s' reads no data"
                         % (what, nuisance))
    if nuisance == "fixed":
        return
    if nuisance in _OBSERVED and observed is None:
        raise ValueError("%s: nuisance='%s' needs observed=, the map the nuisance parameters are fitted to"
                         % (what, nuisance))
    if response is None:
        raise ValueError("%s: nuisance='%s' needs response=, the linear response whose parameters are drawn"
                         % (what, nuisance))
    if metric in _MC_METRICS:
        raise ValueError("%s: nuisance='%s' is not available for '%s' (response= has no form for the "
                         "MC-uncertainty metrics)" % (what, nuisance, metric))
    if nuisance == "fitted":
        _check_linear(response, what, "nuisance='fitted' (the covariance of the observed fit)")
        _check_narrow(response, what, "nuisance='fitted' (the covariance of the observed fit)")
    if generator == "device":
        _check_linear(response, what, "generator='device' with nuisance='%s' (the device draws of the truths)" % nuisance)
        _check_narrow(response, what, "generator='device' with nuisance='%s' (the device draws of the truths)" % nuisance)
    if method == "scaled_poisson":
        raise ValueError("%s: nuisance='%s' has no scaled_poisson draws (the method's row rules compare a row's "
                         "variance with its mean, which moves per trial)" % (what, nuisance))
    if generator == "device" and nuisance != "fitted" and not hasattr(solver, "draw_linear"):
        raise ValueError("ensemble: generator='device' with nuisance='%s' needs a solver with draw_linear(mu, "
                         "response, sigma, method, n_trials, seed, stream, scale, shift, lower, upper, first_trial); "
                         "%s has none" % (nuisance, type(solver).__name__))
    if generator == "device" and nuisance == "fitted" and not hasattr(solver, "draw_linear_mvn"):
        raise ValueError("ensemble: generator='device' with nuisance='fitted' needs a solver with draw_linear_mvn(mu, "
                         "response, sigma, method, n_trials, seed, stream, mean, cov, lower, upper, first_trial); "
                         "%s has none" % type(solver).__name__)
    shape = tuple(response.response.shape)
    if shape[-1] != grid.n_bins or (len(shape) == 3 and shape[0] != len(grid)):
        raise ValueError("%s: the response does not belong to this grid (%s against %d points, %d bins)"
                         % (what, shape, len(grid), grid.n_bins))


def _truth_priors(response, k):
    """what the truths of point k are drawn from -> (R [J, B] as the response holds it, scale, shift, lower, upper
    [J] host arrays): a parameter with a Gaussian prior has scale = its stddev = 1 / inv_prior_sigma and shift =
    -center[k] = prior mean - the parameter's value at the point, so that value + eta ~ N(prior mean, stddev); one
    without keeps scale 0 and shift 0 (it stays at the point's value); the box is the response's at k (None: none)"""
    R = response.response[k] if len(response.response.shape) == 3 else response.response
    ips = np.asarray(response.inv_prior_sigma, dtype=np.float64)
    has = ips > 0
    scale = np.where(has, 1.0 / np.where(has, ips, 1.0), 0.0)
    center = np.zeros(ips.size) if response.center is None else np.asarray(response.center, dtype=np.float64)[k]
    shift = np.where(has, -center, 0.0)
    box = [None if b is None else np.ascontiguousarray(b[k] if b.ndim == 2 else b) for b in (response.lower,
                                                                                             response.upper)]
    return R, scale, shift, box[0], box[1]


def _host_truths(scale, shift, lower, upper, rs):
    """one trial's truths on the stream `rs`: for j ascending, shift_j where scale_j is 0 (nothing is drawn), else
    shift_j + scale_j rs.standard_normal() again and again until the candidate is inside [lower_j, upper_j]"""
    eta = np.array(shift, dtype=np.float64)
    for j in np.nonzero(scale > 0)[0]:
        lo = -np.inf if lower is None else lower[j]
        hi = np.inf if upper is None else upper[j]
        while True:
            x = shift[j] + scale[j] * rs.standard_normal()
            if lo <= x <= hi:
                break
        eta[j] = x
    return eta


def _linear_mean(mu0, R, eta):
    """mu0 + R[0] eta_0 + ... in ascending j, every step rounded (the template the profiled fit works with); a
    negative mean becomes 0, a NaN stays"""
    mu = np.array(mu0, dtype=np.float64)
    for j in range(R.shape[0]):
        mu = mu + R[j] * eta[j]
    with np.errstate(invalid="ignore"):
        return np.where(mu < 0.0, 0.0, mu)


def _loglinear_mean(mu0, rho, eta):
    """mu0 exp(rho[0] eta_0 + ...) with the exponent formed from 0 in ascending j, every step rounded (the template the
    log-linear fit works with); a bin with mu0 == 0 or every rho == 0 keeps mu0 exactly; a negative mean becomes 0, a
    NaN stays"""
    mu0 = np.array(mu0, dtype=np.float64)
    s = np.zeros(mu0.shape)
    for j in range(rho.shape[0]):
        s = s + rho[j] * eta[j]
    with np.errstate(invalid="ignore", over="ignore"):
        responds = (mu0 != 0.0) & np.any(rho != 0.0, axis=0)
        mu = np.where(responds, mu0 * np.exp(np.where(responds, s, 0.0)), mu0)
        return np.where(mu < 0.0, 0.0, mu)


def _mean_of(response):
    """the host generator's mean of a trial by the response's form"""
    return _loglinear_mean if getattr(response, "form", "linear") == "loglinear" else _linear_mean


def _prior_data(grid, k, n_trials, seed_or_rs, generator, solver, method, response, first_trial=0):
    """(data [n_trials, B], eta_true [n_trials, J]) of `nuisance="prior"` at point k: module docstring"""
    R, scale, shift, lower, upper = _truth_priors(response, k)
    sigma = _sigma_row(grid, k, method)
    if generator != "host":
        out = solver.draw_linear(grid.hist[k], R, sigma, method, n_trials, seed_or_rs, stream=k, scale=scale,
                                 shift=shift, lower=lower, upper=upper, first_trial=first_trial)
        return out["data"], out["eta"]
    from scipy.stats import norm

    for j in np.nonzero(scale > 0)[0]:                 # the device generator's rule, so that both refuse alike
        lo, hi = (-np.inf if lower is None else lower[j]), (np.inf if upper is None else upper[j])
        mass = norm.cdf((hi - shift[j]) / scale[j]) - norm.cdf((lo - shift[j]) / scale[j])
        if mass < TRUTH_MIN_MASS:
            raise ValueError("pseudo_data: the box [%g, %g] of '%s' holds %.3g of the mass of its prior; at least %g "
                             "is needed" % (lo, hi, response.names[j], mass, TRUTH_MIN_MASS))
    rs = seed_or_rs
    mu0 = np.asarray(grid.host("hist")[k], dtype=np.float64).ravel()
    R = _host(R).astype(np.float64)
    data, truth = np.empty((max(n_trials, 0), mu0.size)), np.empty((max(n_trials, 0), scale.size))
    mean = _mean_of(response)
    for t in range(data.shape[0]):
        truth[t] = _host_truths(scale, shift, lower, upper, rs)
        data[t] = _host_row(mean(mu0, R, truth[t]), sigma, method, rs)
    return data, truth


def _host_row(mu, sigma, method, rs):
    """one trial's data by `method` from its own mean `mu` on the stream `rs`: the method's own scipy calls"""
    if method != "poisson":
        return _host_fluctuate(mu, sigma, method, rs)
    from scipy.stats import poisson

    ok = ~np.isnan(mu)
    row = np.full(mu.size, np.nan)
    if ok.any():
        row[ok] = poisson.rvs(mu[ok], random_state=rs)
    return row


def _truth_factor(cov):
    """`fl_truth_factor` of csrc/fluctuate_device.hpp in numpy: L [J, J] lower triangular with cov = L L^T over the live
    coordinates (cov[j, j] != 0), rows and columns of the dead ones 0; None where the factor is refused (an entry that
    is not finite, a dead coordinate with a non-zero entry in its row or column, a pivot <= 0 or NaN)"""
    cov = np.asarray(cov, dtype=np.float64)
    J = cov.shape[0]
    L = np.zeros((J, J))
    if cov.shape != (J, J) or not np.isfinite(cov).all():
        return None
    dead = np.diagonal(cov) == 0.0
    if np.any(cov[dead, :] != 0.0) or np.any(cov[:, dead] != 0.0):
        return None
    with np.errstate(all="ignore"):
        for i in np.nonzero(~dead)[0]:
            for j in np.nonzero(~dead[:i + 1])[0]:
                s = cov[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if j < i:
                    s = s / L[j, j]
                else:
                    if not s > 0.0:
                        return None
                    s = np.sqrt(s)
                if not np.isfinite(s):
                    return None
                L[i, j] = s
    return L


def _host_truths_mvn(mean, L, lower, upper, rs):
    """one trial's truths of `nuisance="fitted"` on the stream `rs`: per attempt one rs.standard_normal() per live k
    (L[k, k] != 0) in ascending k, x_j = mean_j + L[j, 0] z_0 + ... + L[j, j] z_j over the live k, and the first
    candidate with every coordinate inside [lower_j, upper_j]; ValueError after TRUTH_ATTEMPTS refused ones (where the
    device generator reports its truths exhausted)"""
    J = mean.size
    live = np.nonzero(np.diagonal(L) != 0.0)[0]
    lo = np.full(J, -np.inf) if lower is None else lower
    hi = np.full(J, np.inf) if upper is None else upper
    for _ in range(TRUTH_ATTEMPTS):
        z = np.zeros(J)
        for k in live:
            z[k] = rs.standard_normal()
        x = np.array(mean, dtype=np.float64)
        for j in live:
            for k in live[live <= j]:
                x[j] = x[j] + L[j, k] * z[k]
        if np.all((lo <= x) & (x <= hi)):
            return x
    raise ValueError("pseudo_data: a trial found no candidate inside the box")


def fit_observed(observed, grid, metric, response, solver=None, covariance=False):
    """The conditional fit of ONE observed map at every point of the grid: `observed` a Map, a MapSet of one map or
    [B] values -> dict of host arrays, eta [K, J] the displacements of the response's parameters that fit the map best
    given point k and status [K] the fit's flags (one `solver.profiled_matrix` call with T = 1), value [K] the
    profiled metric there without the points' penalties; with covariance=True also cov [K, J, J], sigma [K, J] and
    hesse_status [K] (one `solver.hesse` call on the K (map, point) pairs: `delta_metric(..., covariance=True)`
    describes them).  What `nuisance="profiled"` and "fitted" generate their pseudo-data at."""
    _check_metric(metric)
    solver = DeviceSolver() if solver is None else solver
    if response is None:
        raise ValueError("fit_observed: needs response=, the linear response whose parameters are fitted")
    _check_response(response, grid, solver, "fit_observed", metric)
    if covariance:
        _check_linear(response, "fit_observed", "covariance=True")
        _check_narrow(response, "fit_observed", "covariance=True")
        _check_hesse(solver)
    rows = _data_rows(observed)
    if int(rows.shape[0]) != 1 or int(rows.shape[1]) != grid.n_bins:
        raise ValueError("fit_observed: one observed map of %d bins, got %s" % (grid.n_bins, tuple(rows.shape)))
    args = (grid.sigma2_for(metric), response.inv_prior_sigma, response.center)
    out = solver.profiled_matrix(metric, rows, grid.hist, response.response, *args, response.max_iter,
                                 **response.fit_keywords())
    fit = dict(eta=_host(out["eta"])[0], status=_host(out["status"])[0], value=_host(out["value"])[0])
    if covariance:
        n_k = len(grid)
        rep = rows.expand(n_k, -1).contiguous() if hasattr(rows, "expand") else np.repeat(rows, n_k, axis=0)
        h = solver.hesse(metric, rep, grid.hist, response.response, out["eta"][0], np.arange(n_k, dtype=np.int32),
                         *args, **response.bounds())
        fit.update(cov=_host(h["cov"]), sigma=_host(h["sigma"]), hesse_status=_host(h["status"]))
    return fit


def _observed_truths(observed, grid, metric, response, solver, nuisance, points, what):
    """the fit of the observed map the pseudo-data of `points` are generated at, checked -> (eta [K, J], cov [K, J, J]
    or None): a point whose fit carries a flag, has no covariance, whose covariance has no factor or whose box holds
    too little of a coordinate's marginal is refused"""
    from scipy.stats import norm

    for k in points:
        if not 0 <= k < len(grid):
            raise ValueError("%s: point %s outside the grid's %d points" % (what, k, len(grid)))
    fit = fit_observed(observed, grid, metric, response, solver, covariance=nuisance == "fitted")
    bad = [k for k in points if int(fit["status"][k]) & ~_PROFILE_HELD]
    if bad:
        raise ValueError("%s: the fit of the observed map carries a status flag at the points %s (status %s)"
                         % (what, bad, [int(fit["status"][k]) for k in bad]))
    if nuisance != "fitted":
        return fit["eta"], None
    bad = [k for k in points if np.isnan(fit["cov"][k]).any()]
    if bad:
        raise ValueError("%s: the fit of the observed map has no covariance at the points %s (hesse_status %s)"
                         % (what, bad, [int(fit["hesse_status"][k]) for k in bad]))
    bad = [k for k in points if _truth_factor(fit["cov"][k]) is None]
    if bad:
        raise ValueError("%s: the covariance of the fit of the observed map has no Cholesky factor at the points %s"
                         % (what, bad))
    for k in points:
        _, _, _, lower, upper = _truth_priors(response, k)
        mean, var = fit["eta"][k], np.diagonal(fit["cov"][k])
        for j in np.nonzero(var > 0)[0]:
            lo, hi = (-np.inf if lower is None else lower[j]), (np.inf if upper is None else upper[j])
            sd = math.sqrt(var[j])
            mass = norm.cdf((hi - mean[j]) / sd) - norm.cdf((lo - mean[j]) / sd)
            if mass < TRUTH_MIN_MASS:
                raise ValueError("%s: at point %d the box [%g, %g] of '%s' holds %.3g of the mass of its fitted N(%g, "
                                 "%g); at least %g is needed" % (what, k, lo, hi, response.names[j], mass, mean[j], sd,
                                                                 TRUTH_MIN_MASS))
    return fit["eta"], fit["cov"]


def _observed_data(grid, k, n_trials, seed_or_rs, generator, solver, method, response, eta, cov, first_trial=0):
    """(data [n_trials, B], eta_true [n_trials, J]) of `nuisance="profiled"` (cov None: every trial's truths are `eta`
    [J]) and "fitted" (truths from N(eta, cov) inside the response's box) at point k: module docstring"""
    R, _, _, lower, upper = _truth_priors(response, k)
    sigma = _sigma_row(grid, k, method)
    eta = np.ascontiguousarray(eta, dtype=np.float64)
    if generator != "host":
        if cov is None:
            out = solver.draw_linear(grid.hist[k], R, sigma, method, n_trials, seed_or_rs, stream=k,
                                     scale=np.zeros(eta.size), shift=eta, lower=lower, upper=upper,
                                     first_trial=first_trial)
        else:
            out = solver.draw_linear_mvn(grid.hist[k], R, sigma, method, n_trials, seed_or_rs, stream=k, mean=eta,
                                         cov=np.ascontiguousarray(cov, dtype=np.float64), lower=lower, upper=upper,
                                         first_trial=first_trial)
        return out["data"], out["eta"]
    rs = seed_or_rs
    L = None if cov is None else _truth_factor(cov)
    mu0 = np.asarray(grid.host("hist")[k], dtype=np.float64).ravel()
    R = _host(R).astype(np.float64)
    data, truth = np.empty((max(n_trials, 0), mu0.size)), np.empty((max(n_trials, 0), eta.size))
    mean = _mean_of(response)
    for t in range(data.shape[0]):
        truth[t] = eta if L is None else _host_truths_mvn(eta, L, lower, upper, rs)
        data[t] = _host_row(mean(mu0, R, truth[t]), sigma, method, rs)
    return data, truth


def _check_truths(response, grid, solver, generator, method, metric, nuisance, observed, what):
    """`truths=` needs a response of this grid, a metric with a profiled form, a method whose mean may move per trial
    and, for the device generator, a solver with `draw_linear_at`; it generates at GIVEN nuisance values, so the modes
    that choose them (`nuisance=`, `observed=`) are refused beside it"""
    if generator not in GENERATORS:
        raise ValueError("ensemble: generator '%s' not among %s" % (generator, list(GENERATORS)))
    if nuisance != "fixed" or observed is not None:
        raise ValueError("%s: truths= gives every trial's nuisance values itself; leave nuisance at 'fixed' and "
                         "observed= at None" % what)
    if response is None:
        raise ValueError("%s: truths= needs response=, the linear response the truths displace" % what)
    if metric in _MC_METRICS:
        raise ValueError("%s: truths= is not available for '%s' (response= has no form for the MC-uncertainty "
                         "metrics)" % (what, metric))
    if method == "scaled_poisson":
        raise ValueError("%s: truths= has no scaled_poisson draws (the method's row rules compare a row's variance "
                         "with its mean, which moves per trial)" % what)
    if generator == "device":
        _check_linear(response, what, "generator='device' with truths= (the device draws at given truths)")
        _check_narrow(response, what, "generator='device' with truths= (the device draws at given truths)")
    if generator == "device" and not hasattr(solver, "draw_linear_at"):
        raise ValueError("ensemble: generator='device' with truths= needs a solver with draw_linear_at(mu, response, "
                         "sigma, method, eta, seed, stream, first_trial); %s has none" % type(solver).__name__)
    shape = tuple(response.response.shape)
    if shape[-1] != grid.n_bins or (len(shape) == 3 and shape[0] != len(grid)):
        raise ValueError("%s: the response does not belong to this grid (%s against %d points, %d bins)"
                         % (what, shape, len(grid), grid.n_bins))


def _truth_rows(truths, k, n_j, first, n, what):
    """rows [first, first + n) of the truths of point k: `truths` a `PosteriorSample`, a mapping from point index to
    [n, J], or (`pseudo_data`) one [n, J] array"""
    sample = truths if isinstance(truths, PosteriorSample) else None
    if sample is not None:
        if k not in sample.points:
            raise ValueError("%s: the posterior sample holds the points %s, not point %d" % (what, sample.points, k))
        rows = sample.eta[sample.points.index(k)]
    elif hasattr(truths, "keys"):
        if k not in truths:
            raise ValueError("%s: truths= holds no rows for point %d" % (what, k))
        rows = truths[k]
    else:
        rows = truths
    rows = np.asarray(_host(rows), dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != n_j:
        raise ValueError("%s: the truths of point %d are [n, %d] displacements, got %s" % (what, k, n_j, rows.shape))
    if first + n > rows.shape[0]:
        missing = first + n - rows.shape[0]
        if sample is not None:
            steps = -(-missing // sample.n_walkers) * sample.thin
            raise ValueError("%s: %d trials at point %d and %d rows of truths: the sample needs %d steps more (%d rows "
                             "at %d walkers, thin %d)" % (what, first + n, k, rows.shape[0], steps, missing,
                                                          sample.n_walkers, sample.thin))
        raise ValueError("%s: %d trials at point %d and %d rows of truths: %d rows more are needed"
                         % (what, first + n, k, rows.shape[0], missing))
    rows = np.ascontiguousarray(rows[first:first + n])
    if np.isnan(rows).any():
        raise ValueError("%s: the truths of point %d hold a NaN (a posterior sample whose chains did not run?)"
                         % (what, k))
    return rows


def _truths_data(grid, k, rows, seed_or_rs, generator, solver, method, response, first_trial=0):
    """data [n, B] at the truths `rows` [n, J] of the trials first_trial ... at point k: module docstring"""
    R = _truth_priors(response, k)[0]
    sigma = _sigma_row(grid, k, method)
    if generator != "host":
        return solver.draw_linear_at(grid.hist[k], R, sigma, method, rows, seed_or_rs, stream=k,
                                     first_trial=first_trial)["data"]
    rs = seed_or_rs
    mu0 = np.asarray(grid.host("hist")[k], dtype=np.float64).ravel()
    R = _host(R).astype(np.float64)
    data = np.empty((rows.shape[0], mu0.size))
    mean = _mean_of(response)
    for t in range(data.shape[0]):
        data[t] = _host_row(mean(mu0, R, rows[t]), sigma, method, rs)
    return data


def pseudo_data(grid, k, n_trials, random_state=None, generator="host", solver=None, method="poisson", response=None,
                nuisance="fixed", return_truth=False, observed=None, truths=None):
    """[n_trials, B] pseudo-data of template k by `method` (one of `FLUCTUATE_METHODS`; every method but "poisson"
    reads sigma = sqrt(grid.sumw2[k]), and "scaled_poisson" applies the reference's row rules to it first: module
    docstring).  With another method than "poisson" the host generator is the loop of `Map.fluctuate(method,
    random_state=rs)` over the trials on ONE `RandomState`, and the device generator is `solver.fluctuate(grid.hist[k],
    sigma, method, n_trials, seed, stream=k)`.  For "poisson":
    generator="host": trial t is exactly the t-th `Map.fluctuate("poisson", random_state=rs)` of that template from
    ONE `RandomState` rs (one `scipy.stats.poisson.rvs` call on the tiled expectation consumes the stream in the same
    order; NaN bins stay NaN and draw nothing).  Drawn on the host, a host array: the reference's stream.
    generator="device": what `solver.draw(grid.hist[k], n_trials, seed, stream=k)` returns (from `DeviceSolver`, the
    default, a device tensor: `kernels.poisson_fluctuate`), seed = `random_state` or one draw from it if it is a
    RandomState, as in `feldman_cousins`.  A counter-based generator of its own definition, NOT the reference's
    stream; NaN bins stay NaN and a zero bin stays 0 here as well.
    nuisance="prior" (with `response`, a `NuisanceResponse` of this grid): the parameters of the response do not sit
    at the point's values when the data are made; every trial draws their truths eta from their priors -- N(prior
    mean, stddev) for a parameter with a Gaussian prior, truncated to the response's box if it has one; a parameter
    without a prior stays at the point's value -- and its data by `method` ("scaled_poisson" is refused) from the
    linearised template hist[k] + sum_j response[k, j] eta_j, a negative mean taken as 0 ("pseudo-data
    with drawn nuisance truths").  generator="device": `solver.draw_linear` (`kernels.fluctuate_linear`);
    generator="host": per trial, for j ascending, shift_j + scale_j rs.standard_normal() until the candidate is inside
    the box, then the method's own scipy calls on that trial's mean, all on the one RandomState.  nuisance="fixed"
    (the default) is the call without the argument.
    nuisance="profiled" and "fitted" (with `response` and `observed`, the data map: a Map, a MapSet of one map or [B]
    values) generate at the nuisance values fitted to the OBSERVED map given point k (`fit_observed`; DESIGN.md §4,
    "pseudo-data at nuisances fitted to the observed data").  "profiled", the profile construction: every trial's
    truths are the fitted displacements eta_obs[k] -- the generator of "prior" with every scale 0 and the shift
    eta_obs[k], bit for bit, on both generators.  "fitted": every trial draws its truths from the fit's Gaussian
    N(eta_obs[k], cov_obs[k]) truncated to the response's box by rejection of the whole vector, a coordinate the fit
    holds on a bound staying there; generator="device": `solver.draw_linear_mvn` (`kernels.fluctuate_linear_mvn`);
    generator="host": per attempt one rs.standard_normal() per live coordinate k in ascending k, x_j = eta_obs[k, j] +
    L[j, 0] z_0 + ... + L[j, j] z_j with the Cholesky factor L of cov_obs[k], until every coordinate is inside the
    box, then the method's own scipy calls.  return_truth=True returns (data, eta_true [n_trials, J]: the
    displacements from the point's values the fit's eta estimates; None for "fixed").
    truths= (with `response`; nuisance left at "fixed", no `observed`): a `PosteriorSample` of `posterior_sample` that
    holds point k, or [n, J] displacements of the caller's own.  Trial number n is generated at row n of the truths:
    by `method` from hist[k] + sum_j response[k, j] eta_n[j], a negative mean taken as 0.  generator="device":
    `solver.draw_linear_at` (`kernels.fluctuate_linear_at`), stream k; generator="host": `_linear_mean` and the
    method's own scipy calls on the one RandomState.  Fewer rows than trials, a NaN row, "scaled_poisson" and the
    MC-uncertainty metrics are refused; return_truth=True returns the rows used.  With every row equal to
    eta_obs[k] the data are those of nuisance="profiled"."""
    method = _check_method(method, grid)
    if truths is not None:
        solver_ = (DeviceSolver() if solver is None else solver) if generator != "host" else solver
        _check_truths(response, grid, solver_, generator, method, grid.metric, nuisance, observed, "pseudo_data")
        if not 0 <= int(k) < len(grid):
            raise ValueError("pseudo_data: point %s outside the grid's %d points" % (k, len(grid)))
        rows = _truth_rows(truths, int(k), len(response.names), 0, int(n_trials), "pseudo_data")
        if generator == "host":
            source = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(
                random_state)
        else:
            source = _base_seed(random_state)
        data = _truths_data(grid, int(k), rows, source, generator, solver_, method, response)
        return (data, rows) if return_truth else data
    if nuisance != "fixed":
        solver_ = (DeviceSolver() if solver is None else solver) if generator != "host" else solver
        _check_nuisance(nuisance, response, grid, solver_, generator, method, grid.metric, "pseudo_data", observed)
    elif observed is not None:
        _check_nuisance(nuisance, response, grid, solver, generator, method, grid.metric, "pseudo_data", observed)
    if nuisance != "fixed":
        if not 0 <= int(k) < len(grid):
            raise ValueError("pseudo_data: point %s outside the grid's %d points" % (k, len(grid)))
        if nuisance in _OBSERVED:
            eta, cov = _observed_truths(observed, grid, grid.metric, response, solver_, nuisance, [int(k)],
                                        "pseudo_data")
        if generator == "host":
            source = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(
                random_state)
        else:
            source = _base_seed(random_state)
        if nuisance == "prior":
            data, truth = _prior_data(grid, int(k), int(n_trials), source, generator, solver_, method, response)
        else:
            data, truth = _observed_data(grid, int(k), int(n_trials), source, generator, solver_, method, response,
                                         eta[int(k)], None if cov is None else cov[int(k)])
        return (data, truth) if return_truth else data
    if return_truth:
        return pseudo_data(grid, k, n_trials, random_state, generator, solver, method), None
    if generator != "host":
        solver = DeviceSolver() if solver is None else solver
        _check_generator(generator, solver, method)
        return _device_draw(solver, grid, int(k), _sigma_row(grid, k, method), method, int(n_trials),
                            _base_seed(random_state))
    from scipy.stats import poisson

    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    mu = np.asarray(grid.host("hist")[k], dtype=np.float64).ravel()
    if method != "poisson":
        sigma = _sigma_row(grid, k, method)
        out = np.empty((max(int(n_trials), 0), mu.size))
        for t in range(out.shape[0]):
            out[t] = _host_fluctuate(mu, sigma, method, rs)
        return out
    ok = ~np.isnan(mu)
    out = np.full((int(n_trials), mu.size), np.nan)
    if n_trials > 0 and ok.any():
        out[:, ok] = poisson.rvs(np.tile(mu[ok], (int(n_trials), 1)), random_state=rs)
    return out


def _data_rows(data):
    """a Map, a MapSet of one map, or an array -> [T, B] (host array or device tensor)"""
    if hasattr(data, "maps"):
        if len(data.maps) != 1:
            raise ValueError("ensemble: a data MapSet must hold exactly one map")
        data = data.maps[0]
    if hasattr(data, "nominal_values"):
        return np.asarray(data.nominal_values, dtype=np.float64).reshape(1, -1)
    if hasattr(data, "dim"):                       # a device tensor
        return data if data.dim() == 2 else data.reshape(1, -1)
    a = np.asarray(data, dtype=np.float64)
    return a if a.ndim == 2 else a.reshape(1, -1)


def metric_matrix(data, grid, metric, with_penalty=True, solver=None, response=None):
    """[T, K]: `Map.metric_total(template k, metric)` of every data row (+ the priors penalty of point k).  A device
    tensor where the solver returns one, else a host array.  With `response` (a `NuisanceResponse`) every entry is
    profiled over the response's parameters: the metric at the fitted displacements with their prior terms, + the
    penalty of the point's other parameters."""
    _check_metric(metric)
    solver = DeviceSolver() if solver is None else solver
    if response is None:
        m = solver.matrix(metric, _data_rows(data), grid.hist, grid.sigma2_for(metric))
        penalty = grid.penalty if np.any(grid.penalty != 0.0) else None
    else:
        _check_response(response, grid, solver, "metric_matrix", metric)
        m = solver.profiled_matrix(metric, _data_rows(data), grid.hist, response.response, grid.sigma2_for(metric),
                                   response.inv_prior_sigma, response.center, response.max_iter,
                                   **response.fit_keywords())["value"]
        penalty = response.offset(grid)
    if with_penalty and penalty is not None:
        if hasattr(m, "cpu"):
            from pisa_amd import kernels as K

            m = m + K.to_device(penalty)[None, :]
        else:
            m = m + penalty[None, :]
    return m


def delta_metric(data, grid, metric, k0, solver=None, response=None, return_info=False, covariance=False):
    """[T] host array: per data row the distance of point k0 from the best point of the grid, penalties included --
    best - at for the llh metrics, at - best for the chi2 metrics (>= 0; no factor of 2 is applied).  The T x K
    matrix is never written (`pisa_hip_metric_matrix_best`).  With `response` both values are profiled over the
    response's parameters (`pisa_hip_profiled_metric_matrix_best`); `return_info=True` then returns (delta, info) with
    info = dict(flagged: the number of trials whose pair at the best point or at k0 carries a status flag, status
    [T], arg [T], eta_best and eta_at [T, J]: the fitted displacements at both points).  `covariance=True` (with
    `return_info`; needs a solver with `hesse`) adds cov_best and cov_at [T, J, J], the covariance of the displacements
    at both points -- the inverse Hessian of -ln L there with the prior terms, a coordinate the fit holds on a bound
    having zero rows and columns ("Profiled trial ensembles: covariance and pulls") --, sigma_best and
    sigma_at [T, J] = sqrt of their diagonals, and hesse_status [T]: the flags of both calls ORed."""
    _check_metric(metric)
    if covariance and not (return_info and response is not None):
        raise ValueError("delta_metric: covariance=True belongs to response= and return_info=True")
    if not 0 <= int(k0) < len(grid):
        raise ValueError("delta_metric: k0 = %s outside the grid's %d points" % (k0, len(grid)))
    solver = DeviceSolver() if solver is None else solver
    if response is None:
        if return_info:
            raise ValueError("delta_metric: return_info belongs to response=")
        offset = grid.penalty if np.any(grid.penalty != 0.0) else None
        best, _, at = solver.best(metric, _data_rows(data), grid.hist, grid.sigma2_for(metric), offset, int(k0))
        best, at = _host(best), _host(at)
        return best - at if metric in _MAXIMISED else at - best
    _check_response(response, grid, solver, "delta_metric", metric)
    if covariance:
        _check_linear(response, "delta_metric", "covariance=True")
        _check_narrow(response, "delta_metric", "covariance=True")
        _check_hesse(solver)
    out = solver.profiled_best(metric, _data_rows(data), grid.hist, response.response, grid.sigma2_for(metric),
                               response.inv_prior_sigma, response.center, response.offset(grid), int(k0),
                               response.max_iter, **response.fit_keywords())
    best, at = _host(out["best"]), _host(out["at"])
    delta = best - at if metric in _MAXIMISED else at - best
    if not return_info:
        return delta
    status = _host(out["status"])
    info = dict(flagged=int(np.count_nonzero(status)), status=status, arg=_host(out["arg"]),
                eta_best=_host(out["eta_best"]), eta_at=_host(out["eta_at"]))
    if covariance:
        hesse_status = 0
        for which, k in (("best", out["arg"]), ("at", int(k0))):
            h = solver.hesse(metric, _data_rows(data), grid.hist, response.response, out["eta_" + which], k,
                             grid.sigma2_for(metric), response.inv_prior_sigma, response.center, **response.bounds())
            info["cov_" + which], info["sigma_" + which] = _host(h["cov"]), _host(h["sigma"])
            hesse_status = hesse_status | _host(h["status"])
        info["hesse_status"] = hesse_status
    return delta, info


def _check_hesse(solver):
    if not hasattr(solver, "hesse"):
        raise ValueError("ensemble: covariances and pulls need a solver with hesse(kind, data, expected, response, eta, "
                         "k, sigma2, inv_prior_sigma, center, lower=, upper=); %s has none" % type(solver).__name__)


def pulls(data, grid, metric, k0, response, truth, solver=None):
    """[T, J] host array: the pulls (eta_at - truth) / sigma_at of the displacements fitted at point k0 to every data
    row -- `truth` [T, J] the displacements the rows were drawn at (`pseudo_data(..., nuisance="prior",
    return_truth=True)`; zeros for nuisance="fixed"), sigma_at from `delta_metric(..., covariance=True)`.  For an
    ensemble drawn and fitted with the same linear response they are standard normal where the priors are Gaussian
    and the counts large: the closure check of a profiled ensemble.  NaN where sigma is 0 (a coordinate held on a
    bound) or NaN (a flagged fit)."""
    solver = DeviceSolver() if solver is None else solver
    _check_linear(response, "pulls", "the covariance of the fit")
    _check_narrow(response, "pulls", "the covariance of the fit")
    _check_hesse(solver)
    rows = _data_rows(data)
    truth = _host(truth)
    n_j = len(response.names)
    if truth.shape != (int(rows.shape[0]), n_j):
        raise ValueError("pulls: truth holds one displacement per data row and parameter [%d, %d], got %s"
                         % (int(rows.shape[0]), n_j, truth.shape))
    _, info = delta_metric(rows, grid, metric, k0, solver, response, return_info=True, covariance=True)
    sigma = info["sigma_at"]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sigma > 0, (info["eta_at"] - truth) / sigma, np.nan)


def critical_values(delta, cl):
    """per confidence level the value at index ceil(cl * T) - 1 of the ascending sort of `delta` [T]: the smallest
    observed value that at least a fraction cl of the trials do not exceed; no interpolation"""
    d = np.sort(np.asarray(delta, dtype=np.float64).ravel())
    if d.size == 0:
        raise ValueError("critical_values: no trials")
    out = []
    for c in np.atleast_1d(cl):
        if not 0.0 < c <= 1.0:
            raise ValueError("critical_values: confidence level %s outside (0, 1]" % c)
        out.append(d[min(max(int(math.ceil(c * d.size)) - 1, 0), d.size - 1)])
    return np.array(out)


def _base_seed(random_state):
    if random_state is None:
        return int(np.random.SeedSequence().generate_state(1)[0])
    if isinstance(random_state, np.random.RandomState):
        return int(random_state.randint(0, 2 ** 31 - 1))
    seed = int(random_state)
    if not 0 <= seed < 2 ** 32:
        raise ValueError("feldman_cousins: the seed %d is outside [0, 2^32)" % seed)
    return seed


def feldman_cousins(grid, metric, n_trials, cl=(0.6827, 0.90), random_state=None, true_points=None, solver=None,
                    generator="host", chunk_bytes=CHUNK_BYTES, response=None, method="poisson",
                    nuisance="fixed", observed=None, truths=None):
    """Critical values of the Feldman-Cousins ordering on the grid: for every true point k0 (default: all), n_trials
    pseudo-data maps of template k0, their `delta_metric` at k0 and `critical_values` -> crit [len(true_points),
    len(cl)].  seed: `random_state`, or one draw from it if it is a RandomState.
    generator="host": every true point draws from its own RandomState([seed, k0]) (`pseudo_data`) and the data are
    uploaded; generator="device": every true point is the stream k0 of the solver's `draw` under the one seed, the
    draws go from `draw` into `delta_metric` where they are, in chunks of whole trials of at most `chunk_bytes` of
    pseudo-data (trial numbers carried through `first_trial`: the result does not depend on the chunks).  Either way
    a subset of true points reproduces the full run's rows.  `method`: how the pseudo-data fluctuate, as in
    `pseudo_data` (the device generator then draws through the solver's `fluctuate`).  Without `response` nuisance parameters are profiled only
    as far as they are dimensions of the grid (module docstring).  With `response` (a `NuisanceResponse`) every
    distance is profiled over the response's parameters and the return value is (crit, info), info = dict(flagged
    [len(true_points)]: per true point the number of trials whose pair at the best point or at the true point carries
    a status flag of the fit).  nuisance="prior" (needs `response`): the pseudo-data of every true point are those of
    `pseudo_data(..., response=response, nuisance="prior")` -- the response's parameters drawn from their priors trial
    by trial --, the device generator drawing them in the same chunks through the solver's `draw_linear`.
    nuisance="profiled" and "fitted" (need `response` and `observed`, the data map): the observed map is fitted once
    at all points (`fit_observed`) and the pseudo-data of true point k0 are those of `pseudo_data(..., nuisance=...,
    observed=observed)` -- generated at the displacements fitted to the observed map given k0 (the profile
    construction), or at truths drawn from that fit's Gaussian --, in the chunks, seeds and streams of "prior"; info
    gains eta_observed [len(true_points), J] and, for "fitted", cov_observed [len(true_points), J, J].
    truths= (needs `response`; nuisance left at "fixed", no `observed`): a `PosteriorSample` or a mapping from point
    index to [n, J] displacements; trial number n of true point k0 is generated at row n of k0's truths
    (`pseudo_data(..., truths=)`), the distances are profiled over the response as for "prior", and the device
    generator draws in the same chunks through the solver's `draw_linear_at`: the result does not depend on the
    chunks.  info gains truths_used [len(true_points)], the rows read per true point."""
    _check_metric(metric)
    if n_trials < 1:
        raise ValueError("feldman_cousins: n_trials >= 1")
    solver = DeviceSolver() if solver is None else solver
    method = _check_method(method, grid)
    if truths is not None:
        _check_truths(response, grid, solver, generator, method, metric, nuisance, observed, "feldman_cousins")
    else:
        _check_nuisance(nuisance, response, grid, solver, generator, method, metric, "feldman_cousins", observed)
    if nuisance == "fixed" and truths is None:
        _check_generator(generator, solver, method)
    if response is not None:
        _check_response(response, grid, solver, "feldman_cousins", metric)
    seed = _base_seed(random_state)
    flagged = []

    def distances(data, k0):
        if response is None:
            return delta_metric(data, grid, metric, k0, solver)
        delta, info = delta_metric(data, grid, metric, k0, solver, response, return_info=True)
        flagged[-1] += info["flagged"]
        return delta

    points = range(len(grid)) if true_points is None else [int(k) for k in true_points]
    for k0 in points:
        if not 0 <= k0 < len(grid):
            raise ValueError("feldman_cousins: true point %d outside the grid's %d points" % (k0, len(grid)))
    cl = np.atleast_1d(np.asarray(cl, dtype=np.float64))
    crit = np.empty((len(points), cl.size))
    if nuisance in _OBSERVED:
        eta_obs, cov_obs = _observed_truths(observed, grid, metric, response, solver, nuisance, list(points),
                                            "feldman_cousins")
    rows = max(1, int(chunk_bytes) // (8 * grid.n_bins))
    if truths is not None:
        for k0 in points:      # (every point's rows are there before the first draw)
            _truth_rows(truths, k0, len(response.names), 0, n_trials, "feldman_cousins")
    for i, k0 in enumerate(points):
        flagged.append(0)
        if truths is not None:
            parts = []
            source = np.random.RandomState([seed, k0]) if generator == "host" else seed
            for first in range(0, n_trials, n_trials if generator == "host" else rows):
                n = n_trials if generator == "host" else min(rows, n_trials - first)
                at = _truth_rows(truths, k0, len(response.names), first, n, "feldman_cousins")
                parts.append(distances(_truths_data(grid, k0, at, source, generator, solver, method, response, first),
                                       k0))
            delta = np.concatenate(parts)
        elif nuisance != "fixed":
            parts = []
            source = np.random.RandomState([seed, k0]) if generator == "host" else seed
            for first in range(0, n_trials, n_trials if generator == "host" else rows):
                n = n_trials if generator == "host" else min(rows, n_trials - first)
                if nuisance == "prior":
                    data = _prior_data(grid, k0, n, source, generator, solver, method, response, first)[0]
                else:
                    data = _observed_data(grid, k0, n, source, generator, solver, method, response, eta_obs[k0],
                                          None if cov_obs is None else cov_obs[k0], first)[0]
                parts.append(distances(data, k0))
            delta = np.concatenate(parts)
        elif generator == "host":
            data = pseudo_data(grid, k0, n_trials, np.random.RandomState([seed, k0]), method=method)
            delta = distances(data, k0)
        else:
            sigma = _sigma_row(grid, k0, method)
            parts = []
            for first in range(0, n_trials, rows):
                data = _device_draw(solver, grid, k0, sigma, method, min(rows, n_trials - first), seed, first)
                parts.append(distances(data, k0))
            delta = np.concatenate(parts)
        crit[i] = critical_values(delta, cl)
    if response is None:
        return crit
    info = dict(flagged=np.array(flagged, dtype=np.int64))
    if truths is not None:
        info["truths_used"] = np.full(len(points), n_trials, dtype=np.int64)
    if nuisance in _OBSERVED:
        info["eta_observed"] = eta_obs[list(points)]
        if cov_obs is not None:
            info["cov_observed"] = cov_obs[list(points)]
    return crit, info


def accepted(data_map, grid, metric, crit, solver=None, response=None):
    """boolean [K]: point k is inside the confidence region of the observed map -- its `delta_metric` at k (one row
    of the matrix, penalties included, against the row's best) is <= crit[k] ([K]: one confidence level of
    `feldman_cousins` over all points).  `response`: as in `metric_matrix`, for critical values made with it."""
    _check_metric(metric)
    crit = np.asarray(crit, dtype=np.float64)
    if crit.shape != (len(grid),):
        raise ValueError("accepted: crit holds one critical value per point of the grid")
    rows = _data_rows(data_map)
    if rows.shape[0] != 1:
        raise ValueError("accepted: one observed map")
    m = _host(metric_matrix(rows, grid, metric, True, solver, response))[0]
    delta = m.max() - m if metric in _MAXIMISED else m - m.min()
    return delta <= crit


# ------------------------------------------------------------------------------------- the nuisance posterior
_START_STREAM = 0x40000000     # stream of the starts of point k: _START_STREAM + k (the data streams are the points')
_TAU_LENGTHS = 50              # a tau estimate is reliable from this many tau of steps on


def autocorr_time(series, c=5.0):
    """The integrated autocorrelation time of a series [n] (or of every column of [n, J]) in its own steps, as emcee
    defines it: the autocorrelation function by FFT, tau(M) = 1 + 2 sum_{t=1..M} rho(t), and Sokal's window, the
    smallest M with M >= c tau(M) (c = 5).  A constant series gives NaN."""
    x = np.asarray(series, dtype=np.float64)
    if x.ndim == 2:
        return np.array([autocorr_time(x[:, j], c) for j in range(x.shape[1])])
    n = x.size
    if n < 2 or not np.isfinite(x).all() or np.ptp(x) == 0.0:
        return float("nan")
    size = 1 << int(math.ceil(math.log2(2 * n)))
    f = np.fft.rfft(x - x.mean(), n=size)
    acf = np.fft.irfft(f * np.conjugate(f))[:n]
    acf = acf / acf[0]
    taus = 2.0 * np.cumsum(acf) - 1.0
    m = np.arange(n) < c * taus
    window = int(np.argmin(m)) if not m.all() else n - 1
    return float(taus[window])


class PosteriorSample:
    """What `posterior_sample` returns: `points` (the grid points sampled, a list), `names`, and per point i
    eta [P, n_keep * W, J] the displacements, all walkers of the first kept step first (the order of emcee's
    flatchain); values = the parameters' values at the point + eta (None for a response without `values`); logp
    [P, n_keep * W]; acceptance [P], the share of accepted proposals of the kept chain; tau [P, J] the integrated
    autocorrelation time of the walker-mean series in steps; reliable [P]: the chain that tau was estimated on is at
    least 50 tau long; status [P], the sampler's flags (a flagged point is NaN); thin, n_burn, seed, n_walkers."""

    def __init__(self, points, names, eta, values, logp, acceptance, tau, reliable, status, thin, n_burn, seed,
                 n_walkers):
        self.points, self.names = list(points), tuple(names)
        self.eta, self.values, self.logp = eta, values, logp
        self.acceptance, self.tau, self.reliable, self.status = acceptance, tau, reliable, status
        self.thin, self.n_burn, self.seed, self.n_walkers = int(thin), int(n_burn), int(seed), int(n_walkers)

    def __len__(self):
        return int(self.eta.shape[1])

    def mean(self):
        """[P, J]: the posterior means of the displacements"""
        return self.eta.mean(axis=1)

    def cov(self):
        """[P, J, J]: the sample covariance of the displacements"""
        d = self.eta - self.eta.mean(axis=1, keepdims=True)
        return np.einsum("pni,pnj->pij", d, d) / max(self.eta.shape[1] - 1, 1)

    def interval(self, cl=0.6827):
        """(lower, upper) [P, J]: the equal-tailed credible interval of every displacement at the level cl"""
        if not 0.0 < cl < 1.0:
            raise ValueError("PosteriorSample.interval: 0 < cl < 1")
        q = np.quantile(self.eta, [0.5 * (1.0 - cl), 0.5 * (1.0 + cl)], axis=1)
        return q[0], q[1]


def _start_scales(response, k, cov, lower, upper):
    """the spread of the starts of point k per coordinate: sqrt(cov_jj) where that is > 0, else the prior's stddev,
    else an eighth of a finite box; 0 for a pinned coordinate; never more than a quarter of a finite box, so that the
    box holds at least half of the normal the starts are drawn from wherever its centre lies"""
    n_j = len(response.names)
    lo = np.full(n_j, -np.inf) if lower is None else lower
    hi = np.full(n_j, np.inf) if upper is None else upper
    ips = np.asarray(response.inv_prior_sigma, dtype=np.float64)
    scale = np.zeros(n_j)
    for j in range(n_j):
        width = hi[j] - lo[j]
        if width == 0.0:
            continue
        var = float(cov[j, j]) if cov is not None else float("nan")
        if var > 0.0:
            scale[j] = math.sqrt(var)
        elif ips[j] > 0.0:
            scale[j] = 1.0 / ips[j]
        elif np.isfinite(width):
            scale[j] = width / 8.0
        else:
            raise ValueError("posterior_sample: no scale for the starts of '%s' at point %d: the fit gives no variance, "
                             "and the parameter has neither a prior nor a finite range" % (response.names[j], k))
        if np.isfinite(width):
            scale[j] = min(scale[j], width / 4.0)
    return scale


def posterior_sample(observed, grid, metric, response, points=None, n_keep=200, n_walkers=128, thin=None, n_burn=None,
                     pilot_steps=2000, random_state=None, solver=None):
    """Samples of p(eta | observed map, point k) for the points `points` of the grid (default: all): the posterior of
    the response's displacements under the metric's likelihood -- ln p = -Phi (llh, poisson_llh) or -Phi / 2 (chi2,
    mod_chi2) of the profiled fit's objective Phi, Gaussian priors included, flat inside the response's box and on
    the domain where the linearised template is positive -- by the stretch-move ensemble sampler of csrc/posterior.hip,
    every point a chain ensemble of `n_walkers` walkers, all of them in one launch (`solver.posterior`; DESIGN.md §4,
    "Trial ensembles: the nuisance posterior") -> a `PosteriorSample` of n_keep * n_walkers rows per point.
    Start: the observed map is fitted once at all points (`fit_observed(..., covariance=True)`; a point whose fit
    carries a flag other than a held coordinate is refused), and the walkers of point k start at independent normals
    about eta_obs[k] truncated to the box (`solver.draw_linear`, stream 0x40000000 + k, the data discarded) with the
    spreads of `_start_scales`.  The chains of point k read the random numbers of (seed, stream 0, chain id k), so a
    subset of points reproduces the full run's rows.
    Lengths: with `thin` and `n_burn` given, n_burn steps are dropped and every thin-th of the next n_keep * thin kept.
    Where either is None a pilot of `pilot_steps` steps is run first; it is (part of) the burn-in, the chain goes on
    from its end (the sampler's continuation property), and thin = ceil(max tau) of the pilot's second half.  tau is
    `autocorr_time` of the walker-mean series per parameter; where the steps an estimate rests on are fewer than 50
    tau a warning is logged and `reliable` is False.  seed: `random_state`, or one draw from it if a RandomState."""
    from pisa_amd.utils.log import logging

    _check_metric(metric)
    solver = DeviceSolver() if solver is None else solver
    if response is None:
        raise ValueError("posterior_sample: needs response=, the linear response whose parameters are sampled")
    _check_response(response, grid, solver, "posterior_sample", metric)
    _check_linear(response, "posterior_sample", "the sampler")
    _check_narrow(response, "posterior_sample", "the sampler")
    for name in ("posterior", "draw_linear", "hesse"):
        if not hasattr(solver, name):
            raise ValueError("ensemble: posterior_sample needs a solver with %s; %s has none"
                             % (name, type(solver).__name__))
    points = list(range(len(grid))) if points is None else [int(k) for k in points]
    for k in points:
        if not 0 <= k < len(grid):
            raise ValueError("posterior_sample: point %s outside the grid's %d points" % (k, len(grid)))
    n_j, n_w, n_keep = len(response.names), int(n_walkers), int(n_keep)
    if n_w % 2 or not max(2, 2 * n_j) <= n_w <= 256:
        raise ValueError("posterior_sample: %d walkers; an even number from %d (twice the parameters) to 256"
                         % (n_w, max(2, 2 * n_j)))
    if n_keep < 1 or (thin is not None and int(thin) < 1) or (n_burn is not None and int(n_burn) < 0) or (
            (thin is None or n_burn is None) and int(pilot_steps) < 4):
        raise ValueError("posterior_sample: n_keep >= 1, thin >= 1, n_burn >= 0 and pilot_steps >= 4")
    seed = _base_seed(random_state)
    fit = fit_observed(observed, grid, metric, response, solver, covariance=True)
    bad = [k for k in points if int(fit["status"][k]) & ~_PROFILE_HELD]
    if bad:
        raise ValueError("posterior_sample: the fit of the observed map carries a status flag at the points %s (status "
                         "%s)" % (bad, [int(fit["status"][k]) for k in bad]))
    x0 = np.empty((len(points), n_w, n_j))
    for i, k in enumerate(points):
        R, _, _, lower, upper = _truth_priors(response, k)
        cov = fit["cov"][k] if not np.isnan(fit["cov"][k]).any() else None
        scale = _start_scales(response, k, cov, lower, upper)
        out = solver.draw_linear(grid.hist[k], R, None, "poisson", n_w, seed, stream=_START_STREAM + k, scale=scale,
                                 shift=np.ascontiguousarray(fit["eta"][k], dtype=np.float64), lower=lower, upper=upper)
        x0[i] = _host(out["eta"])
    rows = _data_rows(observed)
    kw = dict(t_of=np.zeros(len(points), dtype=np.int32), k_of=np.array(points, dtype=np.int32),
              sigma2=grid.sigma2_for(metric), inv_prior_sigma=response.inv_prior_sigma, center=response.center,
              stream=0, chain_id=np.array(points, dtype=np.int64), **response.bounds())

    def tau_of(chain, step):
        """[P, J] tau in steps of the walker-mean series of chain [P, n, W, J] whose rows are `step` steps apart, and
        which estimates rest on at least 50 tau"""
        tau = np.array([autocorr_time(chain[i].mean(axis=1)) for i in range(chain.shape[0])]).reshape(-1, n_j) * step
        with np.errstate(invalid="ignore"):
            ok = ~(chain.shape[1] * step < _TAU_LENGTHS * tau).any(axis=1)
        return tau, ok

    first = 0
    reliable = np.ones(len(points), dtype=bool)
    if thin is None or n_burn is None:
        pilot = solver.posterior(metric, rows, grid.hist, response.response, x0, int(pilot_steps), seed,
                                 first_step=0, keep_from=int(pilot_steps) // 2, thin=1, **kw)
        tau_pilot, reliable = tau_of(_host(pilot["chain"]), 1)
        if thin is None:
            worst = np.nanmax(tau_pilot) if np.isfinite(tau_pilot).any() else 1.0
            thin = max(1, int(math.ceil(worst)))
        x0, first = _host(pilot["end"]), int(pilot_steps)
        n_burn = max(first, int(n_burn or 0))
    thin, n_burn = int(thin), int(n_burn)
    n_steps = (n_burn - first) + n_keep * thin
    out = solver.posterior(metric, rows, grid.hist, response.response, x0, n_steps, seed, first_step=first,
                           keep_from=n_burn + thin - 1, thin=thin, **kw)
    chain, logp, status = _host(out["chain"]), _host(out["logp"]), _host(out["status"])
    tau, ok = tau_of(chain, thin)
    reliable = reliable & ok
    for i, k in enumerate(points):
        if status[i]:
            logging.warning("posterior_sample: the chains of point %d did not run (status %d)", k, int(status[i]))
        elif not reliable[i]:
            logging.warning("posterior_sample: point %d: tau = %s steps is estimated on fewer than %d tau; run longer",
                            k, np.round(tau[i], 1), _TAU_LENGTHS)
    eta = chain.reshape(len(points), n_keep * n_w, n_j)
    values = None if response.values is None else np.asarray(response.values)[points][:, None, :] + eta
    acceptance = _host(out["accepted"]).sum(axis=1) / float(n_w * n_steps)
    return PosteriorSample(points, response.names, eta, values, logp.reshape(len(points), n_keep * n_w), acceptance,
                           tau, reliable & (status == 0), status, thin, n_burn, seed, n_w)
