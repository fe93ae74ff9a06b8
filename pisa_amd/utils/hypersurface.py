"""Hypersurface fits of discrete-systematics sets (counterpart of pisa/utils/hypersurface/hypersurface.py):
evaluation, loading, and fitting -- `Hypersurface.fit` (:477-1005) and `fit_hypersurfaces` (:1598-1874).  The
per-bin Minuit loop of the reference (:699-959) is ONE launch of `pisa_hip_hypersurface_fit` over all bins of all
maps (csrc/hsfit.hip); everything around it is host code, and the batch solver is an
argument (`solver=`, default `device_batch_solver`).

    scale[bin] = intercept[bin] + sum_p f_p(value_p - nominal_p; coefficients_p[bin])     (:430-433)
    scale      = exp(scale)  if the fit was done in log mode                              (:435)

with the functional forms of :81-205 (`linear`, `quadratic`, `exponential`,
`exponential_scaled`, `logarithmic`), the uncertainty of the scale from the per-bin fit
covariance (:437-470), and `fluctuate` (:1285-1322).

Sources (`load_hypersurfaces`, :1877-1964):
* fit files written by `fit_hypersurfaces` -- JSON (optionally .bz2) holding
  {map name: Hypersurface.serializable_state} (:1182-1215, 1529-1552);
* the CSV hyperplanes of the public IceCube 3-year data release
  (`_load_hypersurfaces_data_release`, :2065-2173): linear terms in the RAW parameter values
  (`using_legacy_data`, :432).
Interpolated hypersurfaces (hyper_interpolator.py) are not part of this build.
"""
import bz2
import copy
import json
import os
from collections import OrderedDict
from collections.abc import Mapping, Sequence

import numpy as np
import pandas as pd

from pisa_amd import FTYPE
from pisa_amd.utils.resources import find_resource

__all__ = ["HypersurfaceInterpolator", "load_interpolated_hypersurfaces", "Hypersurface", "HypersurfaceParam", "HYPERSURFACE_PARAM_FUNCTIONS", "load_hypersurfaces",
           "fit_hypersurfaces", "get_hypersurface_file_name", "device_batch_solver", "FIT_METHOD"]

FIT_METHOD = "pisa_hip_hypersurface_fit"      # what `Hypersurface.fit_method` records: the solver of this build


# functional forms: name -> (number of coefficients, f(p, *coeffts), gradient wrt the coefficients)
def _lin(p, m):
    return m * p


def _lin_grad(p, m):
    return np.broadcast_to(p, np.shape(m * p))[..., np.newaxis]


def _quad(p, m1, m2):
    return m1 * p + m2 * p ** 2


def _quad_grad(p, m1, m2):
    shape = np.shape(m1 * p)
    return np.stack([np.broadcast_to(p, shape), np.broadcast_to(p ** 2, shape)], axis=-1)


def _exp(p, b):
    return np.exp(b * p) - 1.0


def _exp_grad(p, b):
    return (p * np.exp(b * p))[..., np.newaxis]


def _exp_scaled(p, a, b):
    return (a + 1.0) * (np.exp(b * p) - 1.0)


def _exp_scaled_grad(p, a, b):
    return np.stack([np.exp(b * p) - 1.0, (a + 1.0) * p * np.exp(b * p)], axis=-1)


def _log(p, m):
    return np.log(1 + m * p)


def _log_grad(p, m):
    return (p / (1 + m * p))[..., np.newaxis]


HYPERSURFACE_PARAM_FUNCTIONS = OrderedDict([
    ("linear", (1, _lin, _lin_grad)),
    ("quadratic", (2, _quad, _quad_grad)),
    ("exponential", (1, _exp, _exp_grad)),
    ("exponential_scaled", (2, _exp_scaled, _exp_scaled_grad)),
    ("logarithmic", (1, _log, _log_grad)),
])


class HypersurfaceParam:
    """one systematic parameter of a hypersurface: functional form + per-bin coefficients
    `fit_coeffts[binning..., num_fit_coeffts]` (hypersurface.py:1325-1583)"""

    def __init__(self, name, func_name, fit_coeffts=None, nominal_value=0.0, fit_coeffts_sigma=None,
                 initial_fit_coeffts=None, bounds=None, coeff_prior_sigma=None):
        """`fit_coeffts=None`: a parameter that is not fitted yet (the reference's constructor, :1360-1407, with
        its keywords `initial_fit_coeffts`, `bounds` -- one 2-tuple or a tuple of 2-tuples, :868-880 -- and
        `coeff_prior_sigma`)"""
        if func_name not in HYPERSURFACE_PARAM_FUNCTIONS:
            raise ValueError("Hypersurface function '%s' not known; choose from %s"
                             % (func_name, list(HYPERSURFACE_PARAM_FUNCTIONS)))
        self.name, self.func_name = name, func_name
        self.num_fit_coeffts, self._func, self._grad = HYPERSURFACE_PARAM_FUNCTIONS[func_name]
        self.fitted = fit_coeffts is not None
        self.fit_coeffts = None
        if self.fitted:
            self.fit_coeffts = np.asarray(fit_coeffts, dtype=FTYPE)
            assert self.fit_coeffts.shape[-1] == self.num_fit_coeffts
        self.fit_coeffts_sigma = fit_coeffts_sigma
        self.nominal_value = nominal_value
        self.fit_param_values = None
        self.bounds = bounds
        self.coeff_prior_sigma = coeff_prior_sigma
        if coeff_prior_sigma is not None:
            assert len(coeff_prior_sigma) == self.num_fit_coeffts, \
                "number of prior sigma values must equal the number of parameters."
        self.initial_fit_coeffts = initial_fit_coeffts
        if initial_fit_coeffts is not None:
            self.initial_fit_coeffts = np.array(initial_fit_coeffts)
            assert self.initial_fit_coeffts.size == self.num_fit_coeffts, \
                "'initial_fit_coeffts' should have %i values, found %i" % (self.num_fit_coeffts,
                                                                          self.initial_fit_coeffts.size)

    def _fit_bounds(self):
        """(lo, hi) per coefficient, +-inf where there is none (:868-880)"""
        if self.bounds is None:
            return [(-np.inf, np.inf)] * self.num_fit_coeffts
        if np.ndim(self.bounds) == 1:
            assert len(self.bounds) == 2, "bounds on single coefficients must be given as 2-tuples"
            pairs = [self.bounds]
        else:
            assert np.ndim(self.bounds) == 2 and all(len(t) == 2 for t in self.bounds), \
                "bounds must be given as a tuple of 2-tuples"
            pairs = list(self.bounds)
        assert len(pairs) == self.num_fit_coeffts, "one pair of bounds per coefficient"
        return [(-np.inf if a is None else float(a), np.inf if b is None else float(b)) for a, b in pairs]

    def _coeffts(self):
        return [self.fit_coeffts[..., i] for i in range(self.num_fit_coeffts)]

    def evaluate(self, param):
        return self._func(param, *self._coeffts())

    def gradient(self, param):
        return self._grad(param, *self._coeffts())

    @property
    def serializable_state(self):
        def plain(v):
            return None if v is None else np.asarray(v).tolist()

        bounds = None if self.bounds is None else [[None if b is None else float(b) for b in pair]
                                                   for pair in np.asarray(self.bounds, dtype=object).reshape(-1, 2)]
        return OrderedDict(name=self.name, func_name=self.func_name, num_fit_coeffts=self.num_fit_coeffts,
                           fit_coeffts=self.fit_coeffts.tolist(),
                           fit_coeffts_sigma=plain(self.fit_coeffts_sigma),
                           initial_fit_coeffts=plain(self.initial_fit_coeffts), fitted=True,
                           fit_param_values=plain(self.fit_param_values),
                           binning_shape=list(self.fit_coeffts.shape[:-1]),
                           nominal_value=self.nominal_value, bounds=bounds,
                           coeff_prior_sigma=plain(self.coeff_prior_sigma))

    @classmethod
    def from_state(cls, state):
        return cls(state["name"], state["func_name"], np.asarray(state["fit_coeffts"], dtype=FTYPE),
                   nominal_value=state.get("nominal_value", 0.0),
                   fit_coeffts_sigma=state.get("fit_coeffts_sigma"),
                   initial_fit_coeffts=state.get("initial_fit_coeffts"), bounds=state.get("bounds"),
                   coeff_prior_sigma=state.get("coeff_prior_sigma"))


class Hypersurface:
    def __init__(self, binning=None, params=None, intercept=None, log=False, fit_cov_mat=None,
                 using_legacy_data=False, initial_intercept=None):
        """A fitted hypersurface `(binning, params, intercept, ...)`, or -- the reference's constructor, :263-298,
        by keyword -- one still to be fitted: `Hypersurface(params=[...], initial_intercept=None, log=False)`"""
        assert params is not None, "a hypersurface needs its params"
        self.params = OrderedDict()
        for p in params:
            assert p.name not in self.params, "Duplicate param name found : %s" % p.name
            self.params[p.name] = p
        self.log = bool(log)
        self.using_legacy_data = bool(using_legacy_data)
        self.initial_intercept = initial_intercept
        self.binning = binning
        self.intercept = self.intercept_sigma = None
        self.fit_cov_mat = self.fit_chi2 = self.fit_method = self.fit_status = None
        self.fit_maps_raw = self.fit_maps_norm = self.fit_maps_smooth = None
        self.fit_pipeline_param_values = None
        self.fit_info_stored = False
        self.fit_complete = intercept is not None
        if intercept is None:
            return
        shape = binning.shape if binning is not None else np.shape(intercept)
        self.intercept = np.asarray(intercept, dtype=FTYPE).reshape(shape)
        for p in self.params.values():
            p.fit_coeffts = p.fit_coeffts.reshape(tuple(shape) + (p.num_fit_coeffts,))
        self.fit_cov_mat = None if fit_cov_mat is None else np.asarray(fit_cov_mat, dtype=FTYPE)

    param_names = property(lambda self: list(self.params.keys()))
    nominal_values = property(lambda self: OrderedDict((n, p.nominal_value) for n, p in self.params.items()))

    @property
    def num_fit_coeffts(self):
        return int(1 + sum(p.num_fit_coeffts for p in self.params.values()))

    @property
    def fit_coeffts(self):
        """all coefficients of all bins, [binning..., intercept + params' coefficients] (:1144-1157)"""
        cols = [self.intercept]
        for p in self.params.values():
            cols += [p.fit_coeffts[..., i] for i in range(p.num_fit_coeffts)]
        return np.stack(cols, axis=-1)

    def evaluate(self, param_values, return_uncertainty=False):
        """scale factors of all bins for one scalar value per parameter (:356-475, the all-bins
        case the stage uses)"""
        out = np.array(self.intercept, dtype=FTYPE)
        deltas = OrderedDict()
        for name, p in self.params.items():
            value = param_values[name]
            assert np.isscalar(value), "sys param values must be a scalar when evaluating all bins simultaneously"
            deltas[name] = value if self.using_legacy_data else value - p.nominal_value
            out += p.evaluate(deltas[name])
        factors = np.exp(out) if self.log else out
        if not return_uncertainty:
            return factors
        if self.fit_cov_mat is None:
            raise ValueError("this hypersurface carries no fit covariance (e.g. the data-release hyperplanes)")
        grad = np.full(out.shape + (self.num_fit_coeffts,), np.nan, dtype=FTYPE)
        grad[..., 0] = 1.0     # intercept
        i = 1
        for name, p in self.params.items():
            g = p.gradient(deltas[name])
            for j in range(p.num_fit_coeffts):
                grad[..., i] = g[..., j]
                i += 1
        if self.log:
            grad = factors[..., np.newaxis] * grad
        tj = np.einsum("...j,...kj->...k", grad, self.fit_cov_mat)
        variance = np.einsum("...j,...j", tj, grad)
        assert np.all(variance[np.isfinite(variance)] >= 0.0), "invalid covariance"
        return factors, np.sqrt(variance)

    def fluctuate(self, random_state=None):
        """a copy with every bin's coefficients drawn from N(fit, covariance) (:1285-1322)"""
        if self.fit_cov_mat is None:
            raise ValueError("this hypersurface carries no fit covariance")
        rs = random_state if random_state is not None else np.random.RandomState(12345)
        new = copy.deepcopy(self)
        coeffts = self.fit_coeffts
        for idx in np.ndindex(*self.intercept.shape):
            if np.all(np.isfinite(coeffts[idx])):
                draw = rs.multivariate_normal(coeffts[idx], self.fit_cov_mat[idx])
                new.intercept[idx] = draw[0]
                n = 1
                for p in new.params.values():
                    for i in range(p.num_fit_coeffts):
                        p.fit_coeffts[idx + (i,)] = draw[n]
                        n += 1
        return new

    # ------------------------------------------------------------------ fitting
    def fit(self, nominal_map, nominal_param_values, sys_maps, sys_param_values, norm=True, method=None,
            fix_intercept=False, intercept_bounds=None, intercept_sigma=None, include_empty=False,
            keep_maps=True, ref_bin_idx=None, smooth_method=None, smooth_kw=None, solver=None, max_iter=200):
        """Fit the coefficients of every bin to the nominal and systematic maps (hypersurface.py:477-1005).
        `method` and `ref_bin_idx` are accepted for the reference's signature and ignored: the fit is
        `FIT_METHOD`.  `solver`: the batch solver (default `device_batch_solver`, one kernel launch)."""
        job = self._fit_prepare(nominal_map, nominal_param_values, sys_maps, sys_param_values, norm, fix_intercept,
                                intercept_bounds, intercept_sigma, include_empty, smooth_method, smooth_kw)
        _fit_batch([(self, job)], solver, max_iter)
        if not keep_maps:
            self.drop_fit_maps()

    def drop_fit_maps(self):
        self.fit_maps_raw = self.fit_maps_smooth = self.fit_maps_norm = None
        self.fit_info_stored = False

    fit_maps = property(lambda self: self.fit_maps_raw if self.fit_maps_norm is None else self.fit_maps_norm)

    def _fit_prepare(self, nominal_map, nominal_param_values, sys_maps, sys_param_values, norm, fix_intercept,
                     intercept_bounds, intercept_sigma, include_empty, smooth_method, smooth_kw):
        """the reference's checks and data preparation (:533-693) -> the design and the stacked maps of the fit"""
        from pisa_amd.core.map import Map

        assert isinstance(nominal_map, Map)
        assert isinstance(nominal_param_values, Mapping)
        assert set(nominal_param_values.keys()) == set(self.param_names), \
            "Params mismatch : %s != %s" % (set(nominal_param_values.keys()), set(self.param_names))
        assert all(isinstance(k, str) for k in nominal_param_values.keys())
        assert all(np.isscalar(v) for v in nominal_param_values.values())
        assert isinstance(sys_maps, Sequence) and isinstance(sys_param_values, Sequence)
        assert len(sys_maps) == len(sys_param_values)
        for sys_map, vals in zip(sys_maps, sys_param_values):
            assert isinstance(sys_map, Map) and isinstance(vals, Mapping)
            assert set(vals.keys()) == set(self.param_names), \
                "self.param_names: %s\n sys_param_vals.keys(): %s" % (self.param_names, vals.keys())
            assert all(isinstance(k, str) for k in vals.keys())
            assert all(np.isscalar(v) for v in vals.values())
            assert sys_map.binning == nominal_map.binning
        assert not (include_empty and self.log), "empty bins cannot be included in log mode"
        self.fit_method = FIT_METHOD
        self.smooth_method, self.smooth_kw = smooth_method, smooth_kw
        if smooth_method is not None:
            raise Exception("Hypersurface smoothing needs some fixing")      # :606

        # _init (:300-339)
        self.binning = binning = nominal_map.binning
        if self.initial_intercept is None:
            self.initial_intercept = 0.0 if self.log else 1.0
        for p in self.params.values():
            p.nominal_value = nominal_param_values[p.name]
            if p.initial_fit_coeffts is None:
                p.initial_fit_coeffts = np.zeros(p.num_fit_coeffts, dtype=FTYPE)
        maps = [nominal_map] + list(sys_maps)
        param_values = [nominal_param_values] + list(sys_param_values)
        self.fit_maps_raw, self.fit_maps_smooth, self.fit_maps_norm = maps, None, None
        self.fit_info_stored = True
        for name, p in self.params.items():
            p.fit_param_values = np.array([v[name] for v in param_values])
        x = np.asarray([self.params[n].fit_param_values - self.params[n].nominal_value for n in self.params],
                       dtype=FTYPE)

        # normalisation (:654-681): value and error over the nominal value, NaN where that is 0 or masked
        finite_mask = nominal_map.nominal_values != 0
        if binning.mask is not None:
            finite_mask = finite_mask & binning.mask
        if norm:
            nominal = nominal_map.nominal_values
            self.fit_maps_norm = []
            for m in maps:
                val, err = np.full(binning.shape, np.nan), np.full(binning.shape, np.nan)
                val[finite_mask] = m.nominal_values[finite_mask] / nominal[finite_mask]
                err[finite_mask] = m.std_devs[finite_mask] / nominal[finite_mask]
                self.fit_maps_norm.append(Map(m.name, val, binning, error_hist=err))
        for m in self.fit_maps:
            assert np.all(m.nominal_values[finite_mask] >= 0.0), "Found negative bin counts"

        y = np.stack([np.asarray(m.nominal_values, dtype=np.float64).reshape(-1) for m in self.fit_maps])
        sigma = np.stack([np.asarray(m.std_devs, dtype=np.float64).reshape(-1) for m in self.fit_maps])
        if include_empty:
            sigma[sigma == 0.0] = 1.0                                        # :744-747
        if binning.mask is not None:
            y[:, ~binning.mask.reshape(-1)] = np.nan                         # a masked bin is not fitted (:702-717)

        # start point, bounds and prior weights, the intercept first (:760-880)
        p0, bounds, ips = [float(self.initial_intercept)], [(-np.inf, np.inf)], [0.0]
        if not fix_intercept:
            if intercept_bounds is not None:
                assert len(intercept_bounds) == 2 and np.ndim(intercept_bounds) == 1, \
                    "intercept bounds must be given as 2-tuple"
                bounds = [(-np.inf if intercept_bounds[0] is None else float(intercept_bounds[0]),
                           np.inf if intercept_bounds[1] is None else float(intercept_bounds[1]))]
        if intercept_sigma is not None:
            ips = [1.0 / intercept_sigma]
        for p in self.params.values():
            p0 += [float(v) for v in np.asarray(p.initial_fit_coeffts).reshape(-1)]
            bounds += p._fit_bounds()
            ips += [0.0] * p.num_fit_coeffts if p.coeff_prior_sigma is None else \
                [1.0 / v for v in p.coeff_prior_sigma]
        ips = np.array(ips, dtype=np.float64)
        assert np.all(np.isfinite(ips)), "invalid values found in prior sigma. They must not be zero."
        n_free = len(p0) - (1 if fix_intercept else 0)
        assert y.shape[0] >= n_free, \
            "Number of datasets used for fitting (%i) must be >= num free params (%i)" % (y.shape[0], n_free)
        return dict(x=x, forms=[p.func_name for p in self.params.values()], y=y, sigma=sigma,
                    p0=np.array(p0), lo=np.array([b[0] for b in bounds]), hi=np.array([b[1] for b in bounds]),
                    ips=ips, log=self.log, fix_intercept=bool(fix_intercept))

    def _fit_finish(self, res, fix_intercept):
        """the solver's arrays of this map's bins -> the attributes the reference's fit leaves (:934-1005)"""
        shape = tuple(self.binning.shape)
        coef, cov = res["coef"], res["cov"]
        n_coef = coef.shape[1]
        with np.errstate(invalid="ignore"):
            sig = np.sqrt(np.einsum("kii->ki", cov))
        self.intercept = coef[:, 0].reshape(shape).astype(FTYPE)
        self.intercept_sigma = np.full(shape, np.nan, dtype=FTYPE) if fix_intercept else \
            sig[:, 0].reshape(shape).astype(FTYPE)
        i = 1
        for p in self.params.values():
            k = p.num_fit_coeffts
            p.fit_coeffts = coef[:, i:i + k].reshape(shape + (k,)).astype(FTYPE)
            p.fit_coeffts_sigma = sig[:, i:i + k].reshape(shape + (k,)).astype(FTYPE)
            p.fitted = True
            i += k
        self.fit_cov_mat = cov.reshape(shape + (n_coef, n_coef)).astype(FTYPE)
        self.fit_chi2 = np.moveaxis(res["chi2"], 0, -1).reshape(shape + (res["chi2"].shape[0],)).astype(FTYPE)
        self.fit_status = res["status"].reshape(shape).astype(np.int32)
        self.fit_n_iter = res["n_iter"].reshape(shape).astype(np.int32)
        self.fit_complete = True

    @property
    def num_fit_sets(self):
        return len(self.fit_maps)

    @property
    def serializable_state(self):
        """the keys `Hypersurface.from_state` of the reference reads (:1182-1283).  What only a fit fills
        (`intercept_sigma`, `fit_chi2`, `fit_method`, ...) is None for an object that was loaded or built from
        coefficients.  The three map lists are never written (`fit_info_stored: False`): the file is what the
        reference writes after `keep_maps=False`."""
        assert self.fit_complete, "nothing to write: this hypersurface is not fitted"
        state = OrderedDict()
        state["_initialized"] = True
        state["binning"] = None if self.binning is None else getattr(self.binning, "serializable_state", None)
        state["initial_intercept"] = self.initial_intercept
        state["log"] = self.log
        state["intercept"] = self.intercept.tolist()
        state["intercept_sigma"] = None if self.intercept_sigma is None else self.intercept_sigma.tolist()
        state["fit_complete"] = True
        state["fit_info_stored"] = False
        state["fit_maps_norm"] = state["fit_maps_smooth"] = state["fit_maps_raw"] = None
        state["fit_chi2"] = None if self.fit_chi2 is None else self.fit_chi2.tolist()
        state["fit_cov_mat"] = None if self.fit_cov_mat is None else self.fit_cov_mat.tolist()
        state["fit_method"] = self.fit_method
        state["fit_pipeline_param_values"] = self.fit_pipeline_param_values
        state["using_legacy_data"] = self.using_legacy_data
        state["params"] = OrderedDict((n, p.serializable_state) for n, p in self.params.items())
        return state

    @classmethod
    def from_state(cls, state, binning=None):
        if not isinstance(state, Mapping):
            state = _read_json(state)
        params = [HypersurfaceParam.from_state(s) for s in state["params"].values()]
        if binning is None and isinstance(state.get("binning"), Mapping):
            from pisa_amd.core.binning import MultiDimBinning       # the file's own binning (:1262-1264)

            binning = MultiDimBinning(**state["binning"])
        hsf = cls(binning, params, np.asarray(state["intercept"], dtype=FTYPE), log=state.get("log", False),
                  fit_cov_mat=state.get("fit_cov_mat"), using_legacy_data=state.get("using_legacy_data", False),
                  initial_intercept=state.get("initial_intercept"))
        hsf.fit_method = state.get("fit_method")
        hsf.fit_pipeline_param_values = state.get("fit_pipeline_param_values")
        for key in ("intercept_sigma", "fit_chi2"):
            if state.get(key) is not None:
                setattr(hsf, key, np.asarray(state[key], dtype=FTYPE))
        return hsf


def _read_json(path):
    path = find_resource(path)
    opener = bz2.open if path.endswith(".bz2") else open
    with opener(path, "rt") as fh:
        return json.load(fh, object_pairs_hook=OrderedDict)


def _load_data_release(input_file, binning):
    """hypersurface.py:2065-2173: one CSV per map class, columns = bin midpoints, `offset`, one
    gradient per parameter; evaluated with the RAW parameter values"""
    assert binning is not None, "Must provide binning when loading data release hypersurfaces"
    files = OrderedDict([("nue_cc+nuebar_cc", "nue_cc"), ("numu_cc+numubar_cc", "numu_cc"),
                         ("nutau_cc+nutaubar_cc", "nutau_cc"), ("nu_nc+nubar_nc", "all_nc")])
    out = OrderedDict()
    param_names = None
    for map_name, tag in files.items():
        table = pd.read_csv(find_resource(input_file.replace("*", tag)))
        for n in binning.names:
            midpoints = np.unique(table.pop(n).values)
            assert midpoints.size == binning[n].num_bins, \
                "Mismatch between expected and actual binning dimensions"
        offset = table.pop("offset")
        if param_names is None:
            param_names = table.columns.tolist()
        else:
            assert param_names == table.columns.tolist(), \
                "Mismatch between hypersurface params in different files"
        params = [HypersurfaceParam(n, "linear", table[n].values.reshape(binning.shape + (1,)))
                  for n in param_names]
        out[map_name] = Hypersurface(binning, params, offset.values, using_legacy_data=True)
    return out


def _load_legacy(data, expected_binning):
    """hyperplane (linear) fit files of older PISA versions (hypersurface.py:1967-2062):
    `sys_list` = parameter names, `map_names`, and per map an array [binning..., 1 + n_sys] of intercept
    and gradients -- either `data[map_name]` or `data["hyperplanes"][map_name]["fit_params"]`.  The
    nominal values are unknown in such files: evaluated with the RAW parameter values."""
    names = list(data["sys_list"])
    out = OrderedDict()
    for map_name in data["map_names"]:
        coeffts = np.asarray(data["hyperplanes"][map_name]["fit_params"] if "hyperplanes" in data
                             else data[map_name], dtype=FTYPE)
        assert coeffts.shape[-1] == 1 + len(names), "one intercept and one gradient per parameter"
        shape = coeffts.shape[:-1]
        if expected_binning is not None and shape != tuple(expected_binning.shape):
            raise AssertionError("Incompatible binning: hypersurface %s, expected %s"
                                 % (shape, expected_binning.shape))
        params = [HypersurfaceParam(n, "linear", coeffts[..., i + 1: i + 2].copy(), nominal_value=np.nan)
                  for i, n in enumerate(names)]
        out[map_name] = Hypersurface(expected_binning, params, coeffts[..., 0].copy(), using_legacy_data=True)
    return out


def load_hypersurfaces(input_file, expected_binning=None):
    """{map name: Hypersurface} from a fit file (json / json.bz2) or from the data-release CSVs
    ('<dir>/hyperplanes_*.csv[.bz2]'); hypersurface.py:1877-1964"""
    assert isinstance(input_file, str)
    if input_file.endswith("json") or input_file.endswith("json.bz2"):
        data = _read_json(input_file)
        assert isinstance(data, Mapping)
        if "sys_list" in data:
            return _load_legacy(data, expected_binning)
        out = OrderedDict()
        for map_name, state in data.items():
            hsf = Hypersurface.from_state(state, binning=expected_binning)
            if expected_binning is not None and hsf.intercept.shape != tuple(expected_binning.shape):
                raise AssertionError("Incompatible binning: hypersurface %s, expected %s"
                                     % (hsf.intercept.shape, expected_binning.shape))
            out[map_name] = hsf
        return out
    if input_file.endswith("csv") or input_file.endswith("csv.bz2"):
        return _load_data_release(input_file, expected_binning)
    raise Exception("Unknown file format : %s" % input_file)


# ------------------------------------------------------------------ fitting: the batch
def device_batch_solver(x, forms, y, sigma, p0, lo, hi, inv_prior_sigma, log_mode, fix_intercept, max_iter=200):
    """the default batch solver: y / sigma [n_sets, n_prob] (host) through ONE launch of
    `pisa_hip_hypersurface_fit`; returns host arrays coef [n_prob, C], cov [n_prob, C, C], chi2 [n_sets, n_prob],
    loss, n_iter, status [n_prob]"""
    from pisa_amd import kernels as K

    res = K.hypersurface_fit(x, forms, K.to_device(y), K.to_device(sigma), p0, lo, hi, inv_prior_sigma, log_mode,
                             fix_intercept, max_iter)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _fit_batch(jobs, solver=None, max_iter=200):
    """[(hypersurface, prepared job)] of ONE design -> one call of the solver over all their bins"""
    from pisa_amd._lib import HSFIT_NOT_CONVERGED, HSFIT_NOT_POSDEF
    from pisa_amd.utils.log import logging

    solver = device_batch_solver if solver is None else solver
    first = jobs[0][1]
    for _, job in jobs[1:]:
        assert job["forms"] == first["forms"] and job["log"] == first["log"]
        assert job["fix_intercept"] == first["fix_intercept"]
        for key in ("x", "p0", "lo", "hi", "ips"):
            assert np.array_equal(job[key], first[key]), "the maps of one call share the design of the fit"
    sizes = [job["y"].shape[1] for _, job in jobs]
    res = solver(first["x"], first["forms"], np.concatenate([job["y"] for _, job in jobs], axis=1),
                 np.concatenate([job["sigma"] for _, job in jobs], axis=1), first["p0"], first["lo"], first["hi"],
                 first["ips"], first["log"], first["fix_intercept"], max_iter)
    start = 0
    for (hsf, job), n in zip(jobs, sizes):
        part = {k: (v[:, start:start + n] if k == "chi2" else v[start:start + n]) for k, v in res.items()}
        hsf._fit_finish(part, job["fix_intercept"])
        start += n
    n_bad = int(np.count_nonzero(res["status"] & (HSFIT_NOT_CONVERGED | HSFIT_NOT_POSDEF)))
    if n_bad:
        logging.warning("hypersurface fit: %d of %d bins did not converge or have no covariance matrix",
                        n_bad, res["status"].size)


def get_hypersurface_file_name(hypersurface, tag):
    """a descriptive file name (hypersurface.py:1585-1595)"""
    return "%s__hypersurface_fits__%dd__%s.json" % (tag, len(hypersurface.params),
                                                     "_".join(hypersurface.param_names))


def _find_hist_stage(pipeline):
    """index of the hist (or kde) stage of a pipeline and whether it is a kde stage (:1714-1729)"""
    for i, stage in enumerate(pipeline.stages):
        if stage.__class__.__name__ in ("hist", "kde"):
            return i, stage.__class__.__name__ == "kde"
    raise RuntimeError("Could not find hist or kde stage in pipeline, aborting.")


def _dataset_mapsets(cfg, pipeline_param_values=None):
    """the weighted MapSet of a dataset's pipeline, the unweighted one (None for a kde stage) and the pipeline's
    parameter values (:1731-1772).  The unweighted pass runs on a SECOND pipeline whose hist stage has the switch
    set before anything is evaluated: the first pipeline keeps what it has planned for its weighted maps."""
    from pisa_amd.core.pipeline import Pipeline

    def fresh():
        return OrderedDict(copy.deepcopy(cfg)) if isinstance(cfg, Mapping) else cfg

    pipeline = Pipeline(fresh())
    values = {p.name: p.value for p in pipeline.params}
    if pipeline_param_values is not None:
        for name, value in values.items():
            assert value == pipeline_param_values[name], \
                "Mismatch in pipeline param '%s' value between nominal and systematic pipelines : %s != %s" \
                % (name, value, pipeline_param_values[name])
    mapset = copy.deepcopy(pipeline.get_outputs())
    hist_idx, is_kde = _find_hist_stage(pipeline)
    if is_kde:
        assert pipeline.stages[hist_idx].bootstrap, \
            "Hypersurfaces can only be fit to KDE histograms if bootstrapping is enabled."
        return mapset, None, values
    del pipeline
    counting = Pipeline(fresh())
    counting.stages[hist_idx].unweighted = True
    return mapset, copy.deepcopy(counting.get_outputs()), values


def fit_hypersurfaces(nominal_dataset, sys_datasets, params, output_dir, tag, combine_regex=None, log=True,
                      minimum_mc=0, minimum_weight=0, solver=None, **hypersurface_fit_kw):
    """Fit one hypersurface per map of the pipelines' output to the nominal and the systematic datasets --
    each {"pipeline_cfg": cfg file or dict, "sys_params": {name: value}} -- and write them to
    `output_dir/<tag>__hypersurface_fits__<n>d__<names>.json` (hypersurface.py:1598-1874).  All maps go through
    one call of the batch solver.  Returns the path, which `load_hypersurfaces` reads."""
    from pisa_amd.utils.fileio import mkdir
    from pisa_amd.utils.jsons import to_json
    from pisa_amd.utils.log import logging

    nominal_dataset, sys_datasets = copy.deepcopy(nominal_dataset), copy.deepcopy(sys_datasets)
    params = copy.deepcopy(params)
    assert isinstance(sys_datasets, Sequence) and isinstance(params, Sequence)
    assert isinstance(output_dir, str) and isinstance(tag, str)
    for dataset in [nominal_dataset] + list(sys_datasets):
        assert isinstance(dataset, Mapping)
        assert "pipeline_cfg" in dataset and isinstance(dataset["pipeline_cfg"], (str, Mapping))
        assert "sys_params" in dataset and isinstance(dataset["sys_params"], Mapping)
    assert len(params) >= 1 and all(isinstance(p, HypersurfaceParam) for p in params)
    logging.info("Hypersurface fit details :  Num params : %i  Num fit coefficients : %i  Num datasets : "
                 "1 nominal + %i systematics  Nominal values : %s", len(params),
                 sum(p.num_fit_coeffts for p in params), len(sys_datasets), nominal_dataset["sys_params"])

    nominal_dataset["mapset"], nominal_dataset["mapset_unweighted"], pipeline_param_values = \
        _dataset_mapsets(nominal_dataset["pipeline_cfg"])
    for dataset in sys_datasets:
        dataset["mapset"], dataset["mapset_unweighted"], _ = \
            _dataset_mapsets(dataset["pipeline_cfg"], pipeline_param_values)
    if combine_regex is not None:
        for dataset in [nominal_dataset] + list(sys_datasets):
            dataset["mapset"] = dataset["mapset"].combine_re(combine_regex)
            if dataset["mapset_unweighted"] is not None:
                dataset["mapset_unweighted"] = dataset["mapset_unweighted"].combine_re(combine_regex)
    # bins with too few MC events or too little weight: value AND error to zero, the set drops out there (:1788-1798)
    for dataset in list(sys_datasets) + [nominal_dataset]:
        for m in dataset["mapset"]:
            insufficient = m.nominal_values < minimum_weight
            if dataset["mapset_unweighted"] is not None:
                insufficient = insufficient | (dataset["mapset_unweighted"][m.name].nominal_values < minimum_mc)
            if np.any(insufficient):
                values, variances = np.array(m.nominal_values), np.array(m.variances)
                values[insufficient] = 0.0
                variances[insufficient] = 0.0
                m._hist, m._var = values, variances

    fit_kw = dict(norm=True, method=None, fix_intercept=False, intercept_bounds=None, intercept_sigma=None,
                  include_empty=False, keep_maps=True, ref_bin_idx=None, smooth_method=None, smooth_kw=None,
                  max_iter=200)
    unknown = set(hypersurface_fit_kw) - set(fit_kw)
    assert not unknown, "not arguments of Hypersurface.fit: %s" % sorted(unknown)
    fit_kw.update(hypersurface_fit_kw)
    hypersurfaces, jobs = OrderedDict(), []
    for m in nominal_dataset["mapset"]:
        hsf = Hypersurface(params=copy.deepcopy(params), initial_intercept=0.0 if log else 1.0, log=log)
        job = hsf._fit_prepare(m, nominal_dataset["sys_params"], [d["mapset"][m.name] for d in sys_datasets],
                               [d["sys_params"] for d in sys_datasets], fit_kw["norm"], fit_kw["fix_intercept"],
                               fit_kw["intercept_bounds"], fit_kw["intercept_sigma"], fit_kw["include_empty"],
                               fit_kw["smooth_method"], fit_kw["smooth_kw"])
        hsf.fit_pipeline_param_values = pipeline_param_values
        hypersurfaces[m.name] = hsf
        jobs.append((hsf, job))
    _fit_batch(jobs, solver, fit_kw["max_iter"])
    if not fit_kw["keep_maps"]:
        for hsf in hypersurfaces.values():
            hsf.drop_fit_maps()
    output_path = os.path.join(output_dir, get_hypersurface_file_name(list(hypersurfaces.values())[0], tag))
    mkdir(output_dir)
    to_json(hypersurfaces, output_path)
    logging.info("Fit results written : %s", output_path)
    return output_path


# ------------------------------------------------------------------ interpolated hypersurfaces
def _quantity(v):
    """a value of an interpolation grid: Quantity, plain number, or the JSON image of a pint quantity
    `[magnitude, [[unit, exponent], ...]]` (jsons.py:300-301, 448-474) -> (magnitude, unit string)"""
    if hasattr(v, "m_as"):
        return float(v.magnitude), str(v.units)
    if isinstance(v, (list, tuple)) and len(v) == 2 and isinstance(v[1], (list, tuple)):
        units = " * ".join("%s**%r" % (u, float(e)) for u, e in v[1]) or "dimensionless"
        return float(v[0]), units
    return float(v), "dimensionless"


def is_psd(m):
    """positive semi-definite by attempted Cholesky factorisation (matrix.py:31-56)"""
    try:
        np.linalg.cholesky(m)
        return True
    except np.linalg.LinAlgError:
        return False


def frobenius_nearest_psd(m):
    """the PSD matrix closest to `m` in the Frobenius norm (Higham 1988; matrix.py:58-117, there
    spelled `fronebius_nearest_psd`)"""
    from scipy import linalg as lin

    b = (m + m.T) / 2.0
    _, h = lin.polar(b)
    x = (b + h) / 2.0
    x = (x + x.T) / 2.0
    if not is_psd(x):
        spacing = np.spacing(lin.norm(x))
        eye, k = np.eye(x.shape[0]), 1
        while not is_psd(x):
            mineig = np.min(np.real(lin.eigvals(x)))
            x += eye * (-mineig * k ** 2 + spacing)
            k += 1
    return x


class HypersurfaceInterpolator:
    """Hypersurfaces fitted at the points of a rectilinear grid of (e.g. oscillation) parameters,
    their coefficients and fit covariances interpolated piecewise-linearly in between
    (hyper_interpolator.py:48-265; `scipy.interpolate.RegularGridInterpolator`).  Requests outside
    the grid are clipped to its bounds; parameters flagged `scales_log` are interpolated in log10."""

    def __init__(self, interpolation_param_spec, hs_fits, ignore_nan=True):
        from scipy import interpolate

        assert isinstance(interpolation_param_spec, OrderedDict), \
            "interpolation params must be specified as a dict with ordered keys"
        self.interp_param_spec = OrderedDict()
        for name, spec in interpolation_param_spec.items():
            assert set(spec.keys()) == {"values", "scales_log"}
            vals = [_quantity(v) for v in spec["values"]]
            assert len({u for _, u in vals}) == 1, "grid values of %s in different units" % name
            self.interp_param_spec[name] = dict(values=np.array([m for m, _ in vals]), units=vals[0][1],
                                                scales_log=bool(spec["scales_log"]))
        self.ndim = len(self.interp_param_spec)
        reference = hs_fits[0]["hs_fit"]
        self._reference = reference
        self.coeff_shape = reference.fit_coeffts.shape
        self.covars_shape = None if reference.fit_cov_mat is None else reference.fit_cov_mat.shape
        self.interp_shape = tuple(len(v["values"]) for v in self.interp_param_spec.values())
        assert len(hs_fits) == int(np.prod(self.interp_shape)), "one fit per grid point"
        coeff_z = np.zeros(self.interp_shape + self.coeff_shape)
        covar_z = None if self.covars_shape is None else np.zeros(self.interp_shape + self.covars_shape)
        for i, idx in enumerate(np.ndindex(self.interp_shape)):
            # the fits are stored in C order of the grid; their parameter values must say so (:139-150)
            for j, (name, spec) in enumerate(self.interp_param_spec.items()):
                got = _quantity(hs_fits[i]["param_values"][name])[0]
                assert got == spec["values"][idx[j]], \
                    "The stored values where hypersurfaces were fit do not match those in the interpolation grid."
            coeff_z[idx] = hs_fits[i]["hs_fit"].fit_coeffts
            if covar_z is not None:
                covar_z[idx] = hs_fits[i]["hs_fit"].fit_cov_mat
        grid = [np.array(spec["values"], dtype=FTYPE) for spec in self.interp_param_spec.values()]
        self.param_bounds = [(np.min(g), np.max(g)) for g in grid]
        for i, spec in enumerate(self.interp_param_spec.values()):
            if spec["scales_log"]:
                grid[i] = np.log10(grid[i])
        self.coefficients = interpolate.RegularGridInterpolator(grid, coeff_z, bounds_error=True, fill_value=None)
        self.covars = None if covar_z is None else \
            interpolate.RegularGridInterpolator(grid, covar_z, bounds_error=True, fill_value=None)
        self.ignore_nan = ignore_nan

    interpolation_param_names = property(lambda self: list(self.interp_param_spec.keys()))
    param_names = property(lambda self: self._reference.param_names)
    binning = property(lambda self: self._reference.binning)
    num_interp_params = property(lambda self: self.ndim)

    def _point(self, param_kw):
        assert set(param_kw.keys()) == set(self.interp_param_spec.keys()), "invalid parameters"
        x = np.empty(self.ndim)
        for i, (name, spec) in enumerate(self.interp_param_spec.items()):
            v = param_kw[name]
            x[i] = v.m_as(spec["units"]) if hasattr(v, "m_as") else float(v)
            x[i] = np.clip(x[i], *self.param_bounds[i])
            if spec["scales_log"]:
                if x[i] <= 0:
                    raise RuntimeError("A log-scaling parameter cannot become zero or negative!")
                x[i] = np.log10(x[i])
        return x

    def get_hypersurface(self, **param_kw):
        """the Hypersurface at the given values of the interpolation parameters (Quantities or
        magnitudes in the grid's units); hyper_interpolator.py:194-265"""
        x = self._point(param_kw)
        hsf = copy.deepcopy(self._reference)
        if self.covars is not None:
            cov = np.squeeze(self.covars(x), axis=0)
            assert cov.shape == self.covars_shape
            for bin_idx in np.ndindex(cov.shape[:-2]):
                m = cov[bin_idx]
                if np.any(~np.isfinite(m)):
                    assert self.ignore_nan, "invalid cov matrix element encountered in bin %s" % (bin_idx,)
                    cov[bin_idx] = m = np.identity(m.shape[0])
                assert np.allclose(m, m.T, rtol=1e-11), "cov matrix not symmetric in bin %s" % (bin_idx,)
                if not is_psd(m):
                    cov[bin_idx] = frobenius_nearest_psd(m)
            hsf.fit_cov_mat = cov
        coeffts = np.squeeze(self.coefficients(x), axis=0)
        assert coeffts.shape == self.coeff_shape
        bad = ~np.isfinite(coeffts)
        if np.any(bad):
            assert self.ignore_nan, "invalid coeff encountered"
            default = np.zeros(self.coeff_shape)
            default[..., 0] = 1.0          # empty bins: intercept 1, slopes 0
            coeffts = np.where(bad, default, coeffts)
        hsf.intercept = coeffts[..., 0].copy()
        i = 1
        for p in hsf.params.values():
            p.fit_coeffts = coeffts[..., i: i + p.num_fit_coeffts].copy()
            i += p.num_fit_coeffts
        return hsf


def load_interpolated_hypersurfaces(input_file, expected_binning=None):
    """{map name: HypersurfaceInterpolator} from a file of `fit_hypersurfaces` run with interpolation
    parameters (hyper_interpolator.py:920-1039):
        {"interpolation_param_spec": {name: {"values": [...], "scales_log": bool}, ...},
         "hs_fits": [{"param_values": {name: value}, "hs_fit": {map name: hypersurface state}}, ...]}
    and the older layout with "interp_params" / "kind": "linear" and one hypersurface file per point."""
    assert isinstance(input_file, str)
    data = _read_json(input_file)
    if "interpolation_param_spec" not in data:
        assert "interp_params" in data and "hs_fits" in data and "kind" in data
        assert data["kind"] == "linear", "Only linear interpolation supported (input file specifies '%s')" % data["kind"]
        spec = OrderedDict()
        for param_def in data["interp_params"]:
            name = param_def["name"]
            values = [fit["param_values"][name] for fit in data["hs_fits"]]
            uniq = []
            for v in values:
                if not any(_quantity(v) == _quantity(u) for u in uniq):
                    uniq.append(v)
            spec[name] = {"scales_log": False, "values": uniq}
        data["interpolation_param_spec"] = spec
        for fit in data["hs_fits"]:
            fit["hs_fit"] = load_hypersurfaces(fit["file"], expected_binning=expected_binning)
    assert {"interpolation_param_spec", "hs_fits"}.issubset(data.keys()), "missing keys"
    map_names = None
    for fit in data["hs_fits"]:
        maps = fit["hs_fit"]
        if map_names is None:
            map_names = list(maps.keys())
        else:
            assert set(map_names) == set(maps.keys()), "inconsistent maps"
        for name in map_names:
            if not isinstance(maps[name], Hypersurface):
                maps[name] = Hypersurface.from_state(maps[name], binning=expected_binning)
            if expected_binning is not None and maps[name].intercept.shape != tuple(expected_binning.shape):
                raise AssertionError("Binning of loaded hypersurfaces does not match the expected binning")
    spec = data["interpolation_param_spec"]
    if not isinstance(spec, OrderedDict):
        spec = OrderedDict(spec)
    out = OrderedDict()
    for name in map_names:
        fits = [{"param_values": fit["param_values"], "hs_fit": fit["hs_fit"][name]} for fit in data["hs_fits"]]
        out[name] = HypersurfaceInterpolator(spec, fits)
    return out
