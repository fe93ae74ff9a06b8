"""The metrics of the hot path as free functions: the interface of pisa/utils/stats.py (`chi2` :98-167, `llh`
:169-253, `poisson_llh` :255-326, `mcllh_mean` :328-382, `mcllh_eff` :384-438, `conv_llh` :558-596, `mod_chi2`
:651-695, `correct_chi2` :697-730, `signed_sqrt_mod_chi2` :762-786) for code that calls them on arrays rather than
through `Map.metric`.  Each returns the PER-BIN values in the shape of its inputs (the caller sums, `np.nansum` in
`Map.metric`, map.py:1601-1604); the arithmetic is `pisa_hip_metric`'s on the GPU -- there is no host
implementation.  `generalized_poisson_llh` (stats.py:792-879) runs on `pisa_hip_generalized_poisson_llh`; it is not
one of `ALL_METRICS`, as in the reference it takes the containers' maps rather than one expectation.  `barlow_llh`
and `weighted_chi2` are not built.

Where the reference reads expected values AND their standard deviations out of an `uncertainties` array
(every metric here but chi2 / llh / poisson_llh), pass a `Map`, or the values and `sigma=`.
"""
import numpy as np

from pisa_amd import FTYPE

__all__ = ["SMALL_POS", "CHI2_METRICS", "LLH_METRICS", "ALL_METRICS", "chi2", "llh", "poisson_llh", "mod_chi2",
           "correct_chi2", "signed_sqrt_mod_chi2", "mcllh_mean", "mcllh_eff", "conv_llh",
           "generalized_poisson_llh"]

SMALL_POS = 1e-10       # expected values are clipped to [SMALL_POS, inf) before logarithms and divisions (stats.py:74)
CHI2_METRICS = ("chi2", "mod_chi2", "correct_chi2", "signed_sqrt_mod_chi2")
LLH_METRICS = ("llh", "poisson_llh", "conv_llh", "mcllh_mean", "mcllh_eff")
ALL_METRICS = LLH_METRICS + CHI2_METRICS


def _values(x):
    from pisa_amd.core.map import Map

    if isinstance(x, Map):
        return x.hist, x._var
    return np.asarray(x, dtype=FTYPE), None


def _per_bin(kind, actual_values, expected_values, sigma=None):
    from pisa_amd import kernels as K

    a, _ = _values(actual_values)
    e, var = _values(expected_values)
    if a.shape != e.shape:
        raise ValueError("Shape mismatch: actual_values.shape = %s, expected_values.shape = %s" % (a.shape, e.shape))
    if sigma is not None:
        var = np.square(np.asarray(sigma, dtype=FTYPE))
        if var.shape != e.shape:
            raise ValueError("Shape mismatch: sigma.shape = %s, expected_values.shape = %s" % (var.shape, e.shape))
    s2 = None
    if kind in K.VARIANCE_METRICS:
        s2 = K.to_device(np.ascontiguousarray(np.zeros_like(e) if var is None else var).ravel())
    _, per_bin = K.metric(kind, K.to_device(np.ascontiguousarray(a).ravel()), K.to_device(np.ascontiguousarray(e).ravel()),
                          s2, per_bin=True)
    return per_bin.cpu().numpy().reshape(a.shape)


def chi2(actual_values, expected_values):
    """Pearson's (N_actual - N_exp)^2 / N_exp per bin"""
    return _per_bin("chi2", actual_values, expected_values)


def llh(actual_values, expected_values):
    """N_actual ln(N_exp) - N_exp - (N_actual ln(N_actual) - N_actual) per bin (Stirling; NaN where a count is 0)"""
    return _per_bin("llh", actual_values, expected_values)


def poisson_llh(actual_values, expected_values):
    """the Poisson log-probability per bin, with the log-gamma function (stats.py:255-326)"""
    return _per_bin("poisson_llh", actual_values, expected_values)


def mod_chi2(actual_values, expected_values, sigma=None):
    """(N_actual - N_exp)^2 / (sigma^2 + N_exp) per bin; sigma from a `Map`'s errors or given (0 otherwise)"""
    return _per_bin("mod_chi2", actual_values, expected_values, sigma)


def correct_chi2(actual_values, expected_values, sigma=None):
    """(N_actual - N_exp)^2 / (sigma^2 + N_exp) + ln(sigma^2 + N_exp) per bin"""
    return _per_bin("correct_chi2", actual_values, expected_values, sigma)


def signed_sqrt_mod_chi2(actual_values, expected_values, sigma=None):
    """the pull (N_actual - N_exp) / sqrt(sigma^2 + N_exp) per bin"""
    return _per_bin("signed_sqrt_mod_chi2", actual_values, expected_values, sigma)


def mcllh_mean(actual_values, expected_values, sigma=None):
    """L_Mean of JHEP06(2019)030, table 2 (Poisson-gamma mixture, a = 0, b = 0); Poisson where sigma = 0"""
    return _per_bin("mcllh_mean", actual_values, expected_values, sigma)


def mcllh_eff(actual_values, expected_values, sigma=None):
    """L_Eff of JHEP06(2019)030, eq. 3.16 (a = 1, b = 0); Poisson where sigma = 0"""
    return _per_bin("mcllh_eff", actual_values, expected_values, sigma)


def conv_llh(actual_values, expected_values, sigma=None):
    """Poisson smeared with a normal of width sigma (101 steps over +-3 sigma), normalised to the value at
    N_actual = N_exp, minus the same at N_exp := N_actual"""
    return _per_bin("conv_llh", actual_values, expected_values, sigma)


GPLLH_KEYS = ("weights", "llh_alphas", "llh_betas", "n_mc_events")


def _gpllh_tables(actual_values, expected_values):
    """[n_cont, n_bins] host arrays of the four MapSets of `expected_values`, checked before any device call"""
    from collections import OrderedDict

    if not isinstance(expected_values, OrderedDict):
        raise TypeError("expected_values must be an OrderedDict of MapSet objects")
    for key in GPLLH_KEYS:
        if key not in expected_values:
            raise KeyError('expected_values need a key named "%s"' % key)
    n_bins = int(np.asarray(actual_values).size)
    tabs = []
    n_cont = None
    for key in GPLLH_KEYS:
        ms = expected_values[key]
        maps = getattr(ms, "maps", None)
        if maps is None:
            raise TypeError('expected_values["%s"] must be a MapSet' % key)
        rows = [np.asarray(m.hist, dtype=FTYPE).ravel() for m in maps]
        if not rows or any(r.size != n_bins for r in rows):
            raise ValueError('expected_values["%s"]: every map needs the %d bins of actual_values' % (key, n_bins))
        if n_cont is not None and len(rows) != n_cont:
            raise ValueError("expected_values: the MapSets hold different numbers of maps")
        n_cont = len(rows)
        tabs.append(np.ascontiguousarray(np.stack(rows)))
    return tabs


def _gpllh_empty(empty_bins, n_bins):
    if empty_bins is None or len(empty_bins) == 0:
        return None
    idx = np.asarray(empty_bins, dtype=np.int64).ravel()
    if idx.min() < 0 or idx.max() >= n_bins:
        raise IndexError("empty_bins: bin index out of range")
    m = np.zeros(n_bins, dtype=np.uint8)
    m[idx] = 1
    return m


def generalized_poisson_total(actual_values, expected_values=None, empty_bins=None):
    """(total, per-bin values) of `generalized_poisson_llh`; the total is the kernel's fixed-order sum"""
    from pisa_amd import kernels as K

    a = np.ascontiguousarray(np.asarray(actual_values, dtype=FTYPE).ravel())
    w, alpha, beta, n_mc = _gpllh_tables(a, expected_values)
    empty = _gpllh_empty(empty_bins, a.size)
    total, per_bin = K.generalized_poisson_llh(
        K.to_device(a), K.to_device(w), K.to_device(alpha), K.to_device(beta), K.to_device(n_mc),
        None if empty is None else K.to_device(empty, dtype=np.uint8))
    return float(total.item()), per_bin.cpu().numpy()


def generalized_poisson_llh(actual_values, expected_values=None, empty_bins=None):
    """The generalized Poisson-gamma likelihood of arXiv:1902.08831 per bin (stats.py:792-879): `expected_values` an
    OrderedDict of MapSets (one map per container) under "weights", "llh_alphas", "llh_betas" and "n_mc_events" (as
    the likelihood.generalized_llh_params service leaves them), `empty_bins` None or bin indices.  Per bin, k = the
    data count truncated to an integer: listed empty bins give log(1e-10) if k > 0, else 0; bins where every
    container has more than 100 MC events give k ln(sum w) - sum w - (k ln k - k) (-sum w at k = 0: the limit, where
    the reference returns NaN); the others eq. 91 over the containers with finite alpha and beta.  Flat array."""
    return generalized_poisson_total(actual_values, expected_values, empty_bins)[1]
