"""Pull method tools (pisa/utils/pull_method.py): binwise template gradients with respect to the free parameters
and the linearised parameter pulls they give.

`get_derivative_map` and `derivative_from_polycoefficients` are host functions on host arrays, as in the
reference.  `get_gradients` and `calculate_pulls` run on the device: the templates of a parameter's test points
come from the maker's one-sweep path where it has one (`DistributionMaker._fisher_templates`), and the binwise
products and sums are `pisa_hip_fisher`, whose gradients equal `get_derivative_map` bit for bit.

Deviations from the reference (each has a test):
  * `pmaps` is keyed by the test values' magnitudes (in each value's own units): this build's `Quantity` is
    unhashable.
  * A parameter whose test values are not exactly two distinct values raises ValueError (the reference asserts).
  * A fiducial map without errors raises ValueError (the reference divides by zero).
  * `calculate_pulls` takes the nonempty bins of the fiducial map; a `nonempty` that names other bins raises
    ValueError.
"""
import numpy as np

__all__ = ["derivative_from_polycoefficients", "get_derivative_map", "get_gradients", "calculate_pulls"]


def derivative_from_polycoefficients(coeff, loc):
    """derivative of f(x) = coeff[0] + coeff[1] x + coeff[2] x**2 + ... at x = loc (pull_method.py:31-45)"""
    derivative = 0.
    for n, c in enumerate(coeff):
        if n == 0:
            continue
        derivative += n * c * loc ** (n - 1)
    return derivative


def _sorted_pair(test_vals):
    """(lo, hi) of a parameter's test values: exactly two distinct values"""
    vals = list(test_vals)
    if len(vals) != 2:
        raise ValueError("a parameter needs exactly two test values, got %d" % len(vals))
    lo, hi = sorted(vals)
    if not lo < hi:
        raise ValueError("the two test values of a parameter must differ: %s, %s" % (lo, hi))
    return lo, hi


def get_derivative_map(hypo_maps):
    """binwise linear derivatives of counts with respect to a parameter (pull_method.py:48-86): `hypo_maps` maps
    the two test values (Quantities, or the magnitudes `get_gradients` keys by, with `units` unknown) to the
    templates' arrays.  Returns the flat array (T_hi - T_lo) / (hi - lo)."""
    test_points = sorted(hypo_maps.keys())
    hypo_maps_flat = [np.asarray(hypo_maps[pvalue]).flatten() for pvalue in test_points]
    if len(test_points) != 2:
        raise ValueError("get_derivative_map needs exactly two test points, got %d" % len(test_points))
    del_x = test_points[1] - test_points[0]
    del_counts = np.subtract(hypo_maps_flat[1], hypo_maps_flat[0])
    return np.divide(del_counts, getattr(del_x, "magnitude", del_x))


def get_gradients(param, hypo_maker, test_vals):
    """templates at the test values of `param` (each set with `params[param].value = v` and left there) and the
    binwise gradient (pull_method.py:89-128).  Returns (pmaps, gradient_map): pmaps {magnitude: 'total'
    nominal values}, gradient_map as `get_derivative_map`."""
    _sorted_pair(test_vals)
    res = hypo_maker._fisher_templates([param], {param: test_vals})
    pmaps = {v.magnitude if hasattr(v, "magnitude") else v: res["pmaps"][0][i] for i, v in enumerate(test_vals)}
    return pmaps, res["grad"][0]


def calculate_pulls(fisher, fid_maps_truth, fid_hypo_asimov_dist, gradient_maps, nonempty):
    """parameter pulls from the truth, the fiducial template, the Fisher matrix and the binwise gradients
    (pull_method.py:131-193): d_p = sum over nonempty bins of (truth - fiducial) g_p / sigma, on the device
    (`pisa_hip_fisher`), then covariance . d.  Returns [(name, pull)] in `fisher.parameters` order."""
    import torch

    from pisa_amd import kernels as K

    fid = fid_hypo_asimov_dist["total"]
    hist = np.asarray(fid.nominal_values, dtype=np.float64).ravel()
    if not np.array_equal(np.asarray(nonempty[0]), np.nonzero(hist)[0]):
        raise ValueError("nonempty must be the nonzero bins of the fiducial map")
    truth = np.asarray(fid_maps_truth["total"].nominal_values, dtype=np.float64).ravel()
    gm = gradient_maps["total"]
    for param in fisher.parameters:
        if param not in gm:
            raise KeyError("no gradient map for parameter %r" % param)
    n_par, n_bins = len(fisher.parameters), hist.size
    # points: the fiducial, a zero map and the gradients themselves, so that (g - 0) / 1 hands each gradient to
    # the kernel unchanged
    pts = np.zeros((n_par + 2, n_bins))
    pts[0] = hist
    for i, param in enumerate(fisher.parameters):
        pts[i + 2] = np.asarray(gm[param], dtype=np.float64).ravel()
    var = np.zeros_like(pts)
    var[0] = np.asarray(fid.variances, dtype=np.float64).ravel()
    res = K.fisher(K.to_device(pts), K.to_device(var), [1] * n_par, list(range(2, n_par + 2)), [1.0] * n_par,
                   truth=torch.as_tensor(truth))
    if res["status"]:
        raise ValueError("the fiducial map has a nonempty bin without error (sigma = 0): no pulls")
    d = res["pull"].cpu().numpy()
    fisher.calculateCovariance()
    pulls = np.dot(fisher.covariance, d)
    return [(pname, pull) for pname, pull in zip(fisher.parameters, np.asarray(pulls).flat)]
