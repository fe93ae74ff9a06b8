"""Writes tests/golden/fisher_ref.npz: the reference's Fisher matrix and pull method on seeded synthetic templates
(arrays and name lists only).  Needs a checkout of the reference (PISA_REFERENCE_ROOT, as oracle/ref_shim.py).
pisa/utils/fisher_matrix.py (build_fisher_matrix, FisherMatrix) and pisa/utils/pull_method.py
(get_derivative_map, calculate_pulls) are the reference's own code, imported by path through the
oracle/ref_shim.py importer with stand-ins for its file and log utilities, and run on duck-typed MapSets.  Nothing
of the reference is kept.

Cases: 128 bins with empty bins at P = 1, 3 and 8 (matrix, gradients, nonempty bins, pulls, the FisherMatrix
methods), the P = 3 matrix with priors added, the sum of two matrices with overlapping parameters, and a
4 800-bin case (the fine3d binning's size).

    python scripts/dev/gen_fisher_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402


def reference_modules():
    ref_shim.install()
    import logging

    sys.modules["pisa.utils.fileio"] = types.SimpleNamespace(from_file=None, to_file=None)
    sys.modules["pisa.utils.log"] = types.SimpleNamespace(logging=logging.getLogger("ref"),
                                                          set_verbosity=lambda *a: None)
    out = []
    for name in ("fisher_matrix", "pull_method"):
        path = os.path.join(ref_shim.REF_ROOT, "pisa", "utils", name + ".py")
        spec = importlib.util.spec_from_file_location("pisa.utils." + name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["pisa.utils." + name] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


class Q(float):
    """a test value: sortable, with `.magnitude` of differences (what pint gives the reference)"""
    magnitude = property(lambda self: float(self))

    def __sub__(self, other):
        return Q(float(self) - float(other))


class DMap:
    def __init__(self, hist, var):
        self.nominal_values = hist
        self.std_devs = np.sqrt(var)


class DSet:
    def __init__(self, m):
        self.m = m
        self.nominal_values = {"total": m.nominal_values}

    def __getitem__(self, key):
        assert key == "total"
        return self.m


def templates(rs, n_bins, n_par, n_empty):
    """fiducial total, its variances, the 2P test-point totals, their values, a truth map"""
    base = rs.gamma(2.0, 40.0, n_bins)
    base[rs.choice(n_bins, n_empty, replace=False)] = 0.0
    var = base * rs.uniform(0.5, 2.0, n_bins)
    pts, vals = [base], []
    for p in range(n_par):
        x0, h = rs.uniform(0.5, 2.0), rs.uniform(0.01, 0.2)
        vals.append((x0 + h, x0 - h))     # the upper value first: the points are not in sorted order
        slope = rs.normal(0.0, 30.0, n_bins) * (base > 0)
        pts += [base + slope * h + rs.normal(0, 0.1, n_bins) * (base > 0), base - slope * h]
    truth = rs.poisson(base).astype(np.float64)
    return np.stack(pts), var, np.array(vals), truth


def main():
    fm, pm = reference_modules()
    rs = np.random.RandomState(20261016)
    out = {}
    cases = dict(p1=(128, 1, 9), p3=(128, 3, 17), p8=(128, 8, 5), big=(4800, 3, 300))
    fishers = {}
    for key, (n_bins, n_par, n_empty) in cases.items():
        pts, var, vals, truth = templates(rs, n_bins, n_par, n_empty)
        names = ["par_%s" % c for c in "qbzaxmyk"[:n_par]]     # not sorted: the matrix is in sorted order
        grads = {}
        for p, name in enumerate(names):
            grads[name] = pm.get_derivative_map({Q(vals[p][0]): pts[1 + 2 * p], Q(vals[p][1]): pts[2 + 2 * p]})
        fid = DSet(DMap(pts[0], var))
        best = rs.uniform(-1, 1, n_par)
        fisher, nonempty = fm.build_fisher_matrix(grads, fid, types.SimpleNamespace(nominal_values=list(best)))
        pulls = pm.calculate_pulls(fisher, DSet(DMap(truth, truth)), fid, {"total": grads}, nonempty)
        out[key + "_points"] = pts
        out[key + "_var"] = var
        out[key + "_vals"] = vals
        out[key + "_truth"] = truth
        out[key + "_names"] = np.array(names)
        out[key + "_best"] = best
        out[key + "_sorted"] = np.array(fisher.parameters)
        out[key + "_matrix"] = np.asarray(fisher.matrix)
        out[key + "_grads"] = np.stack([grads[n] for n in names])
        out[key + "_nonempty"] = nonempty[0]
        out[key + "_pulls"] = np.array([v for _, v in pulls])
        out[key + "_covariance"] = np.asarray(fisher.covariance)
        fishers[key] = fisher
    # the FisherMatrix methods on the P = 3 matrix, without and with priors
    f = fishers["p3"]
    ps = f.parameters
    for tag in ("free", "prior"):
        if tag == "prior":
            f.setPrior(ps[0], 0.05)
            f.addPrior(ps[1], 0.2)
            f.addPrior(ps[1], 0.3)
            out["p3_prior_values"] = np.array(f.priors)
        out["p3_%s_covariance" % tag] = np.asarray(f.covariance)
        out["p3_%s_sigma" % tag] = np.array([f.getSigma(p) for p in ps])
        out["p3_%s_sigma_nopriors" % tag] = np.array([f.getSigmaNoPriors(p) for p in ps])
        out["p3_%s_sigma_stat" % tag] = np.array([f.getSigmaStatistical(p) for p in ps])
        out["p3_%s_sigma_syst" % tag] = np.array([f.getSigmaSystematic(p) for p in ps])
        out["p3_%s_correlation" % tag] = np.array([[f.getCorrelation(a, b) for b in ps] for a in ps])
        out["p3_%s_ellipse" % tag] = np.array([f.getErrorEllipse(ps[0], ps[1]), f.getErrorEllipse(ps[2], ps[0], 0.9)])
    f.removeAllPriors()
    # a sum: P = 3 plus a matrix over one shared and two new parameters (the reference's order follows a set:
    # stored as the name order it produced)
    a = fishers["p3"]
    m = rs.normal(size=(3, 3))
    other = fm.FisherMatrix(matrix=m @ m.T + 3 * np.eye(3), parameters=[ps[1], "par_new1", "par_new0"],
                            best_fits=[0.1, 0.2, 0.3], priors=[np.inf, 0.5, np.inf])
    s = a + other
    out["sum_other_matrix"] = np.asarray(other.matrix)
    out["sum_other_names"] = np.array(other.parameters)
    out["sum_other_priors"] = np.array(other.priors)
    out["sum_other_best"] = np.array(other.best_fits)
    out["sum_names"] = np.array(s.parameters)
    out["sum_matrix"] = np.asarray(s.matrix)
    out["sum_priors"] = np.array(s.priors)
    out["sum_best"] = np.array(s.best_fits)
    out["sum_covariance"] = np.asarray(s.covariance)
    # removeParameter
    a.removeParameter(ps[1])
    out["p3_removed_names"] = np.array(a.parameters)
    out["p3_removed_covariance"] = np.asarray(a.covariance)
    path = os.path.join(ROOT, "tests", "golden", "fisher_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
