"""The Fisher matrix class and the host parts of the pull method (pisa_amd/utils/fisher_matrix.py,
pisa_amd/utils/pull_method.py) against the reference's own results (tests/golden/fisher_ref.npz, written by
scripts/dev/gen_fisher_golden.py), the save / load round trip, the documented deviations and the argument checks of
`pisa_hip_fisher`, which come before any device access."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from pisa_amd.core.units import ureg
from pisa_amd.utils import pull_method as pm
from pisa_amd.utils.fisher_matrix import FisherMatrix

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fisher_ref.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def _fm(g, key="p3", priors=None):
    return FisherMatrix(matrix=g[key + "_matrix"], parameters=list(g[key + "_sorted"]),
                        best_fits=list(g[key + "_best"]), priors=priors)


def close(a, b):
    np.testing.assert_allclose(np.asarray(a, dtype=float), np.asarray(b, dtype=float), rtol=1e-12, atol=0)


def test_derivative_map_is_the_references(g):
    for key in ("p1", "p3", "p8", "big"):
        pts, vals = g[key + "_points"], g[key + "_vals"]
        for p in range(len(vals)):
            hi, lo = vals[p]
            # keyed by magnitudes (this build's Quantity is unhashable)
            got = pm.get_derivative_map({float(hi): pts[1 + 2 * p], float(lo): pts[2 + 2 * p]})
            assert np.array_equal(got, g[key + "_grads"][p])


def test_derivative_from_polycoefficients():
    assert pm.derivative_from_polycoefficients([5.0, 2.0, 3.0, -1.0], 2.0) == 2.0 + 2 * 3.0 * 2.0 - 3 * 4.0


def test_methods_match_the_reference(g):
    for key in ("p1", "p3", "p8", "big"):
        close(_fm(g, key).covariance, g[key + "_covariance"])
    f = _fm(g)
    ps = f.parameters
    for tag in ("free", "prior"):
        if tag == "prior":
            f.setPrior(ps[0], 0.05)
            f.addPrior(ps[1], 0.2)
            f.addPrior(ps[1], 0.3)
            close(f.priors, g["p3_prior_values"])
        close(f.covariance, g["p3_%s_covariance" % tag])
        close([f.getSigma(p) for p in ps], g["p3_%s_sigma" % tag])
        close([f.getSigmaNoPriors(p) for p in ps], g["p3_%s_sigma_nopriors" % tag])
        close([f.getSigmaStatistical(p) for p in ps], g["p3_%s_sigma_stat" % tag])
        close([f.getSigmaSystematic(p) for p in ps], g["p3_%s_sigma_syst" % tag])
        close([[f.getCorrelation(a, b) for b in ps] for a in ps], g["p3_%s_correlation" % tag])
        close([f.getErrorEllipse(ps[0], ps[1]), f.getErrorEllipse(ps[2], ps[0], 0.9)], g["p3_%s_ellipse" % tag])
    f.removeAllPriors()
    assert f.priors == [np.inf] * 3
    f.removeParameter(ps[1])
    assert f.parameters == list(g["p3_removed_names"])
    close(f.covariance, g["p3_removed_covariance"])


def test_sum_matches_the_reference_and_orders_self_first(g):
    a = _fm(g)
    other = FisherMatrix(matrix=g["sum_other_matrix"], parameters=list(g["sum_other_names"]),
                         best_fits=list(g["sum_other_best"]), priors=list(g["sum_other_priors"]))
    s = a + other
    # deviation: self's parameters, then other's new ones (the reference's order follows a set)
    assert s.parameters == list(a.parameters) + [p for p in other.parameters if p not in a.parameters]
    ref = list(g["sum_names"])
    idx = [ref.index(p) for p in s.parameters]
    close(s.matrix, g["sum_matrix"][np.ix_(idx, idx)])
    close(s.covariance, g["sum_covariance"][np.ix_(idx, idx)])
    close(s.priors, g["sum_priors"][idx])
    assert s.best_fits == [g["sum_best"][i] for i in idx]


def test_save_load_round_trip(g, tmp_path):
    f = _fm(g, priors=[0.1, None, np.inf])
    f.setLabel(f.parameters[0], "first")
    fn = str(tmp_path / "fisher.json")
    f.saveFile(fn)
    h = FisherMatrix.fromFile(fn)
    assert h.parameters == f.parameters and h.labels == f.labels and h.priors == f.priors
    assert np.array_equal(np.asarray(h.matrix), np.asarray(f.matrix))
    assert np.array_equal(np.asarray(h.covariance), np.asarray(f.covariance))
    assert h.best_fits == f.best_fits


def test_consistency_checks_and_errors(g):
    f = _fm(g)
    with pytest.raises(IndexError):
        f.getParameterIndex("nope")
    with pytest.raises(ValueError, match="singular"):
        FisherMatrix(matrix=np.zeros((2, 2)), parameters=["a", "b"], best_fits=[0, 0])
    with pytest.raises(ValueError, match="symmetric"):
        FisherMatrix(matrix=[[1.0, 2.0], [0.0, 1.0]], parameters=["a", "b"], best_fits=[0, 0])
    with pytest.raises(ValueError, match="unique"):
        FisherMatrix(matrix=np.eye(2), parameters=["a", "a"], best_fits=[0, 0])
    with pytest.raises(IndexError):
        FisherMatrix(matrix=np.eye(2), parameters=["a"], best_fits=[0])
    with pytest.raises(TypeError):
        FisherMatrix.translatePrior(types.SimpleNamespace(kind="spline"))
    assert FisherMatrix.translatePrior(types.SimpleNamespace(kind="gaussian", sigma=0.3)) == 0.3
    assert FisherMatrix.translatePrior(types.SimpleNamespace(kind="uniform")) == np.inf


def test_rename_checks_the_list(g):
    f = _fm(g)
    a, b, _ = f.parameters
    f.renameParameter(a, "renamed")
    assert f.parameters[0] == "renamed"
    with pytest.raises(ValueError):
        f.renameParameter("renamed", b)
    f.renameParameter("renamed", "renamed")       # its own name is not a clash


def test_papa_file_is_not_ported():
    assert not hasattr(FisherMatrix, "fromPaPAFile")


def test_sort_by_param(g):
    f = _fm(g)
    p = f.parameters[1]
    out = f.sortByParam(p)
    assert out[0][0] == p and abs(out[0][1] - 100.0) < 1e-9
    assert [v for _, v in out] == sorted([v for _, v in out], reverse=True)


def test_print_results(g, tmp_path, capsys):
    f = _fm(g, priors=[0.1, None, None])
    f.printResults()
    f.printResultsSorted(f.parameters[0], latex=True)
    text = capsys.readouterr().out
    assert "free" in text and "\\toprule" in text
    fn = str(tmp_path / "r.txt")
    f.printResultsSorted(f.parameters[0], file=fn)
    assert "impact" in open(fn).read()


def test_test_values_must_be_two_distinct():
    q = lambda v: ureg.Quantity(v, "dimensionless")  # noqa: E731
    with pytest.raises(ValueError):
        pm._sorted_pair([q(1.0), q(2.0), q(3.0)])
    with pytest.raises(ValueError):
        pm._sorted_pair([q(1.0), q(1.0)])
    with pytest.raises(ValueError):
        pm.get_derivative_map({1.0: np.zeros(3)})
    assert pm._sorted_pair([q(2.0), q(1.0)])[0].magnitude == 1.0


def test_varbinning_outputs_raise():
    from pisa_amd.core.distribution_maker import DistributionMaker

    q = ureg.Quantity(1.0, "dimensionless")
    par = types.SimpleNamespace(value=q)
    maker = types.SimpleNamespace(params={"x": par}, label=None,
                                  _pipelines=[types.SimpleNamespace(fast_path=False, output_binning=None)],
                                  get_outputs=lambda return_sum=False: [object()])
    with pytest.raises(NotImplementedError):
        DistributionMaker._fisher_templates(maker, ["x"], {"x": [q * 0.9, q * 1.1]})


def test_c_abi_rejects_bad_arguments():
    from pisa_amd import _lib

    lib = _lib.lib()
    assert _lib.FISHER_MAX_PARAMS == 32
    buf = C.c_void_p(16)      # never dereferenced: the checks come first

    def call(n_points=5, n_par=2, lo=(1, 3), hi=(2, 4), dx=(0.5, 0.25), n_bins=128, n_rows=1, pull=False):
        a_lo = (C.c_int32 * max(len(lo), 1))(*lo)
        a_hi = (C.c_int32 * max(len(hi), 1))(*hi)
        a_dx = (C.c_double * max(len(dx), 1))(*dx)
        return lib.pisa_hip_fisher(buf, buf, n_points, n_rows, n_bins, n_par, a_lo, a_hi, a_dx,
                                   buf if pull else None, buf, buf, buf if pull else None, None, None, buf, buf, None)

    bad = [dict(lo=(1, 5)), dict(hi=(2, -1)), dict(dx=(0.0, 1.0)), dict(dx=(np.inf, 1.0)), dict(dx=(1.0, np.nan)),
           dict(n_par=0), dict(n_par=33, lo=(0,) * 33, hi=(1,) * 33, dx=(1.0,) * 33), dict(n_bins=0),
           dict(n_bins=1 << 31), dict(n_rows=0), dict(n_points=0), dict(n_rows=1 << 30, n_points=1 << 30)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert lib.pisa_hip_fisher(buf, buf, 5, 1, 128, 2, (C.c_int32 * 2)(1, 3), (C.c_int32 * 2)(2, 4),
                               (C.c_double * 2)(1.0, 1.0), buf, buf, buf, None, None, None, buf, buf, None) == -1
