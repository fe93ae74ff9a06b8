"""tests/ensemble_mc_cases.py and the MC-uncertainty metrics in pisa_amd/analysis/ensemble.py without a GPU: the
palettes' flags in the exact oracle, the numpy restatement of csrc/ensemble_mc.hip against exact values (G_REF measured
again and held against the recorded figures), the restatement at one bin against the CPU oracle's per-bin value,
`metric_matrix`, `delta_metric`, `feldman_cousins` and `accepted` with a numpy solver built on the restatement, and
the refusals.

Worst ratios of the restatement (every shape of the kind; `pytest -s` prints them):
    correct_chi2 1.954 at (1000, 40, 8)   mcllh_mean 0.937 at (15, 16, 3)   mcllh_eff 1.424 at (15, 33, 1)
    conv_llh 1.031 at (33, 15, 3)
"""
import functools

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import ensemble_mc_cases as emc
from tests import metric_cases as mc


@functools.lru_cache(maxsize=None)
def _worst(kind):
    fam = emc.family_of(kind)
    worst, where = 0.0, None
    for shape in emc.shapes_of(kind):
        f = emc.family(fam, *shape)
        value, scale = emc.exact(fam, kind, *shape)
        got = emc.direct_form_mc(kind, f["D"], f["E"], f["S2"])
        assert np.all(np.isfinite(got)), (kind, shape)
        r = float(ec.gate_ratio(got, value, scale).max())
        if r > worst:
            worst, where = r, shape
    return worst, where


def test_palettes_and_families_hold_what_they_promise():
    pd, pe, ps2 = emc.palettes("mc_sigma")
    assert pd.size * pe.size == 945 and tuple(pe[:5]) == emc.CLIPPED and tuple(ps2[:5]) == emc.CLIPPED_S2
    assert np.isclose((ps2[5:] / pe[5:]).max(), 1e3) and ps2.min() == 0 and {0.0, 1.0, 2.0, 170.0, 171.0} <= set(pd)
    pd, pe, ps2 = emc.palettes("mc_conv")
    assert pd.size * pe.size == 432 and tuple(pd) == emc.CONV_DATA
    assert sorted(set(pe)) == sorted({0.5, 0.0, 1.3, 1.0, 1.25, 2.5, 3.25, 20.0, 40.0, 52.0})
    sigma = np.sqrt(ps2)
    assert np.array_equal(sigma, sigma.astype(np.float32).astype(np.float64)) and np.array_equal(sigma * sigma, ps2)
    for kind in emc.KINDS:
        fam = emc.family_of(kind)
        hi, lo, m, flag = emc.exact_table(fam, kind)
        assert np.all(flag == mc.FLAG_VALUE) and np.all(np.isfinite(hi)) and np.all(np.isfinite(m)), kind
    for name, shape in (("mc_sigma", (17, 16, 130)), ("mc_conv", (17, 16, 5))):
        f = emc.family(name, *shape)
        _, pe, ps2 = emc.palettes(name)
        assert np.all(f["D"][1::5] == 0) and f["D"][0].max() > 0
        n = min(shape[2], pe.size)
        assert np.array_equal(f["E"][0, :n], pe[:n]) and np.array_equal(f["S2"][0, :n], ps2[:n])
    p = emc.family("mc_poisson", *emc.BIG_SHAPE)
    assert np.array_equal(p["D"], np.rint(p["D"])) and p["E"].min() >= 1e-2 and p["E"].max() <= 1e3 and p["S2"].min() >= 0


@pytest.mark.parametrize("kind", emc.KINDS)
def test_g_ref_is_the_measured_worst_ratio(kind):
    """the restatement is within G_HOST of the exact values; the recorded G_REF bounds the measured figure and is no
    more than 0.02 above it"""
    measured, where = _worst(kind)
    print("%s: measured %.4f at %s, recorded %.2f" % (kind, measured, where, emc.G_REF[kind]))
    assert measured <= emc.G_HOST
    assert measured <= emc.G_REF[kind] <= measured + 0.02
    assert emc.g_of(kind) == mc.KERNEL_FACTOR * max(1.0, emc.G_REF[kind])
    assert set(emc.G_REF) == set(emc.KINDS)


@pytest.mark.parametrize("kind", emc.KINDS)
def test_one_bin_of_the_restatement_is_the_oracles_per_bin_value(kind):
    """B = 1 over the whole palette: the restatement (hoisted, the identity for conv_llh's second term) against
    `stages_oracle.metric_wide`, the formula as written, within the two host gates added"""
    from oracle import stages_oracle as so

    fam = emc.family_of(kind)
    pd, pe, ps2 = emc.palettes(fam)
    _, _, m, _ = emc.exact_table(fam, kind)
    got = emc.direct_form_mc(kind, pd[:, None], pe[:, None], ps2[:, None])
    with np.errstate(all="ignore"):
        want = np.asarray(so.metric_wide(kind, np.repeat(pd, pe.size), np.tile(pe, pd.size),
                                         np.tile(np.sqrt(ps2), pd.size)), dtype=np.float64).reshape(got.shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    r = np.abs(got - want) / (emc.EPS * (m + 1.0))
    print("%s: worst %.3f eps (m + 1)" % (kind, r.max()))
    assert r.max() <= 2 * emc.G_HOST, (kind, float(r.max()), np.unravel_index(int(np.argmax(r)), r.shape))
    # the scale without a table is the table's (a part in 1e6 is nothing to a gate's scale; conv_llh's nodes, rounded in
    # fp64, move |k ln f_x| by up to 4e-7 of m where an f_x is within rounding of 0)
    np.testing.assert_allclose(emc.scale_mc(kind, pd[:, None], pe[:, None], ps2[:, None]), m + 1.0, rtol=1e-6)


def test_the_solver_and_the_reduction():
    f = emc.family("mc_poisson", 17, 16, 5)
    s = emc.NumpySolverMC()
    for kind in emc.KINDS:
        full = emc.direct_form_mc(kind, f["D"], f["E"], f["S2"])
        assert np.array_equal(s.matrix(kind, f["D"], f["E"], f["S2"]), full)
        best, arg, at = s.best(kind, f["D"], f["E"], f["S2"], None, 4)
        assert np.array_equal(at, full[:, 4])
        want = full.min(axis=1) if kind == "correct_chi2" else full.max(axis=1)
        assert np.array_equal(best, want) and np.array_equal(full[np.arange(17), arg], want)


@pytest.mark.parametrize("metric", emc.KINDS)
def test_ensemble_module_end_to_end_on_the_numpy_solver(metric):
    """3 x 3 toy grid with sumw2 = 0.3 hist: `metric_matrix`, `delta_metric >= 0`, `feldman_cousins` equal to the loop
    over `pseudo_data` + `delta_metric`, `accepted`"""
    from pisa_amd.analysis import ensemble as en

    assert metric in en.METRICS
    hist, sumw2, points, penalty = ec.toy_grid("chi2" if metric == "correct_chi2" else "llh")
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, metric)
    assert grid.sigma2_for(metric) is sumw2 and grid.sigma2_for("llh") is None and grid.sigma2_for("mod_chi2") is sumw2
    solver = emc.NumpySolverMC()
    T, cl, seed = 16, (0.6827, 0.90), 2024
    data = en.pseudo_data(grid, 4, T, np.random.RandomState(3))
    m = en.metric_matrix(data, grid, metric, solver=solver)
    assert np.array_equal(m, emc.direct_form_mc(metric, data, hist, sumw2) + penalty[None, :])
    assert np.array_equal(en.metric_matrix(data, grid, metric, with_penalty=False, solver=solver),
                          emc.direct_form_mc(metric, data, hist, sumw2))
    for k0 in (0, 4, 8):
        delta = en.delta_metric(data, grid, metric, k0, solver)
        want = m.min(axis=1) if metric == "correct_chi2" else m.max(axis=1)
        assert np.all(delta >= 0)
        assert np.array_equal(delta, m[:, k0] - want if metric == "correct_chi2" else want - m[:, k0])
    points_fc = [0, 4, 7]
    crit = en.feldman_cousins(grid, metric, T, cl, seed, true_points=points_fc, solver=solver)
    want = np.array([en.critical_values(en.delta_metric(
        en.pseudo_data(grid, k0, T, np.random.RandomState([seed, k0])), grid, metric, k0, solver), cl)
        for k0 in points_fc])
    assert crit.shape == (3, 2) and np.array_equal(crit, want)
    assert np.all(crit >= 0) and np.all(crit[:, 1] >= crit[:, 0])
    crit_all = np.full(9, crit[:, 1].max())
    observed = en.pseudo_data(grid, 4, 1, np.random.RandomState(99))
    got = en.accepted(observed[0], grid, metric, crit_all, solver)
    row = en.metric_matrix(observed, grid, metric, solver=solver)[0]
    delta = row - row.min() if metric == "correct_chi2" else row.max() - row
    assert got.dtype == bool and np.array_equal(got, delta <= crit_all) and got.any()


def test_refusals():
    import torch

    from pisa_amd import kernels as K
    from pisa_amd.analysis import ensemble as en

    assert tuple(K.METRIC_KIND) == ("llh", "poisson_llh", "chi2", "mod_chi2")
    assert K.ENSEMBLE_MC_KINDS == emc.KINDS and all(k in K.MAP_METRIC_KIND for k in emc.KINDS)
    d, e = torch.zeros((3, 4), dtype=torch.float64), torch.ones((2, 4), dtype=torch.float64)
    r = torch.ones((2, 1, 4), dtype=torch.float64)
    for kind in emc.KINDS:
        for call in (lambda: K.metric_matrix(kind, d, e, e, form="product"),
                     lambda: K.metric_matrix(kind, d, e, None),
                     lambda: K.metric_matrix(kind, d, e, e, form="fast"),
                     lambda: K.metric_matrix_best(kind, d, e, e, form="product"),
                     lambda: K.metric_matrix_best(kind, d, e, None),
                     lambda: K.metric_matrix(kind, d, e, e[:1]),
                     lambda: K.profiled_metric_matrix(kind, d, e, r, e),
                     lambda: K.profiled_metric_matrix_best(kind, d, e, r, e)):
            with pytest.raises(ValueError):
                call()
    for kind in ("barlow_llh", "signed_sqrt_mod_chi2", "generalized_poisson_llh"):
        with pytest.raises(ValueError):
            K.metric_matrix(kind, d, e, e)
        with pytest.raises(ValueError):
            K.metric_matrix_best(kind, d, e, e)
    hist, sumw2, points, penalty = ec.toy_grid("llh")
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, "mcllh_eff")

    class Profiling(emc.NumpySolverMC):
        def profiled_matrix(self, *a, **k):
            raise AssertionError("asked")

        profiled_best = profiled_matrix

    s = Profiling()
    resp = en.NuisanceResponse(["x"], np.ones((9, 1, hist.shape[1])))
    for metric in emc.KINDS:
        with pytest.raises(ValueError):
            en.metric_matrix(hist[:2], grid, metric, solver=s, response=resp)
        with pytest.raises(ValueError):
            en.delta_metric(hist[:2], grid, metric, 0, s, resp)
        with pytest.raises(ValueError):
            en.feldman_cousins(grid, metric, 4, random_state=1, solver=s, response=resp)
        with pytest.raises(ValueError):
            en.accepted(hist[0], grid, metric, np.zeros(9), s, resp)
    for metric in ("barlow_llh", "signed_sqrt_mod_chi2"):
        assert metric not in en.METRICS
        with pytest.raises(ValueError):
            en.metric_matrix(hist[:2], grid, metric, solver=s)
        with pytest.raises(ValueError):
            en.delta_metric(hist[:2], grid, metric, 0, s)
        with pytest.raises(ValueError):
            en.feldman_cousins(grid, metric, 4, solver=s)
    assert not s.calls                        # every refusal came before the evaluator was asked
