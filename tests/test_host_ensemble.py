"""tests/ensemble_cases.py and pisa_amd/analysis/ensemble.py without a GPU: the numpy restatements of both kernel forms
against exact values (held to G_HOST = 2), G_REF measured again and held against the recorded figures, argument checks,
the quantile rule, the order of `grid_points`, `pseudo_data` against sequential `Map.fluctuate` calls, and
`feldman_cousins` / `accepted` with the numpy solver against the reference's loop (`Map.fluctuate` + the CPU oracle's
metric in the place of `Map.metric_total`, which needs the device).

Worst ratios of the restatements, per family (every shape of ensemble_cases.SHAPES; `pytest -s` prints them):
    family    direct: llh  poisson_llh  chi2   mod_chi2   product: llh  poisson_llh
    edges             1.07   1.05       1.23   1.23                1.95   1.40
    asimov            1.11   1.53       1.98   1.98                1.78   1.58
    large             1.05   1.29       1.85   1.85                1.94   1.16
    sigma             0.89   1.03       1.42   1.52                1.77   1.29
    equal             0.77   1.30       1.80   1.80                1.01   1.14
    poisson           0.35   0.43       1.23   1.57                0.61   0.46
"""
import functools

import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import metric_cases as mc


@functools.lru_cache(maxsize=None)
def _worst(fam, kind, form):
    worst, where = 0.0, None
    for shape in (ec.SHAPES if fam != "poisson" else (ec.BIG_SHAPE,)):
        f = ec.family(fam, *shape)
        value, scale = ec.exact(fam, kind, *shape)
        got = ec.form_values(form, kind, f["D"], f["E"], f["S2"])
        assert np.all(np.isfinite(got)), (fam, kind, form, shape)
        r = float(ec.gate_ratio(got, value, scale).max())
        if r > worst:
            worst, where = r, shape
    return worst, where


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("fam", ec.FAMILIES)
def test_restatements_within_g_host_of_the_exact_values(fam, kind):
    for form in ec.forms_of(kind):
        worst, where = _worst(fam, kind, form)
        print("%s %s %s: worst %.3f at %s" % (fam, kind, form, worst, where))
        assert worst <= ec.G_HOST, (fam, kind, form, worst, where)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_g_ref_is_the_measured_worst_ratio(kind):
    """the recorded G_REF bounds the measured figure and is no more than 0.02 above it"""
    for form in ec.forms_of(kind):
        measured = max(_worst(fam, kind, form)[0] for fam in ec.FAMILIES)
        print("%s %s: measured %.4f recorded %.2f" % (form, kind, measured, ec.G_REF[(form, kind)]))
        assert measured <= ec.G_REF[(form, kind)] <= measured + 0.02
        assert ec.g_of(form, kind) == mc.KERNEL_FACTOR * max(1.0, ec.G_REF[(form, kind)])
    assert set(ec.G_REF) == {(form, k) for k in ec.KINDS for form in ec.forms_of(k)}


def test_exact_paths_agree_and_the_families_hold_what_they_promise():
    """the mpmath table and the longdouble restatement on the same integer data; the families' structure"""
    T, K, B = 17, 15, 33
    f2 = ec.family("equal", T, K, B)
    for kind in ec.KINDS:
        ints = np.array([t for t in range(T) if t != T // 2])           # the integer data rows
        ve, se = ec.exact("equal", kind, T, K, B)
        vl, sl = ec.exact_longdouble(kind, f2["D"][ints], f2["E"], f2["S2"])
        assert np.all(np.abs((ve[ints] - vl).astype(np.float64)) <= 0.01 * ec.EPS * se[ints]), kind
        np.testing.assert_allclose(sl, se[ints], rtol=1e-12)
    e = ec.family("edges", 17, 16, 130)
    assert np.all(e["D"][1::5] == 0) and np.all(e["D"][:, 2::4] == 0)
    assert tuple(e["E"][0, :7]) == ec.CLIPPED and e["D"].max() == 2.0 ** 30 and {1.0, 2.0, 170.0, 171.0} <= set(e["D"].ravel())
    a = ec.family("asimov", 33, 16, 5)
    assert not np.array_equal(a["D"], np.rint(a["D"]))
    ratio = a["D"] / a["E"][np.arange(33) % 16] - 1
    assert np.allclose(np.abs(ratio).min(axis=1).min(), 1e-9, rtol=1e-6) and np.abs(ratio).max() < 0.1 + 1e-12
    assert ec.family("large", 16, 16, 128)["D"].max() == 1e9
    s = ec.family("sigma", 16, 16, 128)
    assert s["S2"].min() == 0 and np.isclose((s["S2"] / s["E"]).max(), 1e6)
    q = ec.family("equal", 17, 17, 130)
    rule = ec.chi2_rule(q["D"], q["E"])
    assert rule.sum() == 1 and rule[8, 5]
    for name in ec.PALETTE_FAMILIES:
        pd, pe, _ = ec.palettes(name)
        assert pd.size * pe.size <= 20000
    # chi2's rule reaches the restatement and the exact value: exactly 0 for the equal pair only
    assert ec.direct_form("chi2", q["D"], q["E"])[8, 5] == 0.0 and ec.exact("equal", "chi2", 17, 17, 130)[0][8, 5] == 0
    assert ec.direct_form("mod_chi2", q["D"], q["E"])[8, 5] == 0.0      # (d - mu = 0 in every bin; no rule needed)
    # llh without data in any bin: every bin dropped, exactly 0 in both forms
    z = ec.family("edges", 17, 16, 130)
    for form in ec.FORMS:
        assert np.all(ec.form_values(form, "llh", z["D"], z["E"])[1::5] == 0.0)


def test_reduce_matrix_and_the_numpy_solver():
    m = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 1.0, 5.0]])
    best, arg, at = ec.reduce_matrix("llh", m, None, 3)
    assert list(best) == [3.0, 5.0] and list(arg) == [1, 0] and list(at) == [2.0, 5.0]
    best, arg, at = ec.reduce_matrix("chi2", m, np.array([0.0, 0.0, -1.0, 0.0]), 0)
    assert list(best) == [1.0, 0.0] and list(arg) == [0, 2] and list(at) == [1.0, 5.0]
    f = ec.family("poisson", *ec.BIG_SHAPE)
    s = ec.NumpySolver()
    assert np.array_equal(s.matrix("chi2", f["D"], f["E"]), ec.direct_form("chi2", f["D"], f["E"]))
    assert np.array_equal(s.best("llh", f["D"], f["E"], None, None, 4)[2], ec.direct_form("llh", f["D"], f["E"])[:, 4])
    assert np.array_equal(ec.NumpySolver("product").matrix("llh", f["D"], f["E"]), ec.product_form("llh", f["D"], f["E"]))


def test_argument_checks():
    import torch

    from pisa_amd import kernels as K
    from pisa_amd.analysis import ensemble as en

    d, e = torch.zeros((3, 4), dtype=torch.float64), torch.ones((2, 4), dtype=torch.float64)
    for call in (lambda: K.metric_matrix("barlow_llh", d, e), lambda: K.metric_matrix("llh", d, e, form="fast"),
                 lambda: K.metric_matrix("llh", d[0], e), lambda: K.metric_matrix("llh", d.float(), e),
                 lambda: K.metric_matrix("mod_chi2", d, e, sigma2=e[:1]),
                 lambda: K.metric_matrix_best("llh", d, e, offset=torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()
    hist, sumw2, points, penalty = ec.toy_grid("llh")
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, "llh")
    assert len(grid) == 9 and grid.n_bins == hist.shape[1] and grid.sigma2_for("llh") is None
    assert grid.sigma2_for("mod_chi2") is sumw2
    s = ec.NumpySolver()
    with pytest.raises(ValueError):
        en.TemplateGrid(hist, sumw2[:, :3], points)
    with pytest.raises(ValueError):
        en.TemplateGrid(hist, sumw2, points[:4])
    with pytest.raises(ValueError):
        en.delta_metric(hist[:2], grid, "barlow_llh", 0, s)
    with pytest.raises(ValueError):
        en.delta_metric(hist[:2], grid, "llh", 9, s)
    with pytest.raises(ValueError):
        en.feldman_cousins(grid, "llh", 0, solver=s)
    with pytest.raises(ValueError):
        en.feldman_cousins(grid, "llh", 4, true_points=[9], solver=s)
    with pytest.raises(ValueError):
        en.feldman_cousins(grid, "llh", 4, true_points=[0, 9], solver=s)      # refused before the first point is drawn
    for seed in (-1, 2 ** 32):
        with pytest.raises(ValueError):
            en.feldman_cousins(grid, "llh", 4, random_state=seed, solver=s)
    with pytest.raises(ValueError):
        en.accepted(hist[0], grid, "llh", np.zeros(8), s)
    with pytest.raises(ValueError):
        en.accepted(hist[:2], grid, "llh", np.zeros(9), s)
    with pytest.raises(ValueError):
        en.critical_values([], 0.9)
    with pytest.raises(ValueError):
        en.critical_values([1.0], 0.0)
    assert not s.calls                        # every refusal came before the evaluator was asked


def test_the_quantile_rule():
    from pisa_amd.analysis.ensemble import critical_values

    d = np.random.RandomState(1).permutation(np.arange(1.0, 65.0))       # 1 .. 64
    assert list(critical_values(d, (0.6827, 0.90, 1.0, 1e-9, 0.5))) == [44.0, 58.0, 64.0, 1.0, 32.0]
    assert list(critical_values(np.arange(10.0), 0.9)) == [8.0]          # ceil(9) - 1: no interpolation towards 9
    assert list(critical_values([3.0], (0.1, 0.99))) == [3.0, 3.0]


class _Maker:
    def __init__(self, params):
        self.params = params


def test_grid_points_order_and_rescaling():
    from pisa_amd.analysis.ensemble import grid_points
    from pisa_amd.core.param import Param, ParamSet
    from pisa_amd.core.units import ureg

    a = Param("a", 1.5 * ureg.GeV, prior=None, range=[0.5, 3] * ureg.GeV, is_fixed=False)
    b = Param("b", 20 * ureg.deg, prior=None, range=[0, 90] * ureg.deg, is_fixed=False)
    c = Param("c", 0.3, prior=None, range=[-1, 1], is_fixed=True)
    d = Param("d", 0.25, prior=None, range=[0, 1], is_fixed=False)
    maker = _Maker(ParamSet(a, b, c, d))
    assert list(maker.params.free.names) == ["a", "b", "d"]
    pts = grid_points(maker, {"d": [0.0, 0.5, 1.0], "a": [500 * ureg.MeV, 3 * ureg.GeV]})
    assert pts.shape == (6, 3)
    # the last name (a) runs fastest; b, not named, stays at its current value 20 / 90
    assert np.array_equal(pts[:, 2], [0.0, 0.0, 0.5, 0.5, 1.0, 1.0])
    assert np.array_equal(pts[:, 0], [0.0, 1.0] * 3)
    assert np.allclose(pts[:, 1], 20.0 / 90.0, rtol=1e-15)
    assert a.value == 1.5 * ureg.GeV and d.value.magnitude == 0.25      # nothing moved
    one = grid_points(maker, {"b": np.array([0.0, 45.0, 90.0]) * ureg.deg})
    assert np.allclose(one[:, 1], [0.0, 0.5, 1.0]) and np.allclose(one[:, 0], 0.4) and np.allclose(one[:, 2], 0.25)
    assert grid_points(maker, {}).shape == (1, 3)
    for bad in ({"c": [0.1]}, {"nope": [1.0]}, {"d": [2.0]}, {"d": []}):
        with pytest.raises(ValueError):
            grid_points(maker, bad)


def _template_maps(hist, sumw2):
    from pisa_amd.core.map import Map

    binning = [dict(name="x", bin_edges=np.linspace(0.0, 1.0, hist.shape[1] // 4 + 1)),
               dict(name="y", bin_edges=np.linspace(0.0, 1.0, 5))]
    shape = (hist.shape[1] // 4, 4)
    return [Map(name="total", hist=h.reshape(shape), binning=binning, error_hist=np.sqrt(v).reshape(shape))
            for h, v in zip(hist, sumw2)]


def test_pseudo_data_is_the_sequence_of_map_fluctuate_calls():
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid("llh")
    hist = hist.copy()
    hist[4, 5] = np.nan                     # a NaN bin draws nothing and stays NaN
    hist[4, 6] = 0.0
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, "llh")
    maps = _template_maps(hist, sumw2)
    for k, seed in ((4, 3), (0, 12345)):
        got = en.pseudo_data(grid, k, 37, seed)
        rs = np.random.RandomState(seed)
        want = np.stack([maps[k].fluctuate("poisson", random_state=rs).nominal_values.ravel() for _ in range(37)])
        assert got.shape == (37, hist.shape[1]) and np.array_equal(got, want, equal_nan=True)
    rs = np.random.RandomState(8)           # a RandomState is used, and advanced, as it is
    first, second = en.pseudo_data(grid, 1, 5, rs), en.pseudo_data(grid, 1, 5, rs)
    assert np.array_equal(np.concatenate([first, second]), en.pseudo_data(grid, 1, 10, 8))


@pytest.mark.parametrize("metric", ec.KINDS)
def test_feldman_cousins_and_accepted_equal_the_reference_loop(oracle, metric):
    """3 x 3 grid, T = 64, the numpy solver: crit within the gate's absolute size of the loop's, `accepted` identical;
    the seeds keep every delta_metric 10 gates away from a critical value it is compared with (checked here)"""
    from pisa_amd.analysis import ensemble as en

    hist, sumw2, points, penalty = ec.toy_grid(metric)
    grid = en.TemplateGrid(hist, sumw2, points, None, penalty, metric)
    maps = _template_maps(hist, sumw2)
    s2 = sumw2 if metric == "mod_chi2" else None

    def metric_total(data_map, k):
        return oracle.metric(metric, data_map.nominal_values.ravel(), hist[k], None if s2 is None else s2[k])[1]

    T, cl, seed = 64, (0.6827, 0.90), 2024
    solver = ec.NumpySolver()
    crit = en.feldman_cousins(grid, metric, T, cl, seed, solver=solver)
    want, deltas = ec.loop_feldman_cousins(metric_total, maps, penalty, metric, T, cl, seed)
    assert crit.shape == (9, 2) and [c[0] for c in solver.calls] == ["best"] * 9
    scale = max(float(ec.scale_fp64(metric, en.pseudo_data(grid, k, T, np.random.RandomState([seed, k])), hist, s2).max())
                for k in range(9))
    tol = ec.g_of("direct", metric) * ec.EPS * scale      # the gate's absolute size at the largest scale of the run
    print("%s: |crit - loop| worst %.3g, tol %.3g" % (metric, np.abs(crit - want).max(), tol))
    assert tol < 1e-9
    for k0 in range(9):
        for i in range(len(cl)):
            assert ec.clear_of(deltas[k0], want[k0, i], tol), (k0, i)
    assert np.all(np.abs(crit - want) <= tol), np.abs(crit - want).max()
    assert np.all(crit >= 0) and np.all(crit[:, 1] >= crit[:, 0])
    # a subset of true points reproduces the full run's rows; a RandomState stands for the seed it gives
    sub = en.feldman_cousins(grid, metric, T, cl, seed, true_points=[7, 2], solver=solver)
    assert np.array_equal(sub, crit[[7, 2]])
    drawn = int(np.random.RandomState(5).randint(0, 2 ** 31 - 1))
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, np.random.RandomState(5), true_points=[3], solver=solver),
                          en.feldman_cousins(grid, metric, T, cl, drawn, true_points=[3], solver=solver))
    # the observed map: accepted point by point as the loop says
    observed = maps[4].fluctuate("poisson", random_state=99)
    got = en.accepted(observed, grid, metric, crit[:, 1], solver)
    vals = np.array([metric_total(observed, k) for k in range(9)]) + penalty
    delta = vals.max() - vals if metric in ec.LLH_KINDS else vals - vals.min()
    assert all(ec.clear_of([delta[k]], want[k, 1], tol) for k in range(9))
    assert got.dtype == bool and np.array_equal(got, delta <= want[:, 1])
    assert got.any() and got[4]
    d1 = en.delta_metric(observed, grid, metric, 4, solver)
    assert d1.shape == (1,) and abs(d1[0] - delta[4]) <= tol and d1[0] >= 0
