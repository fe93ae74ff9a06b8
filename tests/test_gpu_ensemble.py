"""The trial-ensemble kernels on the device (csrc/ensemble.hip: `pisa_hip_metric_matrix`, `pisa_hip_metric_matrix_best`
through `kernels.metric_matrix` / `metric_matrix_best`) and pisa_amd/analysis/ensemble.py on example_hip.cfg.

The gate (tests/ensemble_cases.py): |got - exact| <= G eps sum_b (m_b + 1) per entry, G = 4 max(1, G_REF[form, kind])
with G_REF the worst ratio of the numpy restatement of the form, measured on the CPU (tests/test_host_ensemble.py).
Placement and the reduced output are compared with `==`: an entry's bits depend on its two rows alone.

The kernels' own worst ratios on an MI355X (every family and shape; `pytest -s` prints them before each assertion):
    form      llh      poisson_llh   chi2     mod_chi2
    direct    1.108    1.293         1.982    1.982       (gates 4.44  6.12  7.96  7.96)
    product   1.946    1.438         -        -           (gates 7.8   6.32)
"""
import numpy as np
import pytest

from tests import ensemble_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


def _dev(K, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(K.device())


def _matrix(K, kind, form, f, rows=None, cols=None):
    d = f["D"] if rows is None else f["D"][rows]
    e, s2 = (f["E"], f["S2"]) if cols is None else (f["E"][cols], f["S2"][cols])
    return K.metric_matrix(kind, _dev(K, d), _dev(K, e), _dev(K, s2), form=form).cpu().numpy()


def _shapes(fam):
    return ec.SHAPES if fam != "poisson" else (ec.BIG_SHAPE,)


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("fam", ec.FAMILIES)
def test_every_entry_within_the_gate_of_the_exact_value(K, fam, kind):
    """every shape and every form the kind has: all entries finite (no NaN: the dropped bins are dropped), status
    clean (a set status raises), inside the gate"""
    for form in ec.forms_of(kind):
        worst, where = 0.0, None
        for shape in _shapes(fam):
            f = ec.family(fam, *shape)
            value, scale = ec.exact(fam, kind, *shape)
            got = _matrix(K, kind, form, f)
            r = float(ec.gate_ratio(got, value, scale).max())
            if r > worst:
                worst, where = r, shape
            ec.check(got, value, scale, ec.g_of(form, kind), "%s %s %s %s" % (fam, kind, form, shape))
        print("%s %s %s: worst %.3f eps scale at %s (gate %.3g)" % (fam, kind, form, worst, where, ec.g_of(form, kind)))


@pytest.mark.parametrize("kind", ec.LLH_KINDS)
def test_auto_is_the_product_form_and_agrees_with_the_direct_one(K, kind):
    for fam in ec.FAMILIES:
        for shape in (ec.BIG_SHAPE, (17, 33, 127), (33, 16, 5)):
            f = ec.family(fam, *shape)
            _, scale = ec.exact(fam, kind, *shape)
            direct, product = _matrix(K, kind, "direct", f), _matrix(K, kind, "product", f)
            assert np.array_equal(_matrix(K, kind, "auto", f), product)
            bound = (ec.g_of("direct", kind) + ec.g_of("product", kind)) * ec.EPS * scale
            assert np.all(np.abs(product - direct) <= bound), (fam, shape, float(np.max(np.abs(product - direct) / (ec.EPS * np.maximum(scale, 1e-300)))))


@pytest.mark.parametrize("fam,kind", [("poisson", k) for k in ec.KINDS] + [("equal", "chi2"), ("asimov", "mod_chi2")])
def test_entries_are_those_of_the_one_pair_kernel(K, fam, kind):
    """each entry of a (17, 17, 130) matrix against `kernels.metric` of its pair, within the gate of the form;
    chi2's whole-map rule on the `equal` family: exactly 0 for the one equal pair, in both"""
    shape = (17, 17, 130)
    f = ec.family(fam, *shape)
    _, scale = ec.exact(fam, kind, *shape)
    d, e, s2 = _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"])
    want = np.array([[float(K.metric(kind, d[t], e[k], s2[k]).item()) for k in range(shape[1])]
                     for t in range(shape[0])])
    for form in ec.forms_of(kind):
        got = _matrix(K, kind, form, f)
        bound = ec.g_of(form, kind) * ec.EPS * scale
        print("%s %s %s: worst %.3f eps scale (gate %.3g)" % (fam, kind, form, float(np.max(np.abs(got - want) / (ec.EPS * np.maximum(scale, 1e-300)))), ec.g_of(form, kind)))
        assert np.all(np.abs(got - want) <= bound), (form, float(np.max(np.abs(got - want) / (ec.EPS * np.maximum(scale, 1e-300)))))
        if fam == "equal":
            rule = ec.chi2_rule(f["D"], f["E"])
            assert rule.sum() == 1 and rule[shape[0] // 2, shape[1] // 3]
            assert got[rule][0] == 0.0 and want[rule][0] == 0.0 and np.all(got[~rule] > 0)


@pytest.mark.parametrize("kind", ec.KINDS)
def test_placement_changes_no_bit(K, kind):
    """permuted trials and templates, and T and K split over 2 and 3 launches: the same bits, both forms"""
    fam = "sigma" if kind == "mod_chi2" else "poisson"
    T, Kt, B = ec.BIG_SHAPE
    f = ec.family(fam, T, Kt, B)
    rs = np.random.RandomState(5)
    pt, pk = rs.permutation(T), rs.permutation(Kt)
    for form in ec.forms_of(kind):
        full = _matrix(K, kind, form, f)
        assert np.array_equal(_matrix(K, kind, form, f, pt, pk), full[np.ix_(pt, pk)])
        for n in (2, 3):
            parts_t = np.array_split(np.arange(T), n)
            parts_k = np.array_split(np.arange(Kt), n)
            assert np.array_equal(np.concatenate([_matrix(K, kind, form, f, rows=r) for r in parts_t], axis=0), full)
            assert np.array_equal(np.concatenate([_matrix(K, kind, form, f, cols=c) for c in parts_k], axis=1), full)
            assert np.array_equal(_matrix(K, kind, form, f, parts_t[-1], parts_k[-1]),
                                  full[np.ix_(parts_t[-1], parts_k[-1])])


@pytest.mark.parametrize("kind", ec.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_matrix(K, kind):
    """best / first arg / column k0 bit for bit, with and without an offset, with two identical template rows (the
    smaller k wins the tie) and k0 in the last partial tile"""
    fam = "sigma" if kind == "mod_chi2" else "poisson"
    for shape in (ec.TILE_SHAPE, ec.STRIP_SHAPE, ec.BIG_SHAPE, (17, 17, 5), (1, 1, 1)):
        T, Kt, B = shape
        src = ec.family(fam, *shape)
        e, s2 = src["E"].copy(), src["S2"].copy()
        if Kt > 4:
            e[Kt - 2], s2[Kt - 2] = e[1], s2[1]          # a tie between columns 1 and Kt - 2
        f = dict(D=src["D"], E=e, S2=s2)
        d_d, d_e, d_s = _dev(K, f["D"]), _dev(K, e), _dev(K, s2)
        rs = np.random.RandomState(7)
        off = rs.randn(Kt) * 3.0
        if Kt > 4:
            off[Kt - 2] = off[1]
        for form in ec.forms_of(kind):
            full = _matrix(K, kind, form, f)
            for offset in (None, off):
                for k0 in sorted({0, Kt - 1, Kt // 2}):
                    best, arg, at = K.metric_matrix_best(kind, d_d, d_e, d_s, None if offset is None else _dev(K, offset),
                                                         k0=k0, form=form)
                    w_best, w_arg, w_at = ec.reduce_matrix(kind, full, offset, k0)
                    what = (kind, form, shape, offset is not None, k0)
                    assert np.array_equal(arg.cpu().numpy(), w_arg), what
                    assert np.array_equal(best.cpu().numpy(), w_best), what
                    assert np.array_equal(at.cpu().numpy(), w_at), what
            if Kt > 4:
                # the tie is real: forcing both columns far ahead of the rest, the smaller one is reported
                lead = off.copy()
                lead[[1, Kt - 2]] = 1e300 if kind in ec.LLH_KINDS else -1e300
                _, arg, _ = K.metric_matrix_best(kind, d_d, d_e, d_s, _dev(K, lead), k0=0, form=form)
                assert np.all(arg.cpu().numpy() == 1)


def test_status_and_argument_checks(K):
    from pisa_amd import _lib

    f = ec.family("poisson", *ec.BIG_SHAPE)
    for kind in ec.KINDS:
        for form in ec.forms_of(kind):
            for which in ("D", "E"):
                bad = dict(f)
                a = f[which].copy()
                a[3, 7] = -1.0
                bad[which] = a
                with pytest.raises(ValueError):
                    _matrix(K, kind, form, bad)
                with pytest.raises(ValueError):
                    K.metric_matrix_best(kind, _dev(K, bad["D"]), _dev(K, bad["E"]), form=form)
    d, e = _dev(K, f["D"]), _dev(K, f["E"])
    # product with a chi2 kind, bins that do not match, k0 outside the templates: INVALID, nothing launched
    for call in (lambda: K.metric_matrix("chi2", d, e, form="product"),
                 lambda: K.metric_matrix("llh", d, e[:, :100].contiguous()),
                 lambda: K.metric_matrix_best("llh", d, e, k0=e.shape[0]),
                 lambda: K.metric_matrix_best("llh", d, e, k0=-1)):
        with pytest.raises(_lib.PisaHipError) as err:
            call()
        assert err.value.status == -1
    lib = _lib.lib()
    # NULL pointers and bad sizes are refused before any device access
    assert lib.pisa_hip_metric_matrix(0, 0, None, None, None, 4, 4, 4, None, None, None) == -1
    assert lib.pisa_hip_metric_matrix(7, 0, d.data_ptr(), e.data_ptr(), None, 4, 4, 4, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.pisa_hip_metric_matrix(0, 3, d.data_ptr(), e.data_ptr(), None, 4, 4, 4, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.pisa_hip_metric_matrix(0, 0, d.data_ptr(), e.data_ptr(), None, 0, 4, 4, d.data_ptr(), d.data_ptr(), None) == -1
    assert lib.pisa_hip_metric_matrix_best(0, 0, None, None, None, None, 0, 4, 4, 4, None, None, None, None, None) == -1
    with pytest.raises(ValueError):
        K.metric_matrix("barlow_llh", d, e)
    with pytest.raises(ValueError):
        K.metric_matrix("llh", d, e, form="fast")


# ------------------------------------------------------------------ config pipeline
def _maker(free):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    return dm


@pytest.mark.parametrize("free,sweep", [(("theta23", "deltam31"), True),
                                        (("theta23", "deltam31", "delta_index"), False)])
def test_template_grid_and_feldman_cousins_on_the_config_pipeline(K, free, sweep):
    """a 3 x 3 grid over theta23 x deltam31 of example_hip.cfg: one sweep (counted through a wrapped `maps_many`), or
    point by point with delta_index free as well and moved by the grid; rows equal `get_outputs(return_sum=True)` bit for bit, the
    parameters are restored, and `feldman_cousins` (T = 64) equals the loop over `Map.fluctuate` +
    `Map.metric_total` as in the host test"""
    from pisa_amd.analysis import ensemble as en

    metric = "llh" if sweep else "mod_chi2"
    dm = _maker(free)
    th, m31 = dm.params["theta23"].value, dm.params["deltam31"].value
    axes = {"theta23": [th * 0.8, th, th * 1.15], "deltam31": [m31 * 0.85, m31, m31 * 1.2]}
    if not sweep:
        # every point away from the current delta_index: a flux stage moves, which the sweep does not take (a free
        # parameter that stays where it is does not stop it), and the Gaussian prior gives a penalty per point
        axes["delta_index"] = [0.05]
    pts = en.grid_points(dm, axes)
    assert pts.shape == (9, len(free))
    start = [p.value for p in dm.params.free]
    eng = dm.pipelines[0]["hist"]._engine
    calls = []
    orig = eng.maps_many
    eng.maps_many = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        grid = en.TemplateGrid.from_maker(dm, pts, metric)
    finally:
        del eng.maps_many
    assert len(calls) == (1 if sweep else 0) and grid.sweeps == (1 if sweep else 0)
    assert [p.value for p in dm.params.free] == start
    assert grid.hist.is_cuda and tuple(grid.hist.shape) == tuple(grid.sumw2.shape) == (9, grid.n_bins)
    maps = []
    for k in range(9):
        dm._set_rescaled_free_params(pts[k])
        out = dm.get_outputs(return_sum=True)["total"]
        assert np.array_equal(grid.host("hist")[k], out.nominal_values.ravel()), k
        assert np.array_equal(grid.host("sumw2")[k], out.variances.ravel()), k
        assert grid.penalty[k] == dm.params.priors_penalty(metric=metric)
        assert (grid.penalty[k] != 0) == (not sweep)
        maps.append(out._new(out.nominal_values.copy(), out.variances.copy()))
    assert np.array_equal(grid.hist.cpu().numpy(), grid.host("hist"))
    dm.set_free_params(start)
    assert grid.host("hist").std(axis=0).max() > 0          # the points differ

    T, cl, seed = 64, (0.6827, 0.90), 77
    crit = en.feldman_cousins(grid, metric, T, cl, seed)
    want, deltas = ec.loop_feldman_cousins(lambda m, k: m.metric_total(maps[k], metric), maps, grid.penalty, metric, T,
                                           cl, seed)
    s2 = grid.host("sumw2") if metric == "mod_chi2" else None
    scale = max(float(ec.scale_fp64(metric, en.pseudo_data(grid, k, T, np.random.RandomState([seed, k])),
                                    grid.host("hist"), s2).max()) for k in range(9))
    form = "product" if metric in ec.LLH_KINDS else "direct"
    tol = ec.g_of(form, metric) * ec.EPS * scale          # the gate's absolute size at the largest scale of the run
    print("%s: |crit - loop| worst %.3g, tol %.3g" % (metric, np.abs(crit - want).max(), tol))
    for k0 in range(9):
        for i in range(len(cl)):
            assert ec.clear_of(deltas[k0], want[k0, i], tol), (k0, i)
    assert np.all(np.abs(crit - want) <= tol), np.abs(crit - want).max()
    assert np.array_equal(en.feldman_cousins(grid, metric, T, cl, seed, true_points=[5]), crit[[5]])
    observed = maps[4].fluctuate("poisson", random_state=5)
    vals = np.array([observed.metric_total(maps[k], metric) for k in range(9)]) + grid.penalty
    delta = vals.max() - vals if metric in ec.LLH_KINDS else vals - vals.min()
    assert all(ec.clear_of([delta[k]], want[k, 1], tol) for k in range(9))
    assert np.array_equal(en.accepted(observed, grid, metric, crit[:, 1]), delta <= want[:, 1])
    # the full matrix of the analysis layer: a device tensor for device data, rows those of the loop
    data = en.pseudo_data(grid, 4, 5, 3)
    m = en.metric_matrix(K.to_device(data), grid, metric)
    assert m.is_cuda and tuple(m.shape) == (5, 9)
    assert np.array_equal(m.cpu().numpy(), en.metric_matrix(data, grid, metric).cpu().numpy())
