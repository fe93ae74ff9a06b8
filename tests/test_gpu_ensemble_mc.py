"""The MC-uncertainty metrics of the trial-ensemble matrix on the device (csrc/ensemble_mc.hip:
`pisa_hip_metric_matrix_mc`, `pisa_hip_metric_matrix_mc_best` through `kernels.metric_matrix` / `metric_matrix_best`)
and pisa_amd/analysis/ensemble.py with them on example_hip.cfg.

The gate (tests/ensemble_mc_cases.py): |got - exact| <= G eps sum_b (m_b + 1) per entry, G = 4 max(1, G_REF[kind]) with
G_REF the worst ratio of the numpy restatement of the kernels, measured on the CPU (tests/test_host_ensemble_mc.py).
Placement and the reduced output are compared with `==`: an entry's bits depend on its two rows alone.

The kernels' own worst ratios on an MI355X (every shape of the kind; `pytest -s` prints them before each assertion):
    correct_chi2   mcllh_mean   mcllh_eff   conv_llh
    1.954          0.917        1.424       1.031       (gates 7.84  4  5.72  4.16)
On example_hip.cfg `ensemble.metric_matrix` against `Map.metric_total`: 0.479 / 0.028 / 0.027 / 0.011 eps scale.
"""
import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import ensemble_mc_cases as emc
from tests import metric_cases as mc

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


def _matrix(K, kind, f, rows=None, cols=None):
    d = f["D"] if rows is None else f["D"][rows]
    e, s2 = (f["E"], f["S2"]) if cols is None else (f["E"][cols], f["S2"][cols])
    return K.metric_matrix(kind, _dev(K, d), _dev(K, e), _dev(K, s2)).cpu().numpy()


@pytest.mark.parametrize("kind", emc.KINDS)
def test_every_entry_within_the_gate_of_the_exact_value(K, kind):
    """every shape of the kind's family: all entries finite, status clean (a set status raises), inside the gate;
    form "direct" is form "auto" """
    fam = emc.family_of(kind)
    worst, where = 0.0, None
    for shape in emc.shapes_of(kind):
        f = emc.family(fam, *shape)
        value, scale = emc.exact(fam, kind, *shape)
        got = _matrix(K, kind, f)
        r = float(ec.gate_ratio(got, value, scale).max())
        if r > worst:
            worst, where = r, shape
        print("%s %s: %.3f eps scale" % (kind, shape, r))
        ec.check(got, value, scale, emc.g_of(kind), "%s %s %s" % (fam, kind, shape))
    print("%s %s: worst %.3f eps scale at %s (gate %.3g)" % (fam, kind, worst, where, emc.g_of(kind)))
    f = emc.family(fam, *emc.shapes_of(kind)[-1])
    d, e, s2 = _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"])
    assert np.array_equal(K.metric_matrix(kind, d, e, s2, form="direct").cpu().numpy(), _matrix(K, kind, f))


def _placement_family(kind, fam):
    # conv_llh costs 101 steps per bin: both families at the largest of its own shapes
    T, Kt, B = emc.CONV_SHAPES[-1] if kind == "conv_llh" else emc.BIG_SHAPE
    return emc.family(fam, T, Kt, B), (T, Kt, B)


@pytest.mark.parametrize("fam", ("mc_poisson", "mc_sigma"))
@pytest.mark.parametrize("kind", emc.KINDS)
def test_placement_changes_no_bit(K, kind, fam):
    """permuted trials and templates, and T and K split over 2 and 3 launches: the same bits"""
    f, (T, Kt, B) = _placement_family(kind, fam)
    rs = np.random.RandomState(5)
    pt, pk = rs.permutation(T), rs.permutation(Kt)
    full = _matrix(K, kind, f)
    assert np.all(np.isfinite(full))
    assert np.array_equal(_matrix(K, kind, f, pt, pk), full[np.ix_(pt, pk)])
    for n in (2, 3):
        parts_t = np.array_split(np.arange(T), n)
        parts_k = np.array_split(np.arange(Kt), n)
        assert np.array_equal(np.concatenate([_matrix(K, kind, f, rows=r) for r in parts_t], axis=0), full)
        assert np.array_equal(np.concatenate([_matrix(K, kind, f, cols=c) for c in parts_k], axis=1), full)
        assert np.array_equal(_matrix(K, kind, f, parts_t[-1], parts_k[-1]), full[np.ix_(parts_t[-1], parts_k[-1])])


@pytest.mark.parametrize("fam", ("mc_poisson", "mc_sigma"))
@pytest.mark.parametrize("kind", emc.KINDS)
def test_reduced_output_is_the_reduction_of_the_full_matrix(K, kind, fam):
    """best / first arg / column k0 bit for bit, with and without an offset, k0 in (0, K - 1), with two identical
    template rows (the smaller k wins the tie)"""
    src, big = _placement_family(kind, fam)
    shapes = (big, (17, 17, 5), (1, 1, 1)) + (() if kind == "conv_llh" else (emc.STRIP_SHAPE,))
    for shape in shapes:
        T, Kt, B = shape
        if shape != big:
            src = emc.family(fam, *shape)
        e, s2 = src["E"].copy(), src["S2"].copy()
        if Kt > 4:
            e[Kt - 2], s2[Kt - 2] = e[1], s2[1]          # a tie between columns 1 and Kt - 2
        f = dict(D=src["D"], E=e, S2=s2)
        d_d, d_e, d_s = _dev(K, f["D"]), _dev(K, e), _dev(K, s2)
        off = np.random.RandomState(7).randn(Kt) * 3.0
        if Kt > 4:
            off[Kt - 2] = off[1]
        full = _matrix(K, kind, f)
        for offset in (None, off):
            for k0 in sorted({0, Kt - 1}):
                best, arg, at = K.metric_matrix_best(kind, d_d, d_e, d_s, None if offset is None else _dev(K, offset),
                                                     k0=k0)
                w_best, w_arg, w_at = emc.reduce_matrix(kind, full, offset, k0)
                what = (kind, shape, offset is not None, k0)
                assert np.array_equal(arg.cpu().numpy(), w_arg), what
                assert np.array_equal(best.cpu().numpy(), w_best), what
                assert np.array_equal(at.cpu().numpy(), w_at), what
        if Kt > 4:
            # the tie is real: forcing both columns far ahead of the rest, the smaller one is reported
            lead = off.copy()
            lead[[1, Kt - 2]] = 1e300 if kind in emc.LLH_KINDS else -1e300
            _, arg, _ = K.metric_matrix_best(kind, d_d, d_e, d_s, _dev(K, lead), k0=0)
            assert np.all(arg.cpu().numpy() == 1)


def test_status_and_argument_checks(K):
    from pisa_amd import _lib

    f = emc.family("mc_poisson", 17, 16, 5)
    for kind in emc.KINDS:
        clean = _matrix(K, kind, f)
        for which in ("D", "E", "S2"):
            bad = dict(f)
            a = f[which].copy()
            a[3, 2] = -1.0
            bad[which] = a
            if which == "S2" or kind in ("mcllh_mean", "mcllh_eff"):
                with pytest.raises(ValueError):
                    _matrix(K, kind, bad)
                with pytest.raises(ValueError):
                    K.metric_matrix_best(kind, _dev(K, bad["D"]), _dev(K, bad["E"]), _dev(K, bad["S2"]))
            else:
                # clipped: the entries of the other rows keep their bits, the row's own stay finite
                got = _matrix(K, kind, bad)
                keep = np.ones_like(got, dtype=bool)
                if which == "D":
                    keep[3] = False
                else:
                    keep[:, 3] = False
                assert np.all(np.isfinite(got)) and np.array_equal(got[keep], clean[keep])
                assert not np.array_equal(got[~keep], clean[~keep])
                if which == "E" or kind == "conv_llh":
                    # the clip to SMALL_POS: what a zero in that place gives (correct_chi2 clips the expectation
                    # alone, conv_poisson the count as well)
                    zero = dict(f)
                    z = f[which].copy()
                    z[3, 2] = 0.0
                    zero[which] = z
                    assert np.array_equal(got, _matrix(K, kind, zero))
    d, e, s2 = _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"])
    lib = _lib.lib()
    out, st = _dev(K, np.zeros((17, 16))), _dev(K, np.zeros(2))
    p = lambda t: t.data_ptr()
    # any other kind, a NULL pointer, no trials, k0 outside the templates: -1 before any device access
    for kind in (0, 3, 5, 9):
        assert lib.pisa_hip_metric_matrix_mc(kind, p(d), p(e), p(s2), 17, 16, 5, p(out), p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc_best(kind, p(d), p(e), p(s2), None, 0, 17, 16, 5, p(out), p(out), p(out),
                                                  p(st), None) == -1
    for kind in (4, 6, 7, 8):
        assert lib.pisa_hip_metric_matrix_mc(kind, p(d), p(e), None, 17, 16, 5, p(out), p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc(kind, None, p(e), p(s2), 17, 16, 5, p(out), p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc(kind, p(d), p(e), p(s2), 17, 16, 5, None, p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc(kind, p(d), p(e), p(s2), 0, 16, 5, p(out), p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc_best(kind, p(d), p(e), None, None, 0, 17, 16, 5, p(out), p(out), p(out),
                                                  p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc_best(kind, p(d), p(e), p(s2), None, 0, 0, 16, 5, p(out), p(out), p(out),
                                                  p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc_best(kind, p(d), p(e), p(s2), None, 16, 17, 16, 5, p(out), p(out), p(out),
                                                  p(st), None) == -1
        assert lib.pisa_hip_metric_matrix_mc_best(kind, p(d), p(e), p(s2), None, -1, 17, 16, 5, p(out), p(out), p(out),
                                                  p(st), None) == -1
    assert np.all(out.cpu().numpy() == 0) and np.all(st.cpu().numpy() == 0)       # nothing was launched
    with pytest.raises(_lib.PisaHipError) as err:
        K.metric_matrix_best("mcllh_eff", d, e, s2, k0=16)
    assert err.value.status == -1
    with pytest.raises(ValueError):
        K.metric_matrix("conv_llh", d, e, s2, form="product")
    with pytest.raises(ValueError):
        K.metric_matrix("conv_llh", d, e)
    with pytest.raises(ValueError):
        K.metric_matrix("signed_sqrt_mod_chi2", d, e, s2)


# ------------------------------------------------------------------ config pipeline
@pytest.fixture(scope="module")
def pipeline_grid(K):
    """the 3 x 3 grid over theta23 x deltam31 of example_hip.cfg (no prior on either: the penalty is 0 for every
    metric), its template maps and 4 fluctuated data maps"""
    from pisa_amd.analysis import ensemble as en
    from pisa_amd.core.distribution_maker import DistributionMaker

    free = ("theta23", "deltam31")
    dm = DistributionMaker("settings/pipeline/example_hip.cfg")
    for name in dm.params.free.names:
        if name not in free:
            dm.params.fix(name)
    dm.get_outputs(return_sum=True)
    th, m31 = dm.params["theta23"].value, dm.params["deltam31"].value
    pts = en.grid_points(dm, {"theta23": [th * 0.8, th, th * 1.15], "deltam31": [m31 * 0.85, m31, m31 * 1.2]})
    grid = en.TemplateGrid.from_maker(dm, pts, "mcllh_eff")
    assert grid.hist.is_cuda and len(grid) == 9 and np.all(grid.penalty == 0)
    maps = []
    for k in range(9):
        dm._set_rescaled_free_params(pts[k])
        out = dm.get_outputs(return_sum=True)["total"]
        assert np.array_equal(grid.host("hist")[k], out.nominal_values.ravel()), k
        assert np.array_equal(grid.host("sumw2")[k], out.variances.ravel()), k
        maps.append(out._new(out.nominal_values.copy(), out.variances.copy()))
    assert grid.host("sumw2").max() > 0
    rs = np.random.RandomState(31)
    data = [maps[k].fluctuate("poisson", random_state=rs) for k in (0, 4, 4, 8)]
    return grid, maps, data


@pytest.mark.parametrize("metric", emc.KINDS)
def test_the_ensemble_module_on_the_config_pipeline(K, pipeline_grid, metric):
    """`en.metric_matrix` pair by pair against `Map.metric_total` (the one-pair kernel), within the two gates added;
    `feldman_cousins(generator="device")` (T = 64) is `critical_values` of the `delta_metric` loop"""
    from pisa_amd.analysis import ensemble as en

    grid, maps, data = pipeline_grid
    grid.metric = metric
    rows = np.stack([np.asarray(m.nominal_values, dtype=np.float64).ravel() for m in data])
    got = en.metric_matrix(rows, grid, metric, with_penalty=False)
    assert got.is_cuda
    got = got.cpu().numpy()
    want = np.array([[float(m.metric_total(maps[k], metric)) for k in range(9)] for m in data])
    scale = emc.scale_mc(metric, rows, grid.host("hist"), grid.host("sumw2"))
    ratio = np.abs(got - want) / (emc.EPS * scale)
    print("%s: worst %.3f eps scale (bound %.3g)" % (metric, ratio.max(), emc.g_of(metric) + mc.g_kind(metric)))
    assert np.all(np.isfinite(got)) and np.all(ratio <= emc.g_of(metric) + mc.g_kind(metric)), float(ratio.max())
    solver = en.DeviceSolver()
    T, cl, seed = 64, (0.6827, 0.90), 77
    crit = en.feldman_cousins(grid, metric, T, cl, seed, generator="device")
    loop = np.stack([en.critical_values(en.delta_metric(solver.draw(grid.hist[k], T, seed, stream=k), grid, metric, k), cl)
                     for k in range(9)])
    assert np.array_equal(crit, loop) and np.all(crit >= 0) and np.all(crit[:, 1] >= crit[:, 0])
