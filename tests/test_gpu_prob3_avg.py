"""The production-height average of the prob3 kernels on the device ("Production-height averaging"):

  1. every averaged form against the exact QUADRATURE of tests/golden/prob3_avg_exact.npz at every node, 1e-11 absolute
     (the project's gate for an fp64 prob3 form against exact values): `propagate_array(avg_range=)` with rows per
     element and with a shared row, `prob3_grid_planned` on a plan with the range -- as the golden's 5 x 7 grid and
     embedded in 70 energies x 33 rows (ragged energy tile, short rows, rows joined over two and four waves), both
     node orders;
  2. a range of zero is the plain path, bit for bit;
  3. without the golden: the averaged call against the mean of the plain call over a 32-point Gauss-Legendre rule;
  4. several parameter points in one launch against the single-point calls;
  5. through the Stage protocol, its replay and the one-sweep metric;
  6. the refusals at the ABI.

Measured on an MI355X, worst |P - P_exact| of test 1: propagate_array with rows per element, with a shared row and
through the host call 1.29e-13 each, prob3_grid_planned 1.35e-13 as the 5 x 7 grid and embedded in 70 x 33 (either
node order); planned against the array form on all 70 x 33 nodes 1.85e-13; test 3, worst |averaged - mean of 32 plain
calls| 8.2e-15.
"""
import ctypes as C

import numpy as np
import pytest

from tests import prob3_avg_cases as T
from tests import prob3_exact_cases as X

pytestmark = pytest.mark.gpu

# the embedded grid: the golden's energies at these positions of 70 (0 and 63: first and last lane of the full tile,
# 64 and 69: first and last live lane of the ragged one), its rows at these positions of 33
N_E_BIG, N_CZ_BIG = 70, 33
E_AT = (0, 17, 63, 64, 69)
CZ_AT = (0, 5, 11, 16, 21, 27, 32)


@pytest.fixture(scope="module")
def K():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def L():
    from pisa_amd import _lib

    return _lib


def big_grid(g, r):
    """(energy[70], density[33][L], distance[33][L], dl[33]): the golden's energies and midpoint rows of range r at
    E_AT / CZ_AT; the other energies between them, the other rows the golden's with every length (and the range)
    stretched by a few per cent -- the same classes of rows, no two alike"""
    energy = np.exp(np.linspace(np.log(0.12), np.log(900.0), N_E_BIG))
    energy[list(E_AT)] = T.ENERGY
    rho = np.empty((N_CZ_BIG, g["density"][r].shape[1]))
    dist, dl = np.empty_like(rho), np.empty(N_CZ_BIG)
    for k in range(N_CZ_BIG):
        j, f = k % T.N_CZ, 1.0 + 0.013 * (k + 1)
        rho[k], dist[k], dl[k] = g["density"][r][j], g["distance"][r][j] * f, g["dl"][r][j] * f
    for j, k in enumerate(CZ_AT):
        rho[k], dist[k], dl[k] = g["density"][r][j], g["distance"][r][j], g["dl"][r][j]
    return energy, rho, dist, dl


@pytest.fixture(scope="module")
def G(K, L):
    g = T.load()
    g["d_energy"] = K.to_device(g["energy"])
    g["d_node_energy"] = K.to_device(np.repeat(g["energy"], T.N_CZ))
    g["tabs"] = []
    for r in range(len(T.RANGES)):
        rho, dist, dl = g["density"][r], g["distance"][r], g["dl"][r]
        tab = dict(rho=rho, dist=dist, dl=dl, d_rho=K.to_device(rho), d_dist=K.to_device(dist), d_dl=K.to_device(dl),
                   d_node_rho=K.to_device(np.tile(rho, (T.N_E, 1))), d_node_dist=K.to_device(np.tile(dist, (T.N_E, 1))),
                   d_node_dl=K.to_device(np.tile(dl, T.N_E)))
        tab["plan"] = K.GridPlan(tab["d_rho"], tab["d_dist"], avg_range=dl)
        e, brho, bdist, bdl = big_grid(g, r)
        tab["big"] = dict(energy=e, rho=brho, dist=bdist, dl=bdl, d_energy=K.to_device(e), d_rho=K.to_device(brho),
                          d_dist=K.to_device(bdist))
        tab["big"]["plan"] = K.GridPlan(tab["big"]["d_rho"], tab["big"]["d_dist"], avg_range=bdl)
        tab["big"]["plain"] = K.GridPlan(tab["big"]["d_rho"], tab["big"]["d_dist"])
        g["tabs"].append(tab)
    for b in g["blocks"]:
        b["params"] = L.make_prob3_params(*X.params_of(b))
    return g


def _nodes(a, n_e, n_cz, e_major):
    """[n_nodes][...] in the kernel's node order -> [n_e][n_cz][...]"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    tail = a.shape[1:]
    return a.reshape((n_e, n_cz) + tail) if e_major else np.moveaxis(a.reshape((n_cz, n_e) + tail), 0, 1)


def _tables(pepmu, n_e, n_cz, e_major):
    """pepmu[2][3][n_nodes][2] -> [sign][n_e][n_cz][init 0..1][flav]"""
    pm = pepmu.cpu().numpy() if hasattr(pepmu, "cpu") else np.asarray(pepmu)
    out = np.empty((2, n_e, n_cz, 2, 3))
    for side in range(2):
        for f in range(3):
            out[side, :, :, :, f] = _nodes(pm[side, f], n_e, n_cz, e_major)
    return out


def _report(worst):
    for form, v in sorted(worst.items()):
        print("%-44s worst |P - P_exact| %.2e" % (form, v))
    for form, v in worst.items():
        assert v <= T.GATE, (form, v)


# ------------------------------------------------------------------ 1. against the golden
def test_propagate_array_against_the_exact_average(K, G):
    worst = {}
    for k, (b, r) in enumerate(G["cases"]):
        tab = G["tabs"][r]
        for s, nubar in enumerate(T.SIGNS):
            exact = G["P_avg"][k, s]
            got = K.propagate_array(b["params"], nubar, G["d_node_energy"], tab["d_node_rho"], tab["d_node_dist"],
                                    avg_range=tab["d_node_dl"]).cpu().numpy()
            worst["propagate_array rows/element"] = max(worst.get("propagate_array rows/element", 0.0),
                                                        float(np.abs(got - exact).max()))
            got = np.empty((T.N_E, T.N_CZ, 3, 3))
            for j in range(T.N_CZ):
                got[:, j] = K.propagate_array(b["params"], nubar, G["d_energy"], tab["d_rho"][j], tab["d_dist"][j],
                                              avg_range=tab["d_dl"][j:j + 1]).cpu().numpy()
            worst["propagate_array shared row"] = max(worst.get("propagate_array shared row", 0.0),
                                                      float(np.abs(got.reshape(T.N_NODES, 3, 3) - exact).max()))
    _report(worst)


def test_propagate_array_host_against_the_exact_average(L, G):
    """the numpy-in / numpy-out call, once"""
    k = len(G["cases"]) - 1
    b, r = G["cases"][k]
    tab = G["tabs"][r]
    e = np.ascontiguousarray(np.repeat(G["energy"], T.N_CZ))
    rho, dist = np.ascontiguousarray(np.tile(tab["rho"], (T.N_E, 1))), np.ascontiguousarray(np.tile(tab["dist"], (T.N_E, 1)))
    dl = np.ascontiguousarray(np.tile(tab["dl"], T.N_E))
    got = np.full((T.N_NODES, 3, 3), np.nan)
    L.check(L.lib().pisa_hip_propagate_array_avg_host(C.byref(b["params"]), -1, e.ctypes.data, rho.ctypes.data,
                                                      dist.ctypes.data, dl.ctypes.data, T.N_NODES, rho.shape[1], 1,
                                                      got.ctypes.data))
    _report({"propagate_array_avg_host": float(np.abs(got - G["P_avg"][k, 1]).max())})


@pytest.mark.parametrize("e_major", [True, False])
def test_planned_grid_against_the_exact_average(K, G, e_major):
    worst = {}

    def settle(form, nu, nubar, pepmu, n_e, n_cz, pick, k):
        tabs = _tables(pepmu, n_e, n_cz, e_major)
        for s, got in enumerate((nu, nubar)):
            exact = G["P_avg"][k, s].reshape(T.N_E, T.N_CZ, 3, 3)
            d = float(np.abs(pick(_nodes(got, n_e, n_cz, e_major)) - exact).max())
            d = max(d, float(np.abs(pick(tabs[s]) - exact[:, :, :2, :]).max()))
            worst[form] = max(worst.get(form, 0.0), d)

    sub = np.ix_(list(E_AT), list(CZ_AT))
    for k, (b, r) in enumerate(G["cases"]):
        tab = G["tabs"][r]
        res = K.prob3_grid_planned(b["params"], tab["plan"], G["d_energy"], e_major=e_major)
        settle("prob3_grid_planned 5 x 7", *res, T.N_E, T.N_CZ, lambda a: a, k)
        big = tab["big"]
        res = K.prob3_grid_planned(b["params"], big["plan"], big["d_energy"], e_major=e_major)
        settle("prob3_grid_planned in 70 x 33", *res, N_E_BIG, N_CZ_BIG, lambda a: a[sub], k)
        if k == 0:
            # every node of the embedded grid against the reference-order array form (both within 1e-11 of exact)
            for s, nubar in enumerate(T.SIGNS):
                want = K.propagate_array(b["params"], nubar, K.to_device(np.repeat(big["energy"], N_CZ_BIG)),
                                         K.to_device(np.tile(big["rho"], (N_E_BIG, 1))),
                                         K.to_device(np.tile(big["dist"], (N_E_BIG, 1))),
                                         avg_range=K.to_device(np.tile(big["dl"], N_E_BIG))).cpu().numpy()
                d = float(np.abs(_nodes(res[s], N_E_BIG, N_CZ_BIG, e_major).reshape(-1, 3, 3) - want).max())
                print("planned against the array form on all 70 x 33 nodes, nubar %+d: %.2e" % (nubar, d))
                assert d <= 2 * T.GATE
    _report(worst)


# ------------------------------------------------------------------ 2. zero range: the plain path
@pytest.mark.parametrize("e_major", [True, False])
def test_zero_range_is_the_plain_planned_call_bit_for_bit(K, G, e_major):
    import torch

    b = G["blocks"][1]
    big = G["tabs"][1]["big"]
    plain = K.prob3_grid_planned(b["params"], big["plain"], big["d_energy"], e_major=e_major)
    averaged = K.prob3_grid_planned(b["params"], big["plan"], big["d_energy"], e_major=e_major)
    # all zero
    plan = K.GridPlan(big["d_rho"], big["d_dist"], avg_range=np.zeros(N_CZ_BIG))
    for got, want in zip(K.prob3_grid_planned(b["params"], plan, big["d_energy"], e_major=e_major), plain):
        assert torch.equal(got, want)
    # a range on some rows only: the others have the plain bits, these the averaged launch's
    some = np.where(np.arange(N_CZ_BIG) % 3 == 1, big["dl"], 0.0)
    plan.set_avg_range(some)
    res = K.prob3_grid_planned(b["params"], plan, big["d_energy"], e_major=e_major)
    zero = some == 0.0
    for got, want, avg in zip(res[:2], plain[:2], averaged[:2]):
        got, want, avg = (_nodes(a, N_E_BIG, N_CZ_BIG, e_major) for a in (got, want, avg))
        np.testing.assert_array_equal(got[:, zero], want[:, zero])
        np.testing.assert_array_equal(got[:, ~zero], avg[:, ~zero])
        assert np.abs(got[:, ~zero] - want[:, ~zero]).max() > 1e-3
    got, want, avg = (_tables(a, N_E_BIG, N_CZ_BIG, e_major) for a in (res[2], plain[2], averaged[2]))
    np.testing.assert_array_equal(got[:, :, zero], want[:, :, zero])
    np.testing.assert_array_equal(got[:, :, ~zero], avg[:, :, ~zero])
    # cleared: a fresh plan
    plan.set_avg_range(None)
    assert plan.avg_range is None
    for got, want in zip(K.prob3_grid_planned(b["params"], plan, big["d_energy"], e_major=e_major), plain):
        assert torch.equal(got, want)


def test_zero_range_is_the_plain_array_call_bit_for_bit(K, G):
    import torch

    b = G["blocks"][2]
    tab = G["tabs"][1]
    for nubar in T.SIGNS:
        plain = K.propagate_array(b["params"], nubar, G["d_node_energy"], tab["d_node_rho"], tab["d_node_dist"])
        zeros = torch.zeros_like(tab["d_node_dl"])
        assert torch.equal(K.propagate_array(b["params"], nubar, G["d_node_energy"], tab["d_node_rho"], tab["d_node_dist"],
                                             avg_range=zeros), plain)
        some = torch.where(torch.arange(T.N_NODES, device=zeros.device) % 2 == 0, tab["d_node_dl"], zeros)
        got = K.propagate_array(b["params"], nubar, G["d_node_energy"], tab["d_node_rho"], tab["d_node_dist"], avg_range=some)
        assert torch.equal(got[1::2], plain[1::2]) and float((got[0::2] - plain[0::2]).abs().max()) > 1e-3
        j = 3
        plain = K.propagate_array(b["params"], nubar, G["d_energy"], tab["d_rho"][j], tab["d_dist"][j])
        assert torch.equal(K.propagate_array(b["params"], nubar, G["d_energy"], tab["d_rho"][j], tab["d_dist"][j],
                                             avg_range=zeros[:1]), plain)


# ------------------------------------------------------------------ 3. against the plain call under a quadrature
def test_average_against_gauss_legendre_over_the_plain_call(K, L, G):
    """64 random parameter points (the recipe of prob3_exact_cases.cases: angles in [0, pi/2], dm21 in 1e-6 .. 3e-4,
    |dm31| in 5e-4 .. 6e-3 of either sign, every other point with Hermitian NSI), each on one midpoint row at an
    energy that puts the largest x_jk between 0.5 and 8: the mean of the plain call over a 32-point Gauss-Legendre
    rule in the first layer's length (exact for e^{ixt}, |x| <= 8, to 1e-30) against the averaged call.  Both sides are
    within 1e-11 of exact: 2e-11."""
    rs = np.random.RandomState(2024)
    t, w = np.polynomial.legendre.leggauss(32)
    worst = 0.0
    for k in range(64):
        th = rs.rand(3) * np.pi / 2
        delta = rs.rand() * 2 * np.pi
        dm21 = 10 ** rs.uniform(-6, -3.5)
        dm31 = (1 if rs.rand() < 0.5 else -1) * 10 ** rs.uniform(-3.3, -2.2)
        pot = X.STD_POT
        if k % 2 == 1:
            a = (rs.randn(3, 3) + 1j * rs.randn(3, 3)) * 0.2
            pot = X.STD_POT + (a + a.conj().T) / 2
        block = X._block("random_%d" % k, angles_rad=[th[0], th[1], th[2], delta], mat_pot=pot, dm21=dm21, dm31=dm31)
        params = L.make_prob3_params(*X.params_of(block))
        r, j = k % 2, (k // 2) % T.N_CZ
        rho, dist, dl = G["density"][r][j], G["distance"][r][j].copy(), float(G["dl"][r][j])
        f = int(G["first"][r][j])
        dm = block["dm"]
        gap = max(abs(dm[1][0]), abs(dm[2][0]), abs(dm[2][0] - dm[1][0]))
        x = rs.uniform(0.5, 8.0)
        energy = gap * T.HBAR_C_FACTOR * dl / (2 * x)
        assert gap * T.HBAR_C_FACTOR * (dl / energy) / 2 <= 8.0 * (1 + 1e-12)
        rows = np.tile(dist, (32, 1))
        rows[:, f] = dist[f] + 0.5 * dl * t
        d_e1, d_e32 = K.to_device(np.array([energy])), K.to_device(np.full(32, energy))
        d_rho1, d_rho32 = K.to_device(rho), K.to_device(np.tile(rho, (32, 1)))
        d_dist1, d_rows, d_dl = K.to_device(dist), K.to_device(rows), K.to_device(np.array([dl]))
        for nubar in T.SIGNS:
            plain = K.propagate_array(params, nubar, d_e32, d_rho32, d_rows).cpu().numpy()
            mean = np.tensordot(0.5 * w, plain, axes=(0, 0))
            got = K.propagate_array(params, nubar, d_e1, d_rho1, d_dist1, avg_range=d_dl).cpu().numpy()[0]
            worst = max(worst, float(np.abs(got - mean).max()))
    print("averaged call against the 32-point mean of the plain call: worst %.2e" % worst)
    assert worst <= 2 * T.GATE


# ------------------------------------------------------------------ 4. several points in one launch
@pytest.mark.parametrize("e_major", [True, False])
def test_multi_point_launch_is_the_single_point_calls(K, L, G, e_major):
    import torch

    big = G["tabs"][0]["big"]
    n = len(G["blocks"])
    assert n == 3
    arr = (L.Prob3Params * n)()
    for i, b in enumerate(G["blocks"]):
        C.memmove(C.byref(arr[i]), C.byref(b["params"]), C.sizeof(L.Prob3Params))
    nodes = N_E_BIG * N_CZ_BIG
    buf = torch.full((2, 3, nodes, n, 2), float("nan"), dtype=torch.float64, device="cuda")
    L.check(L.lib().pisa_hip_prob3_grid_planned_multi(
        C.cast(arr, C.c_void_p), n, big["plan"].handle, C.c_void_p(big["d_energy"].data_ptr()), N_E_BIG,
        1 if e_major else 0, C.c_void_p(buf.data_ptr()), K._stream()))
    for i, b in enumerate(G["blocks"]):
        _, _, pepmu = K.prob3_grid_planned(b["params"], big["plan"], big["d_energy"], e_major=e_major)
        assert torch.equal(buf[:, :, :, i, :], pepmu), b["name"]
    _, _, plain = K.prob3_grid_planned(G["blocks"][0]["params"], big["plain"], big["d_energy"], e_major=e_major)
    assert float((buf[:, :, :, 0, :] - plain).abs().max()) > 1e-3


# ------------------------------------------------------------------ 5. through the interface
def _cfg(tmp_path, name, osc_lines=""):
    from pisa_amd.utils.resources import find_resource

    text = open(find_resource("settings/pipeline/example_hip.cfg")).read()
    assert "param.n_events = 1.2e5" in text and "[osc.prob3]\n" in text
    text = text.replace("param.n_events = 1.2e5", "param.n_events = 4e3").replace("[osc.prob3]\n", "[osc.prob3]\n" + osc_lines)
    path = tmp_path / name
    path.write_text(text)
    return str(path)


RANGE_LINE = "prop_height_range = 20 * units.km\n"


def test_stage_protocol_replay_and_total_map(K, tmp_path):
    from pisa_amd.core.pipeline import Pipeline
    from pisa_amd.core.units import ureg

    path = _cfg(tmp_path, "avg.cfg", RANGE_LINE)
    slow, fast = Pipeline(path), Pipeline(path)
    slow.fast_path = False
    osc = fast["prob3"]
    assert osc.prop_height_range == 20.0 and osc.grid["plan"].avg_range is not None and np.all(osc.grid["plan"].avg_range > 0)
    for t23, dm31 in ((42.3, 2.457e-3), (47.0, 2.6e-3), (51.0, 2.3e-3)):
        for p in (slow, fast):
            p.params.theta23.value = t23 * ureg.degree
            p.params.deltam31.value = dm31 * ureg.eV ** 2
        for a, b in zip(slow.get_outputs(), fast.get_outputs()):
            np.testing.assert_array_equal(a.hist, b.hist)
            np.testing.assert_array_equal(a.std_devs, b.std_devs)
    assert fast._plan is not None and slow._plan is None, "the second pipeline must have replayed its evaluations"
    plain = Pipeline(_cfg(tmp_path, "plain.cfg"))
    assert plain["prob3"].grid["plan"].avg_range is None
    for p in (plain,):
        p.params.theta23.value = 51.0 * ureg.degree
        p.params.deltam31.value = 2.3e-3 * ureg.eV ** 2
    a, b = sum(fast.get_outputs()).hist, sum(plain.get_outputs()).hist
    assert np.abs(a - b).max() > 1e-6 * np.abs(b).max()


def test_metric_many_on_a_plan_with_the_range(K, tmp_path):
    from pisa_amd.core.distribution_maker import DistributionMaker

    dm = DistributionMaker(_cfg(tmp_path, "avg.cfg", RANGE_LINE))
    for name in dm.params.free.names:
        if name not in ("theta23", "deltam31"):
            dm.params.fix(name)
    data = dm.get_outputs(return_sum=True).fluctuate("poisson", random_state=1)
    dm.get_outputs(return_sum=True)
    assert dm.pipelines[0]._plan is not None
    rs = np.random.RandomState(4)
    x0 = np.array(dm.params.free._rescaled_values)
    pts = [np.clip(x0 + 0.05 * (rs.rand(len(x0)) - 0.5), 0, 1) for _ in range(3)]
    want = []
    for x in pts:
        dm._set_rescaled_free_params(x)
        hypo = dm.get_outputs(return_sum=True)
        want.append(data.metric_total(expected_values=hypo, metric="mod_chi2") + dm.params.priors_penalty(metric="mod_chi2"))
    eng = dm.pipelines[0]["hist"]._engine
    eng.last_many = None
    assert dm.metric_many(pts, data, "mod_chi2") == want
    assert eng.last_many is not None, "the three points must have gone through one sweep"


def test_up_going_rows_keep_the_plain_tables_without_averaging_below_the_horizon(K, tmp_path):
    import torch

    from pisa_amd.core.pipeline import Pipeline

    part = Pipeline(_cfg(tmp_path, "part.cfg", RANGE_LINE + "apply_height_avg_below_hor = False\n"))
    plain = Pipeline(_cfg(tmp_path, "plain.cfg"))
    part.get_outputs()
    plain.get_outputs()
    a, b = part["prob3"], plain["prob3"]
    g = a.grid
    up = (g["coszen"] < 0).cpu().numpy()
    assert up.any() and not up.all()
    rng = g["plan"].avg_range
    assert np.all(rng[up] == 0) and np.all(rng[~up] > 0)
    assert torch.equal(a.grid["rows"][1][torch.from_numpy(up).to(g["coszen"].device)],
                       b.grid["rows"][1][torch.from_numpy(up).to(g["coszen"].device)])
    for s in range(2):
        got = _nodes(a.prob_tables[s], g["n_e"], g["n_cz"], g["e_major"])
        want = _nodes(b.prob_tables[s], g["n_e"], g["n_cz"], g["e_major"])
        np.testing.assert_array_equal(got[:, up], want[:, up])
        assert np.abs(got[:, ~up] - want[:, ~up]).max() > 1e-3


def test_stage_rows_through_the_array_form_give_the_planned_tables(K, tmp_path):
    """what the binned calc modes other than the grid hand to `K.propagate_array(avg_range=)`: the stage's rows and
    ranges (`prob3._rows`, `Layers.height_average_rows` on the device), per node, against the stage's own planned
    tables (both forms within 1e-11 of exact: 2e-11)"""
    from pisa_amd.core.pipeline import Pipeline

    pipe = Pipeline(_cfg(tmp_path, "avg.cfg", RANGE_LINE))
    pipe.get_outputs()
    osc = pipe["prob3"]
    g = osc.grid
    n_e, n_cz = g["n_e"], g["n_cz"]
    dens, dist, rng = osc._rows(g["coszen"])
    np.testing.assert_array_equal(rng.cpu().numpy(), g["plan"].avg_range)
    first = (dist > 0).to(K.torch.int8).argmax(dim=1)
    nominal = osc.layers
    nominal.calcLayers(g["coszen"])
    d_nom = nominal.device_arrays[2]
    rows = K.torch.arange(n_cz, device=dist.device)
    other = K.torch.ones_like(dist, dtype=K.torch.bool)
    other[rows, first] = False
    assert K.torch.equal(dist[other], d_nom[other]) and bool((dens[rows, first] == 0).all())
    # the path length is concave in the production height: Lbar is below the nominal length (equal on a vertical path)
    assert bool((dist[rows, first] <= d_nom[rows, first] * (1 + 1e-12)).all()) and bool((dist[rows, first] < d_nom[rows, first]).any())
    params = osc._matrices()
    energy = g["energy"].repeat_interleave(n_cz)
    got = K.propagate_array(params, 1, energy.contiguous(), dens.repeat(n_e, 1), dist.repeat(n_e, 1), avg_range=rng.repeat(n_e))
    want = _nodes(osc.prob_tables[0], n_e, n_cz, g["e_major"]).reshape(-1, 3, 3)
    d = float(np.abs(got.cpu().numpy() - want).max())
    print("array form on the stage's rows against its planned tables: %.2e" % d)
    assert d <= 2 * T.GATE


# ------------------------------------------------------------------ 6. refusals at the ABI
def test_refusals_at_the_abi(K, L, G):
    import torch

    INVALID = -1
    lib = L.lib()
    tab = G["tabs"][0]
    b = G["blocks"][0]
    decay = X._block("decay", decay_alpha3=1e-4)
    p_decay = L.make_prob3_params(*X.params_of(decay))
    lri = X._block("lri", lri_pot=np.diag([1e-13, 0.0, -1e-13]))
    p_lri = L.make_prob3_params(*X.params_of(lri))
    dense_rho = tab["rho"].copy()
    dense_rho[2, int(G["first"][0][2])] = 2.0
    neg, nan, inf = tab["dl"].copy(), tab["dl"].copy(), tab["dl"].copy()
    neg[4], nan[1], inf[6] = -1.0, np.nan, np.inf

    # planned form: set_avg_range refuses and leaves the plan as it was; a launch with decay or LRI is refused
    plan = K.GridPlan(tab["d_rho"], tab["d_dist"])
    for bad in (neg, nan, inf):
        assert lib.pisa_hip_grid_plan_set_avg_range(plan.handle, bad.ctypes.data) == INVALID
    dense_plan = K.GridPlan(K.to_device(dense_rho), tab["d_dist"])
    assert lib.pisa_hip_grid_plan_set_avg_range(dense_plan.handle, tab["dl"].ctypes.data) == INVALID
    only_others = tab["dl"].copy()
    only_others[2] = 0.0
    assert lib.pisa_hip_grid_plan_set_avg_range(dense_plan.handle, only_others.ctypes.data) == 0
    want = K.prob3_grid_planned(b["params"], K.GridPlan(tab["d_rho"], tab["d_dist"]), G["d_energy"])
    for got, w in zip(K.prob3_grid_planned(b["params"], plan, G["d_energy"]), want):
        assert torch.equal(got, w)          # the refused ranges did not stay with the plan
    outs = [torch.full((T.N_NODES, 3, 3), 7.0, dtype=torch.float64, device="cuda") for _ in range(2)]
    outs.append(torch.full((2, 3, T.N_NODES, 2), 7.0, dtype=torch.float64, device="cuda"))
    for params in (p_decay, p_lri):
        rc = lib.pisa_hip_prob3_grid_planned(C.byref(params), tab["plan"].handle, K._ptr(G["d_energy"]), T.N_E, 1,
                                             K._ptr(outs[0]), K._ptr(outs[1]), K._ptr(outs[2]), K._stream())
        assert rc == INVALID
        arr = (L.Prob3Params * 2)()
        C.memmove(C.byref(arr[0]), C.byref(b["params"]), C.sizeof(L.Prob3Params))
        C.memmove(C.byref(arr[1]), C.byref(params), C.sizeof(L.Prob3Params))
        buf = torch.full((2, 3, T.N_NODES, 2, 2), 7.0, dtype=torch.float64, device="cuda")
        rc = lib.pisa_hip_prob3_grid_planned_multi(C.cast(arr, C.c_void_p), 2, tab["plan"].handle, K._ptr(G["d_energy"]), T.N_E,
                                                   1, K._ptr(buf), K._stream())
        assert rc == INVALID
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs + [buf])
    # decay on a plan whose ranges are all zero is the plain decay call
    zero_plan = K.GridPlan(tab["d_rho"], tab["d_dist"], avg_range=np.zeros(T.N_CZ))
    for got, w in zip(K.prob3_grid_planned(p_decay, zero_plan, G["d_energy"]), K.prob3_grid_planned(p_decay, plan, G["d_energy"])):
        assert torch.equal(got, w)

    # array form, device and host buffers
    out = torch.full((T.N_NODES, 3, 3), 7.0, dtype=torch.float64, device="cuda")
    e, rho, dist = G["d_node_energy"], tab["d_node_rho"], tab["d_node_dist"]
    d_dense = K.to_device(np.tile(dense_rho, (T.N_E, 1)))
    calls = [(b["params"], rho, K.to_device(np.tile(neg, T.N_E))), (b["params"], rho, K.to_device(np.tile(nan, T.N_E))),
             (b["params"], rho, K.to_device(np.tile(inf, T.N_E))), (b["params"], d_dense, tab["d_node_dl"]),
             (p_decay, rho, tab["d_node_dl"]), (p_lri, rho, tab["d_node_dl"])]
    for params, d_rho, d_rng in calls:
        for nubar in T.SIGNS:
            rc = lib.pisa_hip_propagate_array_avg(C.byref(params), nubar, K._ptr(e), K._ptr(d_rho), K._ptr(dist), K._ptr(d_rng),
                                                  T.N_NODES, rho.shape[1], 1, K._ptr(out), K._stream())
            assert rc == INVALID
    # the shared-row form: one range for the row
    for d_rng in (K.to_device(np.array([-1.0])), K.to_device(np.array([np.nan]))):
        rc = lib.pisa_hip_propagate_array_avg(C.byref(b["params"]), 1, K._ptr(G["d_energy"]), K._ptr(tab["d_rho"][0]),
                                              K._ptr(tab["d_dist"][0]), K._ptr(d_rng), T.N_E, rho.shape[1], 0, K._ptr(out),
                                              K._stream())
        assert rc == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    h_out = np.full((T.N_NODES, 3, 3), 7.0)
    h_e = np.ascontiguousarray(np.repeat(G["energy"], T.N_CZ))
    h_rho, h_dist = np.ascontiguousarray(np.tile(tab["rho"], (T.N_E, 1))), np.ascontiguousarray(np.tile(tab["dist"], (T.N_E, 1)))
    for params, bad in ((b["params"], neg), (b["params"], nan), (p_decay, tab["dl"])):
        h_rng = np.ascontiguousarray(np.tile(bad, T.N_E))
        rc = lib.pisa_hip_propagate_array_avg_host(C.byref(params), 1, h_e.ctypes.data, h_rho.ctypes.data, h_dist.ctypes.data,
                                                   h_rng.ctypes.data, T.N_NODES, h_rho.shape[1], 1, h_out.ctypes.data)
        assert rc == INVALID
    assert np.all(h_out == 7.0)
    # decay with every range zero is the plain decay call
    got = K.propagate_array(p_decay, 1, e, rho, dist, avg_range=torch.zeros_like(tab["d_node_dl"]))
    assert torch.equal(got, K.propagate_array(p_decay, 1, e, rho, dist))
