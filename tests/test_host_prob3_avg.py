"""The production-height average of the prob3 kernels, host side ("Production-height averaging"; the device
side is tests/test_gpu_prob3_avg.py):

  * the closed form, restated in numpy (tests/prob3_avg_cases.py), against the QUADRATURE of the exact layered
    probabilities stored in tests/golden/prob3_avg_exact.npz (scripts/dev/gen_prob3_avg_golden.py), within the
    project's gate for an fp64 prob3 form against exact values: 1e-11 absolute, every node;
  * `Layers.height_average_rows` on the CPU oracle's rows;
  * the stage's refusals and the cfg text of `prop_height_range`.
"""
import numpy as np
import pytest

from tests import prob3_avg_cases as T
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def G():
    return T.load()


def test_golden_holds_the_cases_and_the_generator_checked_it(G):
    np.testing.assert_array_equal(G["energy"], T.ENERGY)
    np.testing.assert_array_equal(G["coszen"], T.COSZEN)
    np.testing.assert_array_equal(G["ranges"], T.RANGES)
    assert G["P_avg"].shape == (len(T.cases()), 2, T.N_NODES, 3, 3)
    assert [(b["name"], r) for b, r in G["cases"]] == [(b["name"], r) for b, r in T.cases()]
    for b, want in zip(G["blocks"], T.blocks()):
        for k in ("dm", "mix", "mat_pot"):
            np.testing.assert_array_equal(b[k], want[k])
    # quadrature against the closed form in 55-digit arithmetic, and the quadrature's own error estimate
    assert G["closed_form_agreement"].max() < 1e-30 and G["quad_error"].max() < 1e-30
    # the midpoint rows: first layer without electrons, Lbar inside (L_min, L_max), dL = L_max - L_min
    rr = np.arange(T.N_CZ)
    for r in range(len(T.RANGES)):
        f = G["first"][r]
        assert np.all(G["density"][r][rr, f] == 0.0)
        np.testing.assert_array_equal(G["distance"][r][rr, f], G["lbar"][r])
        np.testing.assert_array_equal(G["dl"][r], G["lmax"][r] - G["lmin"][r])
        assert np.all(G["lmin"][r] < G["lbar"][r]) and np.all(G["lbar"][r] < G["lmax"][r])
    # probabilities: rows and columns of the average still sum to one
    np.testing.assert_allclose(G["P_avg"].sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(G["P_avg"].sum(axis=-2), 1.0, rtol=0, atol=1e-14)


def test_closed_form_against_the_exact_quadrature_at_every_node(G):
    worst, moved = 0.0, 0.0
    for k, (block, r) in enumerate(G["cases"]):
        for s, nubar in enumerate(T.SIGNS):
            for ie, e in enumerate(T.ENERGY):
                for j in range(T.N_CZ):
                    U, Tm = T.chain_product(block, nubar, e, G["density"][r][j], G["distance"][r][j])
                    got = T.closed_form(U, Tm, block["dm"], G["dl"][r][j] / e)
                    want = G["P_avg"][k, s, ie * T.N_CZ + j]
                    worst = max(worst, float(np.abs(got - want).max()))
                    plain = T.closed_form(U, Tm, block["dm"], 0.0)
                    moved = max(moved, float(np.abs(plain - want).max()))
    print("numpy closed form: worst |P - P_exact| %.2e; the average moves a probability by up to %.3f" % (worst, moved))
    assert worst <= T.GATE
    assert moved > 0.1      # the cases are ones where the average matters


def _oracle_rows(oracle, prem, depth, ye):
    def rows_at(cz, height):
        lay = oracle.Layers(prem, depth, height)
        lay.setElecFrac(*ye)
        lay.calcLayers(np.asarray(cz))
        n = len(cz)
        return np.array(lay.density).reshape(n, -1), np.array(lay.distance).reshape(n, -1)

    return rows_at


def test_layers_helper_on_the_oracle_rows(oracle, G):
    from pisa_amd.stages.osc.layers import Layers

    g = load_golden("layers_ref.npz")
    depth, height, yi, yo, ym = g["prem12::args"]
    prem = np.array(g["prem12::prem"], dtype=np.float64, copy=True)
    lay = Layers(prem, depth, height)
    lay.setElecFrac(yi, yo, ym)
    rows_at = _oracle_rows(oracle, prem, depth, (yi, yo, ym))
    cz = np.concatenate([T.COSZEN, np.linspace(-0.97, 0.97, 41)])
    rho_nom, d_nom = rows_at(cz, height)
    for r, rng in enumerate(T.RANGES):
        dens, dist, dl = lay.height_average_rows(cz, rng, rows_at=rows_at)
        _, d_lo = rows_at(cz, height - rng / 2)
        _, d_hi = rows_at(cz, height + rng / 2)
        first = np.argmax(d_nom > 0, axis=1)
        rr = np.arange(len(cz))
        assert np.all(rho_nom[rr, first] == 0.0)           # the atmosphere
        lmin, lmax, lbar = d_lo[rr, first], d_hi[rr, first], dist[rr, first]
        assert np.all(lmin < lbar) and np.all(lbar < lmax)
        np.testing.assert_array_equal(dl, lmax - lmin)
        # every other layer does not depend on the production height: the three Layers agree bit for bit, and the
        # helper returns the nominal ones
        other = np.ones_like(d_nom, dtype=bool)
        other[rr, first] = False
        np.testing.assert_array_equal(dens, rho_nom)
        for d in (dist, d_lo, d_hi):
            np.testing.assert_array_equal(d[other], d_nom[other])
        # dL grows towards the horizon from either side
        for side in (cz >= 0, cz <= 0):
            d_side = dl[side][np.argsort(np.abs(cz[side]), kind="stable")]       # from the horizon to the vertical
            assert np.all(np.diff(d_side) <= 0) and d_side[0] > 5 * d_side[-1]      # (coszen 0 is in the list twice)
            assert len(np.unique(d_side)) == len(d_side) - 1
        assert dl[np.argmin(np.abs(cz))] == dl.max() and abs(dl[np.argmax(np.abs(cz))] - rng) < 1e-9
        # and the golden file's rows are these
        np.testing.assert_array_equal(dist[:T.N_CZ], G["distance"][r])
        np.testing.assert_array_equal(dl[:T.N_CZ], G["dl"][r])
    for bad in (0.0, -1.0, float("nan"), 2 * height + 1e-9):
        with pytest.raises(ValueError):
            lay.height_average_rows(cz, bad, rows_at=rows_at)
    lay.height_average_rows(cz[3:4], 2 * height - 1.0, rows_at=rows_at)      # up to twice the height is a range


def _params():
    from pisa_amd.stages.osc.prob3 import init_test

    return init_test().params


def test_stage_refuses_what_the_average_does_not_cover():
    """before any device work: the constructor raises, nothing is set up"""
    from pisa_amd.core.param import Param
    from pisa_amd.core.units import ureg
    from pisa_amd.stages.osc.prob3 import prob3

    rng = 20 * ureg.km
    with pytest.raises(ValueError, match="calc_mode"):
        prob3(prop_height_range=rng, params=_params(), calc_mode="events", apply_mode="events")
    p = _params()
    p.extend([Param(name="decay_alpha3", value=1e-4 * ureg.eV ** 2)])
    with pytest.raises(ValueError, match="neutrino_decay"):
        prob3(prop_height_range=rng, neutrino_decay=True, params=p)
    p = _params()
    p.extend([Param(name="v_lri", value=1e-14 * ureg.eV)])
    with pytest.raises(ValueError, match="lri_type"):
        prob3(prop_height_range=rng, lri_type="emu-symmetry", params=p)
    for bad in (0 * ureg.km, -3 * ureg.km, 20.0):
        with pytest.raises(ValueError, match="prop_height_range"):
            prob3(prop_height_range=bad, params=_params())
    st = prob3(prop_height_range="20 * units.km", apply_height_avg_below_hor=False, params=_params())
    assert st.prop_height_range == 20.0 and st.apply_height_avg_below_hor is False
    st = prob3(prop_height_range=1500 * ureg.m, params=_params())
    assert st.prop_height_range == 1.5 and st.apply_height_avg_below_hor is True
    assert prob3(params=_params()).prop_height_range is None


def test_cfg_text_gives_the_quantity(tmp_path):
    from pisa_amd.core.config_parser import parse_pipeline_config
    from pisa_amd.core.units import ureg
    from pisa_amd.utils.resources import find_resource

    text = open(find_resource("settings/pipeline/example_hip.cfg")).read()
    text = text.replace("[osc.prob3]\n", "[osc.prob3]\nprop_height_range = 20 * units.km\napply_height_avg_below_hor = False\n")
    path = tmp_path / "avg.cfg"
    path.write_text(text)
    kw = parse_pipeline_config(str(path))[("osc", "prob3")]
    assert kw["prop_height_range"].units == ureg.km and kw["prop_height_range"].magnitude == 20.0
    assert kw["apply_height_avg_below_hor"] is False
