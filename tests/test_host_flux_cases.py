"""Pins tests/flux_cases.py without a GPU: `barr_extended` against the reference's own values
(tests/golden/barr_ref.npz, barr_wide_ref.npz) and against the C oracle on every case family, the figures the gate of
tests/test_gpu_flux.py is built from (G_REF, the smallest |d|, the clamped share of the clamp family), and the
quadrature of the integral-preservation check on the CPU oracle (R_REF_HONDA)."""
import numpy as np
import pytest

from tests.conftest import load_golden
from tests import flux_cases as fc

needs_extended = pytest.mark.skipif(not fc.extended_available(), reason=fc.NO_EXTENDED)


def _patterns(a):
    a = np.asarray(a, dtype=np.float64)
    return np.isnan(a), a == 0


@needs_extended
@pytest.mark.parametrize("golden", ["barr_ref.npz", "barr_wide_ref.npz"])
def test_barr_extended_matches_reference_goldens(golden, oracle):
    """the reference's values, the oracle's and `barr_extended`: the same NaN and zero patterns, and both fp64
    evaluations within G_REF of the extended one"""
    g = load_golden(golden)
    cols = [g[c] for c in fc.COLUMNS]
    for ip, ps in enumerate(g["params"]):
        for nubar, tag in ((1, "nu"), (-1, "nubar")):
            ext, m, d = fc.barr_extended(*cols, nubar, *ps)
            ref = g["out%d_%s" % (ip, tag)]
            orc = oracle.barr_simple(*cols, nubar, *ps)
            for a, b in zip(_patterns(ref), _patterns(orc)):
                assert np.array_equal(a, b)
            for got, what in ((ref, "reference"), (orc, "oracle")):
                fc.check_against_extended(got, ext, m, d, nubar, g["true_energy"], fc.G_REF,
                                          "%s %s set %d %s" % (golden, what, ip, tag))


def test_wide_golden_reaches_what_it_is_for():
    g = load_golden("barr_wide_ref.npz")
    e = g["true_energy"]
    assert e.size == 1024 and e.min() > 0 and np.isfinite(e).all() and e.min() < 0.2 and e.max() > 5e4
    assert list(g["true_coszen"][:3]) == [-1.0, 0.0, 1.0]
    for row, (nu, nub) in enumerate(fc.FLUX_PATTERNS):
        assert tuple(g["nu_flux_nominal"][row]) == nu and tuple(g["nubar_flux_nominal"][row]) == nub
    ps = [tuple(p) for p in g["params"]]
    assert (1.2, 0.7, 0.3, 2.0, -2.0) in ps and (0.5, 2.0, -0.3, -2.0, 2.0) in ps
    assert any(p[3] == 0 for p in ps) and any(p[0] == 0 for p in ps)
    ip = ps.index((1.2, 0.7, 0.3, 2.0, -2.0))
    body = np.arange(e.size) >= 5                           # the clamp: zeros that are not there below 5 TeV
    for tag in ("nu", "nubar"):
        out = g["out%d_%s" % (ip, tag)]
        assert 0.1 < np.mean(out[body] == 0) < 0.5 and np.all(out[body & (e > 7e3)] == 0)
        assert not np.any(out[body & (e < 4e3)] == 0)
    assert np.isnan(g["out%d_nu" % ip][2, 0]) and g["out%d_nu" % ip][2, 1] == 0      # (1, 0) / (0, 0)


@needs_extended
def test_families_against_oracle(oracle):
    """every family, parameter set and sign: the oracle's NaN and zero patterns are `barr_extended`'s, its values lie
    within G_REF; G_REF is what `barr_reference_ratios` measures; |d| stays far from 0; the clamp family clamps"""
    fams = fc.families()
    assert set(fams) == {"wide", "clamp", "patterns", "bad_energy"}
    for name, f in fams.items():
        assert f["true_energy"].size == fc.N_FAMILY == 4099
        good = np.ones(fc.N_FAMILY, dtype=bool)
        if name == "bad_energy":
            good[f["bad_rows"]] = False
            bad = f["true_energy"][~good]
            assert np.isnan(bad).sum() >= 5 and all(np.sum(bad == v) >= 5 for v in fc.BAD_ENERGIES if v == v)
            assert {0, 255, 256, fc.N_FAMILY - 1} <= set(f["bad_rows"].tolist())
        e = f["true_energy"][good]
        assert np.all(e > 0) and np.all(np.isfinite(e))
        for ip, ps in enumerate(f["psets"]):
            for nubar in (1, -1):
                ext, m, d = fc.extended_of(name, ip, nubar)
                orc = oracle.barr_simple(*(f[c] for c in fc.COLUMNS), nubar, *ps)
                fc.check_against_extended(orc, ext, m, d, nubar, f["true_energy"], fc.G_REF,
                                          "%s set %d nubar %d" % (name, ip, nubar))
                assert np.abs(d[good]).min() > 1e-9
                if name == "clamp":
                    share = fc.clamped(d, nubar).any(axis=1).mean()
                    assert (0.1 <= share <= 0.9) if ps[4] < 0 else share == 0
    e = fams["clamp"]["true_energy"]
    assert e.min() >= 3e3 and e.max() <= 1e5
    assert {ps[4] for ps in fams["clamp"]["psets"]} == {-2.0, 2.0}
    # the patterns family holds every flux pattern, the NaN ones included
    f = fams["patterns"]
    rows = f["pattern_rows"]
    for k, (nu, nub) in enumerate(fc.FLUX_PATTERNS):
        r = rows[k::len(fc.FLUX_PATTERNS)]
        assert np.all(f["nu_flux_nominal"][r] == nu) and np.all(f["nubar_flux_nominal"][r] == nub)
    ext = fc.extended_of("patterns", 0, 1)[0]
    assert np.isnan(ext[rows[2::5], 0]).all() and np.all(ext[rows[2::5], 1] == 0)
    worst, mind = fc.barr_reference_ratios(oracle)
    assert max(worst.values()) <= fc.G_REF < 1.05 * max(worst.values()), worst
    assert mind > 1e-9


@needs_extended
def test_gate_sees_the_values_on_the_bad_rows(oracle):
    """the bad-energy rows are not only patterns: E = 0 with delta_index = 0 (pow(0, 0) = 1), 1e-300 and 1e300 GeV
    give finite non-zero outputs, and the gate holds them -- an error of 1e-6 on those rows alone is refused, for
    every parameter set and sign (the gate's extra factor is 1 wherever log10 E is not finite, 60 at 1e+-300)"""
    f = fc.families()["bad_energy"]
    e = f["true_energy"]
    bad = np.zeros(fc.N_FAMILY, dtype=bool)
    bad[f["bad_rows"]] = True
    seen = set()
    for ip, ps in enumerate(f["psets"]):
        for nubar in (1, -1):
            ext, m, d = fc.extended_of("bad_energy", ip, nubar)
            orc = oracle.barr_simple(*(f[c] for c in fc.COLUMNS), nubar, *ps)
            live = bad[:, None] & np.isfinite(orc) & (orc != 0)
            seen |= set(e[live.any(axis=1)].tolist())
            ratio, cond = fc.gate_ratio(orc, ext, m, d, e)
            zero_e = live & (e == 0)[:, None]
            assert np.all(cond[zero_e] == 1.0)                      # m = 0 at E = 0: the plain gate, rtol 1e-12 too
            if not live.any():
                continue
            for rows in (live, zero_e):
                if rows.any():
                    wrong = np.where(rows, orc * (1 + 1e-6), orc)
                    with pytest.raises(AssertionError):
                        fc.check_against_extended(wrong, ext, m, d, nubar, e, fc.G_REF)
    assert {0.0, 1e-300, 1e300} <= seen


def test_extended_rule():
    """the rule of oracle/referee.py: extended means more than fp64's 53 bits"""
    assert fc.extended_available() == (np.finfo(np.longdouble).nmant > 52)


def test_quadrature_is_exact_and_oracle_preserves_the_honda_bins():
    """3 Gauss-Legendre nodes integrate a quadratic per interval exactly; the CPU oracle's interpolant then
    reproduces every bin of the Honda table to R_REF_HONDA of its band's total integral"""
    from pisa_amd.utils.resources import find_resource

    x, w = fc.gauss_nodes(np.array([0.0, 0.5, 2.0]))
    np.testing.assert_allclose((w * (3 * x ** 2 - x)).reshape(2, 3).sum(axis=1), [0.0, 8 - 0.125 - 2 + 0.125], rtol=1e-14, atol=1e-15)
    for name, table, n_e in (("honda", fc.HONDA, 101), ("bartol", fc.BARTOL, 70)):
        energy, bands = fc.read_table(find_resource(table))
        assert energy.size == n_e and all(bands[p].shape == (20, n_e) and np.all(bands[p] > 0) for p in fc.TABLE_COLUMNS)
        pts = fc.quadrature_points(name, energy)
        assert pts["e"].size == 3 * n_e and pts["cz"].size == 60 and abs(pts["wc"].sum() - 2.0) < 1e-14
        assert np.all(np.abs(pts["cz"]) < 1)
    r = fc.oracle_preservation_residual(find_resource(fc.HONDA))
    assert r <= fc.R_REF_HONDA < 2 * r, r
