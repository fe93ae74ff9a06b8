"""The flux chain on the device: `pisa_hip_flux_2d` (flux.honda_ip) and the Barr systematics in both kernel forms
(`pisa_hip_barr_simple[_multi]`; `pisa_hip_barr_factors` + `pisa_hip_barr_fold_multi`).

flux_2d   vs the reference's own values (golden vectors made by importing pisa/utils/flux_weights.py,
          oracle/gen_golden.py:gen_flux), vs the oracle restatement on fresh points, on and next to every kind of
          spline knot and at the launch's block edge, and -- the one check that depends on neither of them -- the
          integral of the interpolant over every bin of the Honda and the Bartol table against the table entry.
Barr      vs `barr_extended` (tests/flux_cases.py: the formulas in extended precision) from 0.1 GeV to 100 TeV, where
          modRatioNuBar clamps, on the flux pairs that give NaN, at energies that do not exist; the one-pass form
          bit for bit against the two-pass one.

The Barr gate (tests/flux_cases.py): |got - ext| <= G eps (1 + |m| / |d|) |ext| with G = KERNEL_FACTOR * G_REF =
4 * 5.1 = 20.4, G_REF being the worst such ratio of the reference's own fp64 values and of the C oracle (5.09 and
4.10, measured on the CPU and held there by tests/test_host_flux_cases.py).  The kernels' own worst ratio on an MI355X:
    4.54 (barr_wide_ref.npz), 4.06 (wide), 3.42 (clamp), 4.10 (patterns), 3.97 (bad-energy family) -- the same
    through `barr_simple` and `barr_simple_multi`; the claim of csrc/metric_flux.hip, "the same value to an ulp / two
    ulp", holds from 0.1 GeV to 100 TeV: the kernels are as close to the extended value as glibc's pow is.
    The bad-energy figure is under a gate that is NOT the formula above at two of its energies: at 1e-300 and 1e300
    GeV the right side carries a further factor |log10 E| / 5 = 60 (tests/flux_cases.py, `gate_ratio`), because the
    exponent of LogLogParam's 10^t is about 140 there and no fp64 evaluation meets the plain gate (the C oracle: 123).
    E = 0, -1, NaN and inf are held to the plain gate.
Integral preservation: |quadrature - table entry| <= 16 r_ref (band's total integral), r_ref = 1.0e-15 (Honda, the
CPU oracle: 8.9e-16 measured) and 1.04e-15 (Bartol, the reference's own function).  The kernel's residuals on an MI355X:
    Honda 9.9e-16, Bartol 1.04e-15 (worst of 4 primaries x 20 bands x 101 / 70 bins) against the bound 1.6e-14.
Every test prints its figure before it asserts (`pytest -s`)."""
import os

import numpy as np
import pytest

from tests import flux_cases as fc

pytestmark = pytest.mark.gpu
needs_extended = pytest.mark.skipif(not fc.extended_available(), reason=fc.NO_EXTENDED)

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TABLE = "flux/honda-2015-spl-solmin-aa.d"
# spline interpolation of tabulated fluxes: the reference's per-event QR solve and
# our cardinal-spline product differ by rounding only
TOL = dict(rtol=1e-10, atol=0.0)


def test_flux_2d_matches_reference_goldens():
    from pisa_amd.utils import flux_weights as fw

    g = np.load(os.path.join(GOLD, "flux_ref.npz"))
    assert str(g["table"]) == TABLE
    table = fw.load_2d_table(TABLE)
    nu, nubar = fw.calculate_2d_flux_weights(g["true_energy"], g["true_coszen"], table)
    nu, nubar = nu.cpu().numpy(), nubar.cpu().numpy()
    np.testing.assert_allclose(nu[:, 0], g["nue"], **TOL)
    np.testing.assert_allclose(nu[:, 1], g["numu"], **TOL)
    np.testing.assert_allclose(nubar[:, 0], g["nuebar"], **TOL)
    np.testing.assert_allclose(nubar[:, 1], g["numubar"], **TOL)


def test_flux_2d_matches_oracle_and_rejects_bad_coszen():
    from oracle import flux_oracle
    from pisa_amd.utils import flux_weights as fw
    from pisa_amd.utils.resources import find_resource

    rs = np.random.RandomState(5)
    n = 3000
    e = 10 ** (rs.rand(n) * 4.5 - 1)
    cz = rs.rand(n) * 2 - 1
    table = fw.load_2d_table(TABLE)
    nu, nubar = fw.calculate_2d_flux_weights(e, cz, table)
    ref = flux_oracle.load_2d_honda_table(find_resource(TABLE))
    sel = slice(0, 300)  # the oracle follows the reference's per-event Python loop
    for col, prim in ((nu[:, 0], "nue"), (nu[:, 1], "numu"), (nubar[:, 0], "nuebar"), (nubar[:, 1], "numubar")):
        want = flux_oracle.calculate_2d_flux_weights(e[sel], cz[sel], ref[prim])
        np.testing.assert_allclose(col.cpu().numpy()[sel], want, **TOL)
    assert np.all(nu.cpu().numpy() > 0)
    cz[17] = 1.0000001
    with pytest.raises(ValueError):
        fw.calculate_2d_flux_weights(e, cz, table)
    with pytest.raises(ValueError):
        fw.load_2d_table("flux/honda-2015-spl-solmin.d")  # not azimuth averaged


def test_bartol_table_matches_reference_goldens():
    """`load_2d_table` on a Bartol table (flux_weights.py:133-203: Honda-like layout, two energy step
    widths) -> the band splines have non-uniform knots; same kernel.  Against values produced by the
    reference's own code (tests/golden/flux_bartol_ref.npz, oracle/gen_golden.py:gen_flux)."""
    from pisa_amd.utils import flux_weights as fw

    g = np.load(os.path.join(GOLD, "flux_bartol_ref.npz"))
    table = fw.load_2d_table(str(g["table"]))
    assert table["name"] == "bartol"
    nu, nubar = fw.calculate_2d_flux_weights(g["true_energy"], g["true_coszen"], table)
    nu, nubar = nu.cpu().numpy(), nubar.cpu().numpy()
    np.testing.assert_allclose(nu[:, 0], g["nue"], **TOL)
    np.testing.assert_allclose(nu[:, 1], g["numu"], **TOL)
    np.testing.assert_allclose(nubar[:, 0], g["nuebar"], **TOL)
    np.testing.assert_allclose(nubar[:, 1], g["numubar"], **TOL)


# ------------------------------------------------------------- flux_2d: what the table itself demands
@pytest.mark.parametrize("name, table_file, r_ref", [("honda", fc.HONDA, fc.R_REF_HONDA), ("bartol", fc.BARTOL, fc.R_REF_BARTOL)])
def test_flux_2d_preserves_the_table_integrals(name, table_file, r_ref):
    """The interpolation is integral preserving: over every table bin (one data interval in log10 E x one coszen
    band) the kernel's flux x E^enpow, summed over the bin's 3 x 3 Gauss-Legendre nodes (exact: a quadratic in each
    variable), gives table x E^enpow x dlogE x dcz to 16 r_ref of the band's total integral.  Nothing here comes from
    scipy's coefficients, the oracle or a golden: the table text is read with numpy."""
    from pisa_amd.utils import flux_weights as fw
    from pisa_amd.utils.resources import find_resource

    energy, bands = fc.read_table(find_resource(table_file))
    pts = fc.quadrature_points(name, energy)
    ee, cc = [np.ascontiguousarray(a.ravel()) for a in np.meshgrid(pts["e"], pts["cz"], indexing="ij")]
    table = fw.load_2d_table(table_file)
    assert table["name"] == name
    nu, nubar = fw.calculate_2d_flux_weights(ee, cc, table)
    nu, nubar = nu.cpu().numpy(), nubar.cpu().numpy()
    grids = dict(nue=nu[:, 0], numu=nu[:, 1], nuebar=nubar[:, 0], numubar=nubar[:, 1])
    res = {p: fc.preservation_residual(name, energy, bands[p], pts, grids[p].reshape(pts["e"].size, -1))
           for p in fc.TABLE_COLUMNS}
    print("integral preservation, %s: worst residual / band integral %s (r_ref %.3g, bound %.3g)"
          % (name, {p: "%.3g" % r for p, r in res.items()}, r_ref, fc.QUAD_FACTOR * r_ref))
    assert max(res.values()) <= fc.QUAD_FACTOR * r_ref, res


def _knot_points(table):
    """<= 300 points on and next to the knots of both splines, and beyond both ends of the table's energies"""
    rs = np.random.RandomState(8)
    t_e = np.unique(np.asarray(table["nue"]["0.95"][0]))            # -1.025, then the data points 2 .. 99, 4.025
    pick = np.unique(np.concatenate([np.arange(0, t_e.size, 8), [1, 2, t_e.size - 3, t_e.size - 2, t_e.size - 1]]))
    e_k = 10 ** t_e[pick]
    e_special = np.concatenate([e_k, np.nextafter(e_k, 0.0), np.nextafter(e_k, np.inf)])
    cz_k = np.linspace(-1, 1, 21)                                   # every knot of the coszen spline
    cz_special = np.concatenate([cz_k, np.nextafter(cz_k, -2.0)[1:], np.nextafter(cz_k, 2.0)[:-1]])
    assert cz_special.size == 61 and cz_special.min() == -1.0 and cz_special.max() == 1.0
    n_e, n_c = e_special.size, cz_special.size
    e = np.concatenate([10 ** (rs.rand(n_c) * 4.5 - 1), e_special, np.resize(e_special, n_c + 20),
                        np.repeat([0.05, 3e4], 4)])
    cz = np.concatenate([cz_special, rs.rand(n_e) * 2 - 1, np.resize(cz_special, n_c + 20),
                         np.tile([-1.0, 0.0, 0.33, 1.0], 2)])
    assert e.size == cz.size <= 300
    # the knots are hit: log10 lands on a knot or within two ulp of it, on either side
    x = np.log10(e_special)[:, None]
    off = np.min(np.abs(x - t_e[None, :]), axis=1)
    assert np.all(off <= 4 * np.finfo(float).eps * np.maximum(1, np.abs(x[:, 0]))) and np.any(off == 0)
    return e, cz


def test_flux_2d_on_the_knots_matches_oracle():
    """`find_interval` decides where log10(E) or coszen sits exactly on a knot of its spline, one ulp below or one
    above: all 21 coszen knots; of the 100 distinct energy knots every 8th and the three at either end, the two
    not-a-knot ends among them (18 knots: each costs three energies and the oracle is a Python loop, so 300 points do
    not hold them all); both table ends (0.05 GeV, 30 TeV).
    What this can and cannot see: the flux is the DERIVATIVE of a cubic spline, continuous with its own derivative
    across a knot, so the polynomial of either neighbouring interval gives the same value there to rounding -- a
    `find_interval` that takes the left interval on a knot (`x > t[mid]`) passes, rightly; one that is off by an
    interval anywhere else, or that leaves the coefficient window, does not."""
    from oracle import flux_oracle
    from pisa_amd.utils import flux_weights as fw
    from pisa_amd.utils.resources import find_resource

    table = fw.load_2d_table(TABLE)
    e, cz = _knot_points(table)
    nu, nubar = fw.calculate_2d_flux_weights(e, cz, table)
    ref = flux_oracle.load_2d_honda_table(find_resource(TABLE))
    for col, prim in ((nu[:, 0], "nue"), (nu[:, 1], "numu"), (nubar[:, 0], "nuebar"), (nubar[:, 1], "numubar")):
        want = flux_oracle.calculate_2d_flux_weights(e, cz, ref[prim])
        got = col.cpu().numpy()
        print("knots, %s: worst relative deviation %.3g" % (prim, np.max(np.abs(got - want) / np.abs(want))))
        np.testing.assert_allclose(got, want, **TOL)


def test_flux_2d_launch_edges_and_rejections():
    """n = 1, 255, 256, 257 (the launch's block edge): the rows of one large call, bit for bit, and nothing written
    past n.  coszen outside [-1, 1] or NaN raises like the reference; a NaN or non-positive ENERGY is NaN for that
    event alone (the reference: log10 -> NaN through its splines), raises nothing and leaves its neighbours' bits."""
    import torch

    from pisa_amd import kernels as K
    from pisa_amd.utils import flux_weights as fw

    table = fw.load_2d_table(TABLE)
    rs = np.random.RandomState(9)
    n_big = 700
    e = 10 ** (rs.rand(n_big) * 5 - 1)
    cz = rs.rand(n_big) * 2 - 1
    cz[[0, 254, 255, 256]] = [-1.0, 1.0, -1.0, 1.0]             # the ends of the range do not raise
    e_d, cz_d = K.to_device(e), K.to_device(cz)
    big_nu, big_nubar = fw.calculate_2d_flux_weights(e_d, cz_d, table)
    assert torch.isfinite(big_nu).all() and torch.isfinite(big_nubar).all()
    for n in (1, 255, 256, 257):
        out_nu = torch.full((n + 2, 2), -7.0, dtype=torch.float64, device="cuda")
        out_nubar = torch.full((n + 2, 2), -7.0, dtype=torch.float64, device="cuda")
        fw.calculate_2d_flux_weights(e_d[:n].contiguous(), cz_d[:n].contiguous(), table, out_nu, out_nubar)
        assert torch.equal(out_nu[:n], big_nu[:n]) and torch.equal(out_nubar[:n], big_nubar[:n]), n
        assert torch.all(out_nu[n:] == -7.0) and torch.all(out_nubar[n:] == -7.0), n
    for bad_cz in (np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), np.nan):
        for where in (0, 255, 256, n_big - 1):
            cz_bad = cz.copy()
            cz_bad[where] = bad_cz
            with pytest.raises(ValueError):
                fw.calculate_2d_flux_weights(e, cz_bad, table)
    where = np.array([0, 17, 255, 256, 257, n_big - 1])
    e_bad = e.copy()
    e_bad[where] = [np.nan, 0.0, -1.0, -0.0, np.nan, -1e300]
    nu, nubar = fw.calculate_2d_flux_weights(e_bad, cz, table)     # no status, no exception
    keep = np.ones(n_big, dtype=bool)
    keep[where] = False
    keep_d = torch.from_numpy(keep).cuda()
    assert torch.isnan(nu[~keep_d]).all() and torch.isnan(nubar[~keep_d]).all()
    assert torch.equal(nu[keep_d], big_nu[keep_d]) and torch.equal(nubar[keep_d], big_nubar[keep_d])


# ------------------------------------------------------------------------------ Barr systematics
_DEV = {}


def _columns(name, rows=None):
    """a family's four columns on the device (moved once)"""
    from pisa_amd import kernels as K

    if name not in _DEV:
        f = fc.families()[name]
        _DEV[name] = tuple(K.to_device(np.array(f[c])) for c in fc.COLUMNS)
    cols = _DEV[name]
    return cols if rows is None else tuple(c[:rows].contiguous() for c in cols)


def _barr(entry, cols, ps):
    """{+1: out, -1: out} as device tensors through `barr_simple` or one `barr_simple_multi` launch of both signs"""
    import torch

    from pisa_amd import kernels as K

    if entry == "single":
        return {sg: K.barr_simple(*cols, sg, *ps) for sg in (1, -1)}
    n = cols[0].numel()
    outs = {sg: torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda") for sg in (1, -1)}
    K.barr_simple_multi(K.barr_sets([cols + (sg, outs[sg]) for sg in (1, -1)]), *ps)
    return outs


ENTRIES = ("single", "multi")


@pytest.mark.parametrize("entry", ENTRIES)
def test_barr_wide_golden_patterns(entry):
    """against the reference's own values from 0.1 GeV to 100 TeV (tests/golden/barr_wide_ref.npz): the NaN
    pattern and the zero pattern -- the clamp of modRatioNuBar, the flux pairs (x, 0) -- are the reference's"""
    from pisa_amd import kernels as K
    from tests.conftest import load_golden

    g = load_golden("barr_wide_ref.npz")
    cols = tuple(K.to_device(g[c]) for c in fc.COLUMNS)
    zeros = 0
    for ip, ps in enumerate(g["params"]):
        outs = _barr(entry, cols, ps)
        for sg, tag in ((1, "nu"), (-1, "nubar")):
            got, want = outs[sg].cpu().numpy(), g["out%d_%s" % (ip, tag)]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (ip, tag)
            assert np.array_equal(got == 0, want == 0), (ip, tag)
            zeros += int(np.sum(want[5:] == 0))
    assert zeros > 400      # the clamp is there


@needs_extended
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("source", ["barr_wide_ref.npz"] + list(fc.good_energy_families()))
def test_barr_against_extended(entry, source):
    """NaN and zero pattern of the extended value, exactly 0.0 where it is clamped, elsewhere within
    4 G_REF eps (1 + |m| / |d|) of it -- and within the suite's rtol = 1e-12 wherever 1 + |m| / |d| < 10"""
    from pisa_amd import kernels as K
    from tests.conftest import load_golden

    if source.endswith(".npz"):
        g = load_golden(source)
        host = [g[c] for c in fc.COLUMNS]
        cols, psets = tuple(K.to_device(a) for a in host), [tuple(p) for p in g["params"]]
        ext_of = lambda ip, sg: fc.barr_extended(*host, sg, *psets[ip])  # noqa: E731
    else:
        host = [fc.families()[source][c] for c in fc.COLUMNS]
        cols, psets = _columns(source), fc.families()[source]["psets"]
        ext_of = lambda ip, sg: fc.extended_of(source, ip, sg)  # noqa: E731
    worst = 0.0
    for ip, ps in enumerate(psets):
        outs = _barr(entry, cols, ps)
        for sg in (1, -1):
            ext, m, d = ext_of(ip, sg)
            worst = max(worst, fc.check_against_extended(outs[sg].cpu().numpy(), ext, m, d, sg, host[0],
                                                         fc.KERNEL_FACTOR * fc.G_REF,
                                                         "%s %s set %d nubar %d" % (entry, source, ip, sg)))
    print("Barr %s, %s: worst gate ratio %.3g (G_REF %.3g, gate %.3g)"
          % (entry, source, worst, fc.G_REF, fc.KERNEL_FACTOR * fc.G_REF))


@needs_extended
@pytest.mark.parametrize("entry", ENTRIES)
def test_barr_bad_energies_two_pass(entry, oracle):
    """E = 0, -1, NaN, inf, 1e-300, 1e300 among good events (the two-pass form takes them; the one-pass form refuses):
    the oracle's NaN, inf and zero pattern (the reference's pow for E <= 0), the extended value at the same gate
    wherever there is one -- E = 0 with delta_index = 0 gives pow(0, 0) = 1 and an ordinary flux, held to the plain gate
    and to rtol = 1e-12; 1e-300 and 1e300 GeV are held to 60 times the plain gate (`flux_cases.gate_ratio`: not even the
    C oracle meets the plain one there, it deviates by 123 eps) -- and the good events keep the bits they have without
    the bad ones"""
    import torch

    from pisa_amd import kernels as K

    f = fc.families()["bad_energy"]
    host = [f[c] for c in fc.COLUMNS]
    cols = _columns("bad_energy")
    good = np.ones(fc.N_FAMILY, dtype=bool)
    good[f["bad_rows"]] = False
    good_d = torch.from_numpy(good).cuda()
    clean = (K.to_device(np.where(good, host[0], 1.0)),) + cols[1:]
    worst = 0.0
    for ip, ps in enumerate(f["psets"]):
        outs, outs_clean = _barr(entry, cols, ps), _barr(entry, clean, ps)
        for sg in (1, -1):
            got = outs[sg].cpu().numpy()
            orc = oracle.barr_simple(*host, sg, *ps)
            differ = np.isnan(got) != np.isnan(orc)
            assert not differ.any(), (ps, sg, host[0][differ.any(axis=1)][:8], got[differ.any(axis=1)][:8])
            assert np.array_equal(np.isinf(got), np.isinf(orc)) and np.array_equal(got == 0, orc == 0), (ip, sg)
            assert not np.isnan(got[good]).any()
            ext, m, d = fc.extended_of("bad_energy", ip, sg)
            worst = max(worst, fc.check_against_extended(got, ext, m, d, sg, host[0], fc.KERNEL_FACTOR * fc.G_REF,
                                                         "%s bad_energy set %d nubar %d" % (entry, ip, sg)))
            assert torch.equal(outs[sg][good_d], outs_clean[sg][good_d]), (ip, sg)
            if ps[2] == 0:      # values, not only patterns, on bad rows: E = 0 among them
                valued = ~good[:, None] & np.isfinite(got) & (got != 0)
                assert valued[host[0] == 0].any() and valued[host[0] == 1e300].any(), (ip, sg)
    print("Barr %s, bad_energy: worst gate ratio %.3g (gate %.3g)" % (entry, worst, fc.KERNEL_FACTOR * fc.G_REF))


def _one_pass(sets, ps):
    """`pisa_hip_barr_factors` per set, then ONE `pisa_hip_barr_fold_multi` launch with static_w = 1 ->
    (outputs with two guard rows each, status word of the factors)"""
    import torch

    from pisa_amd import _lib
    from pisa_amd import kernels as K

    lib = _lib.lib()
    arr = (_lib.BarrFoldSet * len(sets))()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep, outs = [], []
    for d, (cols, sg) in zip(arr, sets):
        e, cz, nu, nub = cols
        n = e.numel()
        fac = torch.full((5 * n + 2,), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.pisa_hip_barr_factors(K._ptr(e), K._ptr(cz), n, K._ptr(fac), K._ptr(status), K._stream()))
        assert torch.all(fac[5 * n:] == -7.0)
        w = torch.ones(n, dtype=torch.float64, device="cuda")
        out = torch.full((n + 2, 2), -7.0, dtype=torch.float64, device="cuda")
        d.n, d.nubar = n, sg
        d.d_nu_flux_nominal, d.d_nubar_flux_nominal = nu.data_ptr(), nub.data_ptr()
        d.d_factors, d.d_static_w, d.d_out = fac.data_ptr(), w.data_ptr(), out.data_ptr()
        keep += [fac, w]
        outs.append(out)
    _lib.check(lib.pisa_hip_barr_fold_multi(arr, len(sets), *[float(p) for p in ps], K._stream()))
    torch.cuda.synchronize()
    return outs, int(status.item())


def test_barr_one_pass_equals_two_pass_bit_for_bit():
    """the one-pass form (five stored factors per event, folded with static_w = 1) over the wide and the clamp
    family in one launch of two ragged sets: the bits of `barr_simple`, nothing written past a set's n, status 0;
    one non-positive (or NaN, or infinite) energy among them sets the status word"""
    import torch

    from pisa_amd import kernels as K

    ragged = {"wide": fc.N_FAMILY, "clamp": 11 * 256 + 1}
    psets = list(fc.PSETS_WIDE) + list(fc.PSETS_CLAMP[1:])
    for flip in (1, -1):
        sets = [(_columns("wide", ragged["wide"]), flip), (_columns("clamp", ragged["clamp"]), -flip)]
        for ps in psets:
            outs, status = _one_pass(sets, ps)
            assert status == 0
            for (cols, sg), out in zip(sets, outs):
                n = cols[0].numel()
                assert torch.equal(out[:n], K.barr_simple(*cols, sg, *ps)), (flip, ps, n)
                assert torch.all(out[n:] == -7.0)
    cols = _columns("wide")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        e = cols[0].clone()
        e[300] = bad
        _, status = _one_pass([((e,) + cols[1:], 1)], psets[0])
        assert status != 0, bad
