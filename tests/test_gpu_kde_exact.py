"""Every form of csrc/kde.hip against exact values (np.longdouble, held to mpmath by tests/test_host_kde_cases.py):
the pilot stage through the local bandwidths it produces, the point evaluation and `kde_eval` over given arrays, the
lattice recurrence at every strip length and lane-group width.  Families, exact values and the gate are in
tests/kde_cases.py:

    |got - exact| <= G eps S + c_T tol sum coef + lambda sum a + U        (per density value)

Departures from the issue's wording (argued in tests/kde_cases.py, used to less than 1 % by the device except where
stated): an underflow term U = (n + sum coef) 2^-1074 in the gate (met only by the far queries at tol = 0); `+ G eps`
in the s2 / coef allowance; G_REF per family and stage (tighter than one constant for every family but `narrow`).
The one-sided check is made on density values (point evaluation, written-out lattice); the pilot is not handed out.

The pilot densities themselves are not handed out; they are gated through s2 = lam^2 and coef, whose allowance is the
pilot's carried through lam = (p / g)^alpha (kde_cases.pilot_allowances).  Point evaluation and lattice are gated
against the exact sum over the DEVICE's own (ys, coef, s2), so the pilot's error does not enter, and one-sidedly too
(a cut-off only drops positive terms).

Worst ratios to the gate on an MI355X (printed by every test under `pytest -s`; the gate is 1) are in RESULTS below,
with what the capped-grid and featherweight tests found and which scratch mutation of kde.hip fails which test.
"""
import numpy as np
import pytest

from tests import kde_cases as kc

pytestmark = pytest.mark.gpu
LD = np.longdouble

RESULTS = """
form (kernels)                                                     worst |got - exact| / gate      of it above exact
pilot, local expansions (flag 2; orders 14, 16 MFMA / 18, 20 VALU)  cloud1500 7.4e-4  clumps 8.0e-3  cloud1000 7.2e-4
pilot, series per target (flag 1; kde_hermite_pilot_kernel<P>)      cloud1500 7.5e-4  clumps 8.0e-3
pilot, pair sums (flag 0 / n = 999; kde_pairs_kernel<2, false, 2>)  cloud1500 3.7e-3  clumps 4.0e-2  cloud999 2.8e-3
pilot, capped grids (pair sums after the fix, both flags)           w100 2.2e-3  w60 3.0e-5  u200 2.4e-2
pilot, feather                                                      flag 2 6.5e-10  flag 0 7.9e-10
point evaluation, tol > 0 (kde_pairs_kernel<D, true, 1>)            <= 0.093 (narrow); clouds 3.5e-3         <= 0.25 G eps S
point evaluation, tol = 0                                           cloud1500 0.25  dim1 0.31  dim3 0.39     <= 0.26 G eps S
kde_eval (all pairs, library exp)                                   0.25 (|error| <= 8.8 eps S, as the CPU oracle's)
lattice R = 32 / 16 / 8, LG = 8                                     0.033 / 0.028 / 0.028
lattice written out (R = 0)                                         0.0027
lattice R = 8, LG = 16 / 32 / 64                                    0.17 / 0.35 / 0.26
(the pilot is held through s2 and coef: its allowance is dominated by c_T tol sum coef over the pilot itself, so the
ratios are small wherever the pilot is far above tol; 98-100 % of cloud / capped / feather sources and a third of
`clumps` are held to better than 1e-9 relative, the rest -- tails at the cut-off -- to what the truncation bound says)

Capped grid: REAL.  The library before the fix ran a series of order 20 on all three samples (n_dense 49 / 55 / 11) at
cells of 3.83 / 2.84 / 1.96, where the order's own truncation bound is 7.7e-4 / 1.9e-6 / 1.2e-9 of a cell's weight against
the 4e-14 / 4e-12 / 4e-14 promised: test_pilot_stage_on_a_capped_grid[*-2] fails there.  After the fix n_dense = 0 and
the ratios above.
Featherweight sources: NOT CONFIRMED on this family.  Under both pilot forms each of the 40 sources (1e-18 ... 1e-6 of the
mean weight, 0 ... 1.01 r_cut from a cell of 290 heavy sources) got a positive pilot and a bandwidth inside the gate;
none kept s2 == 1.  kde.hip is unchanged there.
exp_nonpos' "2 ulp": a host replica of its instruction sequence against long double, 2e7 arguments in [-708, 0]: 1.000 ulp
at worst.  The lattice's 3e-13: tests/kde_cases.py (derivation and replica: 2.1e-13); the device uses a third of the gate.

Scratch mutations of kde.hip (nothing of them is in the tree) and the tests that fail:
  1. highest-order row of the Hermite coefficients (both coefficient kernels) set to 0: NO test fails.  The dropped row is
     what the next lower order would truncate, and the order is chosen so that the bound is met with room: the worst
     ratios move from 7.4e-4 to 8.3e-4 (cloud1500, tol 1e-10) and from 6.5e-10 to 1.3e-8 (feather), nothing else moves.
     The gate is the code's promise (4 tol of a cell's weight), and this mutation keeps it.
  2. `reach` one cell short on one side in the first h2l pass (both kernels): test_pilot_stage_with_featherweight_sources[2]
     fails at 7.6 x the gate -- the sources at 0.9 ... 1.01 r_cut are the ones that need the outermost cell.
  3. Q_3 of the lattice's table x (1 + 1e-9): every test_lattice_every_strip_length case with R > 0 and more than one
     point along index 0 (7) and all three test_lattice_every_lane_group_width cases fail.
  4. cell_s2min replaced by the cell's largest s2: test_point_evaluation_over_the_devices_own_arrays fails on capped_w100,
     capped_w60 and the three adaptive dim3 cases at tol 1e-14, test_lattice_every_strip_length on the written-out lattice,
     test_lattice_every_lane_group_width (through the point evaluation it is held to) on all three.
  5. 1/13! doubled in exp_nonpos: NO test fails, no printed ratio moves.  The change is 0.75 ulp of a term at most
     (r^13 / 13! at |r| = ln 2 / 2); the gate's rounding term is G >= 18 eps because the fp64 CPU restatement it is
     scaled by is itself 4.6 ... 37 eps S off.  A gate of a few ulp needs a reference chain that whitens first.
"""

def _estimator(name, **over):
    from pisa_amd import kernels as K

    x, w, kw = kc.family(name)
    kw.update(over)
    est = K.KdeEstimator(K.to_device(np.array(x)), K.to_device(np.array(w)), **kw)
    return est, x, w, kw


def _arrays(est):
    return tuple(np.array(t.cpu().numpy()) for t in est.arrays())


def _configured(flag):
    from pisa_amd import _lib

    lib = _lib.lib()

    class Ctx:
        def __enter__(self):
            self.old = lib.pisa_hip_kde_configure(-1)
            lib.pisa_hip_kde_configure(flag)

        def __exit__(self, *a):
            lib.pisa_hip_kde_configure(self.old)

    return Ctx()


def _gate_pilot(name, est, x, w, kw, what):
    """s2 and coef of the estimator against the exact estimator; returns the exact values in the device's order"""
    d, n = x.shape
    ys, coef, s2 = _arrays(est)
    idx = kc.match_sources(ys, est.inv_cov, est.mean, x)
    ex = kc.exact_case(name, alpha=kw["alpha"])
    c_t = 0.0 if kw["tol"] == 0 else (5.0 if est.n_dense > 0 else 1.0)
    rel_s2, rel_coef, rho = kc.pilot_allowances(ex, kc.g_of(name, "pilot"), c_t, kw["tol"], kw["alpha"], d)
    pos = np.asarray(w)[idx] > 0
    assert np.all(s2[~pos] == 1.0) and np.all(coef[~pos] == 0.0)          # weightless: the global bandwidth, no term
    assert np.all(np.isfinite(s2)) and np.all(s2 > 0) and np.all(coef[pos] > 0)
    r_s2 = np.abs(LD(1) * s2 - ex["s2"][idx]) / (ex["s2"][idx] * rel_s2[idx])
    r_cf = np.where(pos, np.abs(LD(1) * coef - ex["coef"][idx]) / np.where(pos, ex["coef"][idx] * rel_coef[idx], 1), 0)
    worst = float(max(r_s2[pos].max(), r_cf.max()))
    tight = float(np.mean(rho[np.asarray(w) > 0] < 1e-9))
    print("pilot %-44s n_dense %4d  c_T %d  worst ratio %.3g (s2 %.3g, coef %.3g); %.0f %% of the sources held to < 1e-9"
          % (what, est.n_dense, c_t, worst, float(r_s2[pos].max()), float(r_cf.max()), 100 * tight))
    assert worst <= 1.0, (what, worst)
    return ex, idx, s2, pos


@pytest.mark.parametrize("flag", [2, 1, 0])
@pytest.mark.parametrize("tol", kc.TOLS)
@pytest.mark.parametrize("name", ["cloud1500", "clumps"])
def test_pilot_stage_every_order_and_form(name, tol, flag):
    """orders 14 / 16 (matrix cores: kde_hermite_coef_mfma_kernel, kde_h2l_mfma_kernel<0/1>,
    kde_local_pilot_wave_kernel<14/16>) and 18 / 20 (vector units: kde_hermite_coef_kernel, kde_h2l4_kernel,
    kde_local_pilot_kernel<18/20, false>) under flag 2, kde_hermite_pilot_kernel<P> under flag 1 (on `clumps` beside
    direct sums of the cells without a series), kde_pairs_kernel<2, false, 2> under flag 0"""
    with _configured(flag):
        est, x, w, kw = _estimator(name, tol=tol)
    g = kc.grid_rule(x, w, kw["bw_method"], tol)
    assert est.cell == pytest.approx(g["cell"], rel=1e-12) and g["order"] == dict(zip(kc.TOLS, (14, 16, 18, 20)))[tol]
    assert (est.n_dense > 0) == (flag != 0 and x.shape[1] >= kc.EXPANSION_MIN_N)
    if flag == 1 and name == "clumps":
        assert 0 < est.n_dense < np.unique(g["cell_of"]).size
    if flag == 2:       # a series for every non-empty cell (a source on a cell's edge may fall either way in fp64)
        assert abs(est.n_dense - np.unique(g["cell_of"]).size) <= 2
    _gate_pilot(name, est, x, w, kw, "%s tol %g flag %d" % (name, tol, flag))


@pytest.mark.parametrize("name,dense", [("cloud999", False), ("cloud1000", True)])
def test_pilot_stage_either_side_of_the_expansion_threshold(name, dense):
    est, x, w, kw = _estimator(name)
    assert (est.n_dense > 0) == dense
    _gate_pilot(name, est, x, w, kw, name)


@pytest.mark.parametrize("flag", [2, 0])
@pytest.mark.parametrize("name", list(kc.CAPPED))
def test_pilot_stage_on_a_capped_grid(name, flag):
    """FOUND HERE: where the cell grid had to fit max(4096, 4 n) cells (two far events, with or without weight, widen
    the bounding box) the cells are up to 3.8 wide instead of r_cut / 8 = 1.0 and series order 20 was taken without
    its bound being checked: truncation bound 7.7e-4 / 1.9e-6 / 1.2e-9 of a cell's weight at a tolerance of 1e-14 /
    1e-12 / 1e-14.  FIXED: the expansion is admitted only where an order up to 20 meets 4 tol; otherwise the pilot is
    the pair sum (n_dense = 0)."""
    with _configured(flag):
        est, x, w, kw = _estimator(name)
    assert est.cell > est.r_cut / 8 * 1.2
    assert est.cell == pytest.approx(kc.CAPPED[name], abs=0.006)
    _gate_pilot(name, est, x, w, kw, "%s flag %d" % (name, flag))      # (c_T = 5 if a series ran all the same)
    assert est.n_dense == 0


@pytest.mark.parametrize("flag", [2, 0])
def test_pilot_stage_with_featherweight_sources(flag):
    """sources of 1e-18 ... 1e-6 of the mean weight beside a heavy cell, up to and just beyond its cut-off: their
    exact pilot is positive (the cell's tail plus their own term), so none may silently keep the global bandwidth"""
    with _configured(flag):
        est, x, w, kw = _estimator("feather")
    assert (est.n_dense > 0) == (flag != 0)
    ex, idx, s2, pos = _gate_pilot("feather", est, x, w, kw, "feather flag %d" % flag)
    kept = pos & (s2 == 1.0) & np.asarray(ex["lam"][idx] != 1)
    print("feather flag %d: %d weighted sources with s2 == 1.0 exactly" % (flag, kept.sum()))
    assert not kept.any(), np.asarray(w)[idx][kept]


# ------------------------------------------------------------------ point evaluation, stage-isolated
_POINT_CASES = [(name, {}, 700) for name in kc.SAMPLE_FAMILIES]
_POINT_CASES += [("cloud1500", dict(tol=0.0), 700), ("cloud1500", {}, 1), ("cloud1500", {}, 257), ("dim3", {}, 1), ("dim1", {}, 257),
                 ("clumps", dict(tol=1e-10), 700)]
_POINT_CASES += [(name, dict(tol=tol, adaptive=ad, bw_method=bw), 700) for name in ("dim1", "dim3") for tol in (1e-14, 0.0)
                 for ad in (True, False) for bw in ("silverman", "scott")]


def _gate_density(got, ys, coef, s2, yq, g, tol, lam, what, far=None):
    val, S = kc.exact_density(ys, coef, s2, yq)
    n = ys.shape[1]
    sc = float(np.sum(coef))
    allow = kc.allowance(val, S, sc, n, g, 1.0 if tol > 0 else 0.0, tol, lam)
    worst = kc.gate_ratio(got, val, allow)
    over = kc.one_sided_ratio(got, val, S, sc, n, g) if lam == 0 else float("nan")
    rounding = float(np.max(np.where(S > 0, np.abs(LD(1) * got - val) / np.where(S > 0, kc.EPS * S, 1), 0)))
    print("%-60s worst ratio %.3g; above the exact value: %.3g of G eps S; |error| / (eps S) %.3g (G %.3g)" % (what, worst, over, rounding, g))
    assert worst <= 1.0, (what, worst)
    if lam == 0:
        assert over <= 1.0, (what, over)
    if far is not None and far.any():
        assert np.all(np.asarray(got)[far] == 0.0)


@pytest.mark.parametrize("name,over,m", _POINT_CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, str) else v)
def test_point_evaluation_over_the_devices_own_arrays(name, over, m):
    """`est(q)` (kde_pairs_kernel<D, true, 1>, n_split > 1) against the exact sum over the estimator's own arrays:
    inside the cloud, outside it, exactly on sources, and where every kernel value is below fp64's range (0)"""
    from pisa_amd import kernels as K

    est, x, w, kw = _estimator(name, **over)
    ys, coef, s2 = _arrays(est)
    if not kw["adaptive"]:
        assert np.all(s2 == 1.0)
    q, far = kc.queries(name, m)
    got = est(K.to_device(q)).cpu().numpy()
    yq = kc.whiten(q, est.inv_cov, est.mean)
    _gate_density(got, ys, coef, s2, yq, kc.g_of(name, "eval"), kw["tol"], 0.0,
                  "point %s %s m %d" % (name, ",".join("%s=%s" % kv for kv in sorted(over.items())), m), far)
    if kw["tol"] == 0:
        assert est.pairs_eval == x.shape[1] * m


def test_kde_eval_all_pairs_kernel():
    """`kde_eval` (every pair, the library's exp) at the shapes of test_gpu_kde.py::test_kde_kernel_vs_oracle"""
    from pisa_amd import kernels as K

    for name in kc.KERNEL_FAMILIES:
        src, coef, s2, qry, inv_cov = kc.kernel_family(name)
        got = K.kde_eval(K.to_device(src), K.to_device(coef), K.to_device(s2), K.to_device(qry), inv_cov).cpu().numpy()
        val, S = kc.exact_quadratic(src, coef, s2, qry, inv_cov)
        g = kc.g_of(name, "eval")
        worst = kc.gate_ratio(got, val, kc.allowance(val, S, float(coef.sum()), src.shape[1], g))
        print("kde_eval %s: worst ratio %.3g; |error| / (eps S) %.3g (G %.3g)" % (name, worst, worst * g, g))
        assert worst <= 1.0


# ------------------------------------------------------------------ lattice
_LAT = {}


def _lattice_estimator():
    if not _LAT:
        est, x, w, kw = _estimator("cloud1500", alpha=0.5)
        ys, coef, s2 = _arrays(est)
        U = np.array(kc.whitening(est.inv_cov), dtype=float)
        _LAT.update(est=est, x=x, kw=kw, ys=ys, coef=coef, s2=s2, u00=U[0, 0], u11=U[1, 1])
    return _LAT


def _lattice_points(origin, step, counts):
    i0, i1 = np.meshgrid(np.arange(counts[0]), np.arange(counts[1]), indexing="ij")
    return np.stack([LD(origin[0]) + i0.ravel() * LD(step[0]), LD(origin[1]) + i1.ravel() * LD(step[1])])


def _lattice_case(da_s, counts, want_r, want_lg=None, sample=False):
    """lattice centred on the cloud; step 0 = da_s / (U00 sqrt(max s2)) so that the strip rule sees da_s"""
    from pisa_amd import kernels as K

    L = _lattice_estimator()
    est, x = L["est"], L["x"]
    step = [da_s / (L["u00"] * np.sqrt(L["s2"].max())), (x[1].max() - x[1].min()) * 1.2 / max(counts[1] - 1, 1)]
    origin = [np.median(x[0]) - step[0] * (counts[0] - 1) * 0.47, x[1].min() - 0.1 * (x[1].max() - x[1].min())]
    tol = L["kw"]["tol"]
    assert kc.lattice_strip(L["u00"] * step[0] * np.sqrt(L["s2"].max()), tol) == want_r
    if want_lg:
        assert kc.lattice_shape(x.shape[1], tol, L["u00"], L["u11"], step, counts, want_r)[1] == want_lg
        assert kc.lattice_shape(x.shape[1], tol, L["u00"], L["u11"], step, counts, want_r)[2] <= 4096 < \
            (counts[0] + want_r - 1) // want_r * counts[1] / (want_lg // 2)
    elif want_r:
        assert kc.lattice_shape(x.shape[1], tol, L["u00"], L["u11"], step, counts, want_r)[1] == 8
    lat = est.evaluate_lattice(origin, step, counts).cpu().numpy()
    pts = _lattice_points(origin, step, counts)
    m = pts.shape[1]
    what = "lattice R %d LG %s counts %s" % (want_r, want_lg or 8, counts)
    if sample:
        direct = est(K.to_device(np.array(pts, dtype=float))).cpu().numpy()
        np.testing.assert_allclose(lat, direct, rtol=2e-12, atol=1e-13 * direct.max())
        pick = np.zeros(m, dtype=bool)
        pick[::97] = True
        pick[[0, counts[1] - 1, m - counts[1], m - 1]] = True
        pick.reshape(counts)[:, -1] = True
        pick.reshape(counts)[-1, :] = True
        # ... and, since nearly all of such a lattice lies beyond every cut-off, up to 4000 of the points that do not
        y64 = np.array(kc.whitening(est.inv_cov), dtype=float) @ (np.array(pts, dtype=float) - est.mean[:, None])
        gap = np.maximum(np.maximum(L["ys"].min(axis=1)[:, None] - y64, y64 - L["ys"].max(axis=1)[:, None]), 0)
        inside = np.flatnonzero(np.sum(gap * gap, axis=0) * L["s2"].min() <= 2.0 * np.log(1.0 / tol))
        pick[inside[::max(1, inside.size // 4000)]] = True
        pick = np.flatnonzero(pick)
    else:
        pick = np.arange(m)
    yq = kc.whiten(pts[:, pick], est.inv_cov, est.mean)
    # a point further than r_cut / sqrt(min s2) from the box of the sources has every term below coef_i tol: the exact
    # value is within [0, tol sum coef] by that alone, and so must the device's be (which is the gate's truncation term)
    lo, hi = L["ys"].min(axis=1)[:, None], L["ys"].max(axis=1)[:, None]
    gap = np.maximum(np.maximum(lo - yq, yq - hi), 0)
    beyond = np.array(np.sum(gap * gap, axis=0) * L["s2"].min() > 2.0 * np.log(1.0 / tol) * (1 + 1e-9), dtype=bool)
    # (the recurrence skips a strip only if EVERY point of it is beyond the cut-off, the pair kernel a cell likewise: a
    #  point beyond it may still receive terms, each below coef_i tol)
    sum_coef = float(np.sum(L["coef"]))
    assert np.all(lat[pick[beyond]] >= 0.0) and np.all(lat[pick[beyond]] <= tol * sum_coef * (1 + 1e-12))
    near = ~beyond
    assert near.sum() >= min(m, 20)
    _gate_density(lat[pick[near]], L["ys"], L["coef"], L["s2"], yq[:, near], kc.g_of("cloud1500", "eval"), tol,
                  kc.LATTICE_LAMBDA if want_r else 0.0, what + " (%d of %d points summed exactly)" % (near.sum(), m))
    assert lat.max() > 0


@pytest.mark.parametrize("da_s,counts,want_r", [
    (0.15, (131, 45), 32),      # counts that are no multiple of the strip or of the sub-patch
    (1.5, (67, 33), 32),        # the longest strip at the coarsest step it is admitted for
    (2.5, (37, 45), 16),
    (3.125, (35, 9), 16),
    (5.0, (19, 45), 8),
    (6.25, (9, 70), 8),
    (8.0, (7, 45), 0),          # the points written out
    (0.15, (1, 45), 32),        # a count of 1 in either index
    (0.15, (131, 1), 32),
    (5.0, (1, 1), 8),
])
def test_lattice_every_strip_length(da_s, counts, want_r):
    """kde_lattice_kernel<32 / 16 / 8, 8> and the written-out fallback, every point against the exact sum over the
    estimator's arrays, with lambda = 3e-13 of the value for the recurrence"""
    _lattice_case(da_s, counts, want_r)


@pytest.mark.parametrize("counts,lg", [((551, 557), 16), ((787, 769), 32), ((1103, 1109), 64)])
def test_lattice_every_lane_group_width(counts, lg):
    """more than 4096 sub-patches at R = 8: kde_lattice_kernel<8, 16 / 32 / 64>.  The whole lattice against the point
    evaluation (rtol 2e-12, atol 1e-13 max), every 97th point, the corners, the last line and the last column exactly"""
    _lattice_case(5.0, counts, 8, lg, sample=True)
