"""tests/kde_cases.py pinned without a GPU: the longdouble values against mpmath at 50 digits, G_REF measured again
on the fp64 restatement, and the regime each family is there to reach (cell sizes and series orders from the
restated cell-grid rule of pisa_hip_kde_create)."""
import numpy as np
import pytest

from tests import kde_cases as kc

LD = np.longdouble


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2e-19


def _mp_chain(x, w, bw, pick):
    """the pilot densities of the sources `pick` and their S, in mpmath from the raw sample (2-D / 1-D / 3-D)"""
    import mpmath as mp

    mp.mp.dps = 50
    d, n = x.shape
    X = [[mp.mpf(float(v)) for v in row] for row in x]
    W = [mp.mpf(float(v)) for v in w]
    sw = mp.fsum(W)
    wn = [v / sw for v in W]
    base = mp.mpf(n) * (d + 2) / 4 if bw == "silverman" else mp.mpf(n)
    factor = base ** (-mp.mpf(1) / (d + 4))
    mean = [mp.fsum(a * b for a, b in zip(X[k], wn)) for k in range(d)]
    Xc = [[v - mean[k] for v in X[k]] for k in range(d)]
    den = 1 - mp.fsum(v * v for v in wn)
    cov = mp.matrix(d, d)
    for a in range(d):
        for b in range(d):
            cov[a, b] = mp.fsum(Xc[a][i] * Xc[b][i] * wn[i] for i in range(n)) / den * factor ** 2
    inv = cov ** -1
    norm = mp.sqrt((2 * mp.pi) ** d * mp.det(cov))
    L = mp.cholesky(inv)       # inv = L L^T: |L^T v|^2 = v^T inv v
    Y = [[mp.fsum(L[a, k] * Xc[a][i] for a in range(k, d)) for i in range(n)] for k in range(d)]
    vals, Ss = [], []
    half = mp.mpf(1) / 2
    for j in pick:
        val = s_sum = mp.mpf(0)
        for i in range(n):
            if wn[i] == 0:
                continue
            e = half * sum((Y[k][i] - Y[k][j]) ** 2 for k in range(d))
            t = wn[i] * mp.exp(-e)
            val += t
            s_sum += t * (1 + e)
        vals.append(val / norm)
        Ss.append(s_sum / norm)
    return vals, Ss, inv, mean


@pytest.mark.parametrize("name", kc.SAMPLE_FAMILIES)
def test_longdouble_values_against_mpmath(name):
    """32 sources' pilots (the whole chain from the raw sample) and 32 queries' densities (given arrays): the
    longdouble values agree with 50-digit arithmetic to 0.01 eps S"""
    import mpmath as mp

    x, w, kw = kc.family(name)
    ex = kc.exact_case(name)
    d, n = x.shape
    rs = np.random.RandomState(5)
    pick = rs.choice(np.flatnonzero(w > 0), 32, replace=False)
    # (`narrow`'s pilot is not gated: x - mean and the whitening lose five digits there, in longdouble as well)
    vals, Ss, _, _ = _mp_chain(x, w, kw["bw_method"], pick if kc.G_REF[name][0] is not None else [])
    for j, v, s in zip(pick, vals, Ss):
        assert abs(mp.mpf(float(ex["pilot"][j])) + mp.mpf(float(ex["pilot"][j] - LD(float(ex["pilot"][j])))) - v) <= 0.01 * kc.EPS * s, (name, j)
        assert abs(float(ex["pilot_S"][j]) - float(s)) <= 1e-12 * float(s)
    # densities over given arrays: the estimator's own (rounded to fp64, as the device hands them over)
    if "coef" in ex:
        ys, coef, s2 = (np.array(ex[k], dtype=float) for k in ("ys", "coef", "s2"))
    else:       # (pilot-derived numbers are withheld for this family: the fixed-bandwidth arrays serve as given ones)
        ys, coef, s2 = np.array(ex["ys"], dtype=float), np.array(ex["wn"] / ex["norm"], dtype=float), np.ones(n)
    q, _ = kc.queries(name, 700)
    yq = np.array(kc.whiten(q, np.array(ex["inv_cov"], dtype=float), np.array(ex["mean"], dtype=float)), dtype=float)[:, rs.choice(700, 32, replace=False)]
    val, S = kc.exact_density(ys, coef, s2, yq)
    mp.mp.dps = 50
    mys = [[mp.mpf(float(v)) for v in row] for row in ys]
    mhs = [mp.mpf(float(v)) / 2 for v in s2]
    mcf = [mp.mpf(float(v)) for v in coef]
    for k in range(32):
        want = mp.mpf(0)
        mq = [mp.mpf(float(yq[a, k])) for a in range(d)]
        for i in range(n):
            if coef[i] != 0.0:
                want += mcf[i] * mp.exp(-mhs[i] * sum((mq[a] - mys[a][i]) ** 2 for a in range(d)))
        hi = float(val[k])
        got = mp.mpf(hi) + mp.mpf(float(val[k] - LD(hi)))
        assert abs(got - want) <= 0.01 * kc.EPS * mp.mpf(float(S[k])) + mp.mpf(2) ** -1074, (name, k)


def _measure_sample(orc, name):
    x, w, kw = kc.family(name)
    ex = kc.exact_case(name)
    f = kc.fp64_estimator(orc, np.array(x), np.array(w), kw["bw_method"], True, kw["alpha"])
    pos = np.asarray(w) > 0
    pilot = None
    if kc.G_REF[name][0] is not None:
        pilot = float(np.max(np.abs(f["pilot"][pos] - ex["pilot"][pos]) / (kc.EPS * ex["pilot_S"][pos])))
    else:
        assert "pilot" not in ex and "s2" not in ex
    # the sum over given arrays: the restatement's own coef, s2 and inverse bandwidth matrix, exact sum of THOSE
    q, _ = kc.queries(name, 700)
    got = orc.kde_eval(np.array(x), f["coef"], f["s2"], q, f["inv_cov"])
    val, S = kc.exact_density(kc.whiten(x, f["inv_cov"], f["mean"]), f["coef"], f["s2"], kc.whiten(q, f["inv_cov"], f["mean"]))
    # (with the gate's underflow term: a query a thousand spans away has terms below fp64's range)
    ev = float(np.max(np.abs(got - val) / (kc.EPS * S + (x.shape[1] + np.sum(f["coef"])) * kc.TINY)))
    return pilot, ev


def _measure_kernel(orc, name):
    src, coef, s2, qry, inv_cov = kc.kernel_family(name)
    val, S = kc.exact_quadratic(src, coef, s2, qry, inv_cov)
    got = orc.kde_eval(src, coef, s2, qry, inv_cov)
    return None, float(np.max(np.abs(got - val) / (kc.EPS * S)))


def test_g_ref_is_the_fp64_restatement_measured(oracle):
    """G_REF of kde_cases.py is what the CPU restatement (oracle.kde_eval under oracle/kde_oracle.py's chain) measures:
    no constant below its measurement, none more than twice above it (or 1)"""
    for name in kc.SAMPLE_FAMILIES + kc.KERNEL_FAMILIES:
        meas = _measure_kernel(oracle, name) if name in kc.KERNEL_FAMILIES else _measure_sample(oracle, name)
        print("G_REF %-12s pilot %-8s eval %.3g    constants %r" % (name, "-" if meas[0] is None else "%.3g" % meas[0], meas[1], kc.G_REF[name]))
        for m, c in zip(meas, kc.G_REF[name]):
            if c is None:
                continue
            assert m <= c <= max(1.0, 2.0 * m), (name, m, c)
        assert kc.g_of(name, "eval") == kc.KERNEL_FACTOR * max(1.0, kc.G_REF[name][1])


def test_oracle_chain_is_the_restatement(oracle):
    """`fp64_estimator` IS oracle/kde_oracle.py's estimator: same densities, bit for bit"""
    from oracle import kde_oracle

    x, w, kw = kc.family("cloud1000")
    q, _ = kc.queries("cloud1000", 257)
    f = kc.fp64_estimator(oracle, np.array(x), np.array(w), "silverman", True, 0.3)
    np.testing.assert_array_equal(oracle.kde_eval(np.array(x), f["coef"], f["s2"], q, f["inv_cov"]),
                                  kde_oracle.gaussian_kde_eval(np.array(x), np.array(w), q, "silverman", True, 0.3))


def test_capped_rows_are_the_table():
    """the cell grows by factors of 1.25 from r_cut / 8 until the grid fits max(4096, 4 n) cells; order 20 was taken
    unchecked there, with a bound far above 4 tol; with the bound checked there is no admissible order"""
    for name, cell in kc.CAPPED.items():
        x, w, kw = kc.family(name)
        g = kc.grid_rule(x, w, kw["bw_method"], kw["tol"])
        assert abs(g["cell"] - cell) < 0.006, (name, g["cell"])
        assert g["cell"] > g["r_cut"] / 8 * 1.2
        assert g["order_unchecked"] == 20 and g["order"] == 0 and g["bound20"] > 4 * kw["tol"]
    np.testing.assert_allclose([kc.grid_rule(*kc.family(n)[:2], "silverman", kc.family(n)[2]["tol"])["bound20"] for n in kc.CAPPED],
                               [7.7e-4, 1.9e-6, 1.2e-9], rtol=0.05)
    # the first row of the table: N(0,1)^2, n = 1000, nothing far away
    x = np.random.RandomState(30).randn(2, 1000)
    g = kc.grid_rule(x, np.ones(1000), "silverman", 1e-14)
    assert abs(g["cell"] - 1.004) < 1e-3 and g["order"] == 20 and abs(g["bound20"] / 1.8e-15 - 1) < 0.05


def test_cloud_orders_and_thresholds():
    for name in ("cloud999", "cloud1000", "cloud1500", "clumps", "feather"):
        x, w, _ = kc.family(name)
        for tol, order in zip(kc.TOLS, (14, 16, 18, 20)):
            g = kc.grid_rule(x, w, "silverman", tol)
            assert g["order"] == order == g["order_unchecked"] and g["cell"] == g["r_cut"] / 8, (name, tol)
    x, w, _ = kc.family("cloud1500")
    for tol in kc.TOLS:      # the series evaluated per target (flag 1) has a cell to work on at every order
        assert np.bincount(kc.grid_rule(x, w, "silverman", tol)["cell_of"]).max() >= kc.HERMITE_MIN_SERIES + 1
    assert kc.family("cloud999")[0].shape[1] == kc.EXPANSION_MIN_N - 1
    assert kc.family("cloud1000")[0].shape[1] == kc.EXPANSION_MIN_N


def test_clumps_and_feather_regimes():
    x, w, _ = kc.family("clumps")
    assert x.shape == (2, 3000)
    for tol in kc.TOLS:
        occ = np.bincount(kc.grid_rule(x, w, "silverman", tol)["cell_of"])
        occ = occ[occ > 0]
        assert 3 <= np.count_nonzero(occ >= kc.HERMITE_MIN_SERIES) < 0.02 * occ.size      # a few series, most cells none
        assert np.count_nonzero(occ == 1) > 0.7 * occ.size
    for tol in (1e-12, 1e-14):
        assert np.bincount(kc.grid_rule(x, w, "silverman", tol)["cell_of"]).max() > kc.Q_CHUNK     # cut into equal parts
    x, w, kw = kc.family("feather")
    ex = kc.exact_case("feather")
    assert x.shape == (2, 1200) and np.all(w > 0)
    light = w < 1e-5 * w.mean()
    assert light.sum() == 40 and w[light].min() < 2e-18 * w.mean()
    r = np.array(np.sqrt(np.sum((ex["ys"][:, light] - (ex["U"] @ (np.array([-1.0, -1.0]) - ex["mean"]))[:, None]) ** 2, axis=0)), dtype=float)
    r_cut = np.sqrt(2 * np.log(1e14))
    for f in (0.5, 0.9, 0.99, 1.01):
        assert np.count_nonzero(np.abs(r / r_cut - f) < 1e-6) == 8
    assert np.count_nonzero(r < 0.2) == 8
    assert np.all(ex["pilot"] > 0) and np.all(ex["lam"][light] != 1)


def test_other_families():
    x, w, _ = kc.family("narrow")
    assert abs(np.corrcoef(x)[0, 1] - 0.999) < 5e-4 and np.all(np.abs(x.mean(axis=1) - 1e3) < 0.2)
    assert kc.family("dim1")[0].shape == (1, 800) and kc.family("dim3")[0].shape == (3, 900)
    for name in kc.SAMPLE_FAMILIES:
        q, far = kc.queries(name, 700)
        x = kc.family(name)[0]
        assert q.shape == (x.shape[0], 700) and far.sum() == 8
        on = sum(np.any(np.all(q[:, k:k + 1] == x, axis=0)) for k in range(700))
        assert on >= 16
        outside = np.any((q < x.min(axis=1)[:, None]) | (q > x.max(axis=1)[:, None]), axis=0)
        assert outside.sum() >= 8
        assert kc.queries(name, 1)[0].shape[1] == 1 and kc.queries(name, 257)[0].shape[1] == 257
