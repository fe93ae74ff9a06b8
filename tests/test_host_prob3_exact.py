"""The exact layered propagator (oracle/exact_prob3.py) against closed forms it does not use, its
independence of the working precision, the committed golden file against a recomputation, and the fp64
oracle against the exact values: the condition under which tests/test_gpu_prob3_exact.py may hold the
device to the reference's own gate at EVERY node."""
import numpy as np
import pytest

mp = pytest.importorskip("mpmath")

from oracle import exact_prob3 as X                          # noqa: E402
from tests import prob3_exact_cases as T                      # noqa: E402
from tests.conftest import PROB3_ATOL, PROB3_RTOL, load_golden  # noqa: E402

TIGHT = mp.mpf(10) ** -30


@pytest.fixture(scope="module")
def G():
    return T.load()


def _f(x):
    return mp.mpf(float(x))


def _zero():
    return mp.matrix(3, 3)


def _unitary(th12, th13, th23, delta):
    """the PMNS matrix from angles at the working precision: unitary to that precision, which the fp64 matrix
    of a case (fp64 sines, c = sqrt(1 - s^2) rounded) is only to 1e-16"""
    s12, s13, s23 = (mp.sin(_f(t)) for t in (th12, th13, th23))
    c12, c13, c23 = (mp.cos(_f(t)) for t in (th12, th13, th23))
    ed = mp.expj(_f(delta))
    return mp.matrix([[c12 * c13, s12 * c13, s13 / ed],
                      [-s12 * c23 - c12 * s23 * s13 * ed, c12 * c23 - s12 * s23 * s13 * ed, s23 * c13],
                      [s12 * s23 - c12 * c23 * s13 * ed, -c12 * s23 - s12 * c23 * s13 * ed, c23 * c13]])


def _amplitude(U, dm21, dm31, nubar, energy, density, distance, pot=None, lri=None, decay=None):
    return X.amplitude_mp(U, _f(dm21), _f(dm31), X._mat(T.STD_POT) if pot is None else pot, -1 if decay is None else 1,
                          _zero() if decay is None else decay, _zero() if lri is None else lri, nubar, _f(energy),
                          [_f(x) for x in density], [_f(x) for x in distance], X.cache_sources(density, distance))


def test_two_flavour_vacuum_formula():
    """theta12 = theta13 = 0: nu_mu <-> nu_tau with the splitting dm32, P = sin^2(2 theta23) sin^2(dm32 (L/E) 2.534 / 2),
    nu_e decoupled; three baselines, cut into vacuum layers of unequal length; both signs"""
    th23, dm21, dm31 = 0.7, 7.5e-5, 2.457e-3
    with mp.workdps(X.DPS + X.GUARD):
        U = _unitary(0.0, 0.0, th23, 0.0)
        for energy, lengths in ((0.37, [20.0, 312.5]), (6.1, [12742.0]), (1e3, [1.0, 2.0, 4000.0, 8000.25])):
            arg = (_f(dm31) - _f(dm21)) * sum(_f(x) / _f(energy) for x in lengths) * _f(X.HBAR_C_FACTOR) / 2
            want = mp.sin(2 * _f(th23)) ** 2 * mp.sin(arg) ** 2
            for nubar in T.SIGNS:
                P = X.probabilities_of(_amplitude(U, dm21, dm31, nubar, energy, np.zeros(len(lengths)), lengths))
                assert abs(P[1][2] - want) < TIGHT and abs(P[2][1] - want) < TIGHT
                assert abs(P[1][1] - (1 - want)) < TIGHT and abs(P[2][2] - (1 - want)) < TIGHT
                assert abs(P[0][0] - 1) < TIGHT and abs(P[0][1]) < TIGHT and abs(P[0][2]) < TIGHT


def test_three_flavour_vacuum_sum_over_U():
    """P(i -> j) = |sum_k U_jk exp(-i m_k (L/E) 2.534) conj(U_ik)|^2 with m = (0, dm21, dm31): no matrix exponential"""
    with mp.workdps(X.DPS + X.GUARD):
        for angles, dm21, dm31 in (((0.58, 0.148, 0.73, 0.0), 7.5e-5, 2.457e-3), ((0.58, 0.149, 0.86, 4.43), 7.5e-5, -2.374e-3),
                                   ((1.3, 0.9, 0.2, 2.0), 1e-6, 5e-3)):
            U = _unitary(*angles)
            for energy, baseline in ((0.1, 12742.0), (2.9, 500.0), (1e4, 9000.0)):
                for nubar in T.SIGNS:
                    V = U if nubar > 0 else U.apply(mp.conj)
                    phi = _f(baseline) / _f(energy) * _f(X.HBAR_C_FACTOR)
                    e = [mp.expj(-m * phi) for m in (mp.mpf(0), _f(dm21), _f(dm31))]
                    P = X.probabilities_of(_amplitude(U, dm21, dm31, nubar, energy, [0.0], [baseline]))
                    for i in range(3):
                        for j in range(3):
                            want = abs(sum(V[j, k] * e[k] * mp.conj(V[i, k]) for k in range(3))) ** 2
                            assert abs(P[i][j] - want) < TIGHT, (angles, energy, nubar, i, j)


def test_rows_and_columns_sum_to_one_without_decay(G):
    """through the whole Earth (core row, core-limit row, mantle row of the stored tables), in standard matter, with
    a Hermitian NSI potential and with a long-range potential"""
    tab = G["earths"]["prem12"]
    rs = np.random.RandomState(8)
    a = (rs.randn(3, 3) + 1j * rs.randn(3, 3)) * 0.2
    b = rs.randn(3, 3) * 1e-13
    with mp.workdps(X.DPS + X.GUARD):
        U = _unitary(0.58, 0.148, 0.73, 1.1)
        for pot, lri in ((None, None), (X._mat(T.STD_POT + (a + a.conj().T) / 2), None), (None, X._mat((b + b.T) / 2))):
            for nubar in T.SIGNS:
                for energy, row in ((0.37, 0), (40.0, 2), (1e5, 3)):
                    P = X.probabilities_of(_amplitude(U, 7.5e-5, 2.457e-3, nubar, energy, tab["density"][row],
                                                      tab["distance"][row], pot=pot, lri=lri))
                    for k in range(3):
                        assert abs(sum(P[k]) - 1) < TIGHT and abs(sum(P[m][k] for m in range(3)) - 1) < TIGHT


def test_one_layer_equals_its_two_unequal_parts():
    """exp(-i H (l1 + l2)) = exp(-i H l1) exp(-i H l2), with decay as well; the cache rule does not merge 300 and 700 km"""
    assert X.cache_sources([4.5, 4.5], [300.0, 700.0]) == [0, 1]
    decay = _zero()
    with mp.workdps(X.DPS + X.GUARD):
        decay[2, 2] = mp.mpc(0, -_f(1e-4))
        U = _unitary(0.58, 0.148, 0.73, 1.1)
        for dec in (None, decay):
            for nubar in T.SIGNS:
                for energy in (0.37, 40.0, 1e4):
                    whole = X.probabilities_of(_amplitude(U, 7.5e-5, 2.457e-3, nubar, energy, [4.5], [1000.0], decay=dec))
                    parts = X.probabilities_of(_amplitude(U, 7.5e-5, 2.457e-3, nubar, energy, [4.5, 4.5], [300.0, 700.0], decay=dec))
                    for i in range(3):
                        for j in range(3):
                            assert abs(whole[i][j] - parts[i][j]) < TIGHT, (dec is not None, nubar, energy)
                    if dec is not None:
                        assert sum(whole[2]) < 1 - 1e-6 or energy > 1e3      # decay loses probability


def test_cache_rule_is_the_reference_s():
    # the LAST earlier match, matches chain, zero-length layers neither match nor are matched
    rho = [1.0, 2.0, 1.0 + 5e-6, 1.0, 3.0, 1.0]
    dist = [10.0, 10.0, 10.0, 10.0 - 5e-6, 0.0, 10.0 + 2e-5]
    assert X.cache_sources(rho, dist) == [0, 1, 0, 2, -1, 5]
    # a layer handed the matrix of a DIFFERENT layer: the result follows the cache, not the layer's own values
    c = T.cases()[0]
    a = X.probabilities(*T.params_of(c), 1, 2.9, np.array([3.0, 3.0 + 9e-6]), np.array([900.0, 900.0 - 9e-6]))
    b = X.probabilities(*T.params_of(c), 1, 2.9, np.array([3.0, 3.0]), np.array([900.0, 900.0]))
    np.testing.assert_array_equal(a, b)


def _one_node(i):
    """one node per case, a different one from case to case, walking through energies, coszen and signs"""
    return i % 2, (i * 19 + 3) % T.N_NODES


def test_working_precision_does_not_matter(G):
    for i, c in enumerate(G["cases"]):
        s, n = _one_node(i)
        tab = G["earths"][c["earth"]]
        e, rho, dist = T.node_rows(tab)
        a = X.probabilities(*T.params_of(c), T.SIGNS[s], e[n], rho[n], dist[n], dps=40)
        b = X.probabilities(*T.params_of(c), T.SIGNS[s], e[n], rho[n], dist[n], dps=60)
        np.testing.assert_array_equal(a, b, err_msg=c["name"])


def test_committed_file_is_what_the_case_table_gives(G, oracle):
    """the stored parameter blocks, rows and Earth tables are those of `cases()` / `earth_tables()`, and one
    node per case recomputed has the stored bits"""
    cases = T.cases()
    assert [c["name"] for c in cases] == [c["name"] for c in G["cases"]] and len(cases) == 23
    earths = T.earth_tables(oracle, load_golden("layers_ref.npz"))
    for e in T.EARTHS:
        for k in earths[e]:
            np.testing.assert_array_equal(np.asarray(earths[e][k]), np.asarray(G["earths"][e][k]), err_msg=e + " " + k)
    np.testing.assert_array_equal(G["energy"], T.ENERGY)
    np.testing.assert_array_equal(G["coszen"], T.COSZEN)
    assert G["P_exact"].shape == (23, 2, T.N_NODES, 3, 3) and np.all(np.isfinite(G["P_exact"]))
    for i, (c, g) in enumerate(zip(cases, G["cases"])):
        assert c["earth"] == g["earth"]
        for k in T.PARAM_KEYS:
            np.testing.assert_array_equal(np.asarray(c[k]), np.asarray(g[k]), err_msg=c["name"] + " " + k)
        s, n = _one_node(i + 1)
        e, rho, dist = T.node_rows(earths[c["earth"]])
        P = X.probabilities(*T.params_of(c), T.SIGNS[s], e[n], rho[n], dist[n])
        np.testing.assert_array_equal(P, G["P_exact"][i, s, n], err_msg=c["name"])


def test_cases_reach_what_they_are_there_for(G):
    P = G["P_exact"]
    names = [c["name"] for c in G["cases"]]
    # the down-going column is P ~ 1 / P ~ 0 at high energy: measured by the absolute tolerance alone
    assert P[names.index("std_no"), 0, -1][0, 1] * PROB3_RTOL < PROB3_ATOL
    # decay loses probability, alpha3 = 0 with the flag on does not
    assert P[names.index("decay_1e-2")].sum(axis=-1).min() < 0.9
    np.testing.assert_allclose(P[names.index("decay_0")].sum(axis=-1), 1.0, rtol=0, atol=1e-14)
    # the Earth variants and the potentials move the probabilities
    for a, b in (("std_no", "std_no_equal"), ("std_no", "vacuum"), ("std_no", "lri_0"), ("std_no", "dm21_0")):
        assert np.abs(P[names.index(a)] - P[names.index(b)]).max() > 1e-3, (a, b)
    # both signs differ
    assert np.abs(P[:, 0] - P[:, 1]).max() > 0.1
    # three cases on the Earth whose cache hands a layer the matrix of another shell
    assert sum(c["earth"] == "prem12_equal" for c in G["cases"]) == 3
    # ... two of its shells share a density (the event kernel then resolves the cache in its staged form), as all
    # shells of the vacuum Earth do; the shells of the plain PREM-12 below the detector are pairwise distinct
    inner = slice(2, -1)          # (the production layer and the detector's own shell aside; the innermost two are one shell)
    assert len(set(G["earths"]["prem12"]["rhos"][inner])) == len(G["earths"]["prem12"]["rhos"][inner])
    assert len(set(G["earths"]["prem12_equal"]["rhos"][inner])) == len(G["earths"]["prem12_equal"]["rhos"][inner]) - 1
    assert not G["earths"]["vacuum"]["rhos"].any() and not G["earths"]["vacuum"]["density"].any()


def test_fp64_oracle_is_inside_the_gate_at_every_node(G, oracle):
    """the condition that makes the GPU gate legitimate: the reference's arithmetic in fp64 (the C oracle) stays
    inside rtol 1e-10 / atol 1e-14 of the exact values on all of these inputs, so no node is left out"""
    for i, c in enumerate(G["cases"]):
        e, rho, dist = T.node_rows(G["earths"][c["earth"]])
        worst = 0.0
        for s, nubar in enumerate(T.SIGNS):
            P = oracle.propagate_array(*T.params_of(c), nubar, e, rho, dist)
            worst = max(worst, T.gate_ratio(P, G["P_exact"][i, s], PROB3_RTOL, PROB3_ATOL).max())
        print("%-28s oracle err/gate %.3f" % (c["name"], worst))
        assert worst == G["oracle_over_gate"][i], c["name"]
        assert worst <= 1.0, c["name"]
