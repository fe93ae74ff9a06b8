"""The case table of the comparison of every prob3 kernel form with the exact layered propagator
(oracle/exact_prob3.py): shared by the generator (oracle/gen_prob3_exact.py), the host test
(tests/test_host_prob3_exact.py) and the GPU test (tests/test_gpu_prob3_exact.py).  A plain helper module
(no fixtures, numpy only): the generator and the host test build the cases from it, the GPU test reads
what the generator stored in tests/golden/prob3_exact_ref.npz.

Every case is one parameter block on one Earth, evaluated on the same small grid for both `nubar` signs:
8 energies x 7 coszen = 56 nodes per sign (a multiple of neither the wavefront nor the workgroup size),
node = iE * 7 + jcz.  The coszen cover the core (-1, -0.9), the neighbourhood of the core limit (-0.84; the
limit is -0.8375), the mantle only (-0.6, -0.2), the horizon (0) and a down-going path (0.6) whose P ~ 1
is measured by the absolute tolerance alone.

The gate is the reference's own (numba_osc_tests.py:82, `PROB3_RTOL`, `PROB3_ATOL` of tests/conftest.py):
|P - P_exact| <= 1e-10 |P_exact| + 1e-14, at every node, element, sign and case.
"""
import os

import numpy as np

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prob3_exact_ref.npz")

ENERGY = np.array([0.1, 0.37, 2.9, 6.1, 40.0, 1e3, 1e4, 1e5])
COSZEN = np.array([-1.0, -0.9, -0.84, -0.6, -0.2, 0.0, 0.6])
N_E, N_CZ = len(ENERGY), len(COSZEN)
N_NODES = N_E * N_CZ
SIGNS = (1, -1)

# the Earths: PREM-12 with the electron fractions and the detector depth of tests/golden/layers_ref.npz
# ("prem12"); the same with two mantle shells given one density, so that the reference's layer cache hands a
# layer the matrix of another shell and the event kernel takes its staged form ("prem12_equal", as in
# test_prob3_events_vs_oracle); the same geometry with every density zero ("vacuum")
EARTHS = ("prem12", "prem12_equal", "vacuum")

# the reference's standard values (settings/pipeline/osc_example.cfg and its inverted-ordering twin, as in
# oracle/gen_golden.py): angles in degrees
STD_NO = dict(theta12=33.48, theta13=8.5, theta23=42.0, deltacp=0.0, dm21=7.5e-5, dm31=2.457e-3)
STD_IO = dict(theta12=33.48, theta13=8.51, theta23=49.5, deltacp=254.0, dm21=7.5e-5, dm31=-2.374e-3)

STD_POT = np.diag([1.0, 0.0, 0.0]).astype(np.complex128)
ZERO_C = np.zeros((3, 3), np.complex128)
ZERO_R = np.zeros((3, 3), np.float64)

RANDOM_SEED = 1234      # test_reduced_form_against_reference_order_over_random_parameters draws with 77


def mix_matrix(theta12, theta13, theta23, deltacp):
    """osc_params.py:174-211, angles in rad (the reference keeps sin(theta) and takes c = sqrt(1 - s^2))"""
    s12, s13, s23 = np.sin(theta12), np.sin(theta13), np.sin(theta23)
    sd, cd = np.sin(deltacp), np.cos(deltacp)
    c12, c13, c23 = np.sqrt(1.0 - s12 ** 2), np.sqrt(1.0 - s13 ** 2), np.sqrt(1.0 - s23 ** 2)
    m = np.zeros((3, 3), np.complex128)
    m[0, 0] = c12 * c13
    m[0, 1] = s12 * c13
    m[0, 2] = s13 * cd - 1j * s13 * sd
    m[1, 0] = -s12 * c23 - c12 * s23 * s13 * cd - 1j * c12 * s23 * s13 * sd
    m[1, 1] = c12 * c23 - s12 * s23 * s13 * cd - 1j * s12 * s23 * s13 * sd
    m[1, 2] = s23 * c13
    m[2, 0] = s12 * s23 - c12 * c23 * s13 * cd - 1j * c12 * c23 * s13 * sd
    m[2, 1] = -c12 * s23 - s12 * c23 * s13 * cd - 1j * s12 * c23 * s13 * sd
    m[2, 2] = c23 * c13
    return m


def dm_matrix(dm21, dm31):
    """osc_params.py:265-292: an exactly zero splitting is moved by 5e-9 eV^2"""
    m = np.zeros(3)
    m[1], m[2] = dm21, dm31
    if m[1] == 0.0:
        m[0] -= 5.0e-9
    if m[2] == 0.0:
        m[2] += 5.0e-9
    return m[:, None] - m[None, :]


def _block(name, earth="prem12", angles_rad=None, mat_pot=STD_POT, decay_alpha3=None, lri_pot=ZERO_R, **osc):
    v = dict(STD_NO)
    v.update(osc)
    if angles_rad is None:
        angles_rad = [np.deg2rad(v[k]) for k in ("theta12", "theta13", "theta23", "deltacp")]
    mat_decay = ZERO_C.copy()
    if decay_alpha3 is not None:
        mat_decay[2, 2] = -1j * decay_alpha3            # prob3.py:559-563
    return dict(name=name, earth=earth, dm=dm_matrix(v["dm21"], v["dm31"]), mix=mix_matrix(*angles_rad),
                mat_pot=np.array(mat_pot, np.complex128), decay_flag=-1 if decay_alpha3 is None else 1,
                mat_decay=mat_decay, lri_pot=np.array(lri_pot, np.float64))


def cases():
    """the list of cases, each a dict: name, earth, dm, mix, mat_pot, decay_flag, mat_decay, lri_pot"""
    out = [
        # standard matter, no decay
        _block("std_no"),
        _block("std_io", **STD_IO),
        _block("std_no_equal", earth="prem12_equal"),
        _block("dm21_1e-6", dm21=1e-6),
        _block("dm21_1e-8", dm21=1e-8),
        _block("dm21_0", dm21=0.0),
        _block("theta13_0", theta13=0.0, deltacp=0.0),
        _block("angles_0", theta12=0.0, theta13=0.0, theta23=0.0, deltacp=0.0),
        _block("theta23_max_io", theta13=8.51, theta23=45.0, deltacp=0.0, dm31=-2.374e-3),
        # all densities zero: the matter eigenvalues must be matched to the vacuum ones
        _block("vacuum", earth="vacuum"),
    ]
    # random points by the recipe of test_reduced_form_against_reference_order_over_random_parameters
    rs = np.random.RandomState(RANDOM_SEED)
    for k in range(6):
        th = rs.rand(3) * np.pi / 2
        delta = rs.rand() * 2 * np.pi
        dm21 = 10 ** rs.uniform(-6, -3.5)
        dm31 = (1 if rs.rand() < 0.5 else -1) * 10 ** rs.uniform(-3.3, -2.2)
        pot = STD_POT
        if k % 2 == 1:                                   # Hermitian NSI
            a = (rs.randn(3, 3) + 1j * rs.randn(3, 3)) * 0.2
            pot = STD_POT + (a + a.conj().T) / 2
        out.append(_block("random_%d%s" % (k, "_nsi" if k % 2 == 1 else ""), angles_rad=[th[0], th[1], th[2], delta],
                          mat_pot=pot, dm21=dm21, dm31=dm31))
    # long-range potentials: real symmetric, of order 1e-13 eV
    for k, earth in enumerate(("prem12", "prem12_equal")):
        b = rs.randn(3, 3) * 1e-13
        out.append(_block("lri_%d%s" % (k, "_equal" if k else ""), earth=earth, lri_pot=(b + b.T) / 2))
    # decay, mat_decay = diag(0, 0, -i alpha3): the (nearly) degenerate ones put the Lagrange and the Newton
    # form of layer_amplitude_decay_poly into one wavefront (atmosphere / vacuum layers against mantle layers)
    out += [
        _block("decay_1e-4", decay_alpha3=1e-4),
        _block("decay_1e-4_dm21_0", decay_alpha3=1e-4, dm21=0.0),
        _block("decay_1e-4_dm21_1e-7_equal", earth="prem12_equal", decay_alpha3=1e-4, dm21=1e-7),
        _block("decay_1e-2", decay_alpha3=1e-2),
        _block("decay_0", decay_alpha3=0.0),
    ]
    return out


PARAM_KEYS = ("dm", "mix", "mat_pot", "decay_flag", "mat_decay", "lri_pot")


def params_of(case):
    """the six leading arguments of `propagate_array` / `make_prob3_params`"""
    return [case[k] for k in PARAM_KEYS]


def earth_tables(oracle, layers_golden):
    """{earth: dict(radii, rhos, coszen_limit, r_detector, density[n_cz][L], distance[n_cz][L])} from
    `oracle.Layers` (the CPU oracle's restatement of layers.py) on COSZEN"""
    g = layers_golden
    depth, height, yi, yo, ym = g["prem12::args"]
    out = {}
    for earth in EARTHS:
        prem = np.array(g["prem12::prem"], dtype=np.float64, copy=True)
        if earth == "prem12_equal":
            prem[6, 1] = prem[7, 1]
        if earth == "vacuum":
            prem[:, 1] = 0.0
        lay = oracle.Layers(prem, depth, height)
        lay.setElecFrac(yi, yo, ym)
        lay.calcLayers(COSZEN)
        out[earth] = dict(radii=np.array(lay.radii), rhos=np.array(lay.rhos), coszen_limit=np.array(lay.coszen_limit),
                          r_detector=float(lay.r_detector), density=np.array(lay.density), distance=np.array(lay.distance))
    return out


def node_rows(table):
    """per-node (energy[n], density[n][L], distance[n][L]) of one Earth, node = iE * N_CZ + jcz"""
    return (np.repeat(ENERGY, N_CZ), np.tile(table["density"], (N_E, 1)), np.tile(table["distance"], (N_E, 1)))


def gate_ratio(got, exact, rtol, atol):
    """|got - exact| / (rtol |exact| + atol), elementwise: <= 1 is what assert_allclose(rtol, atol) asks"""
    return np.abs(got - exact) / (rtol * np.abs(exact) + atol)


def load():
    """the committed golden file as a dict of arrays, the cases rebuilt as the list `cases()` gives"""
    g = np.load(GOLDEN_FILE, allow_pickle=False)
    d = {k: g[k] for k in g.files}
    names = [str(s) for s in d["case_names"]]
    earths = [str(s) for s in d["earth_names"]]
    d["cases"] = [dict(name=n, earth=earths[int(d["case_earth"][i])], dm=d["dm"][i], mix=d["mix"][i],
                       mat_pot=d["mat_pot"][i], decay_flag=int(d["decay_flag"][i]), mat_decay=d["mat_decay"][i],
                       lri_pot=d["lri_pot"][i]) for i, n in enumerate(names)]
    d["earths"] = {e: dict(radii=d["earth_radii"][k], rhos=d["earth_rhos"][k], coszen_limit=d["earth_coszen_limit"][k],
                           r_detector=float(d["earth_r_detector"][k]), density=d["density"][k], distance=d["distance"][k])
                   for k, e in enumerate(earths)}
    return d
