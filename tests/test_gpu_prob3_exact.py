"""Every prob3 kernel form against the EXACT layered propagator (oracle/exact_prob3.py: a 3x3 matrix
exponential per layer in 40-digit arithmetic, no closed forms), at every node of every case of
tests/prob3_exact_cases.py, under the reference's own gate (numba_osc_tests.py:82):

    assert_allclose(got, exact, rtol=PROB3_RTOL, atol=PROB3_ATOL)

No node, element, sign or case is left out or given a tolerance of its own.  What makes that gate the right
one for the device: the reference's arithmetic in fp64 (the C oracle) stays inside it on these very inputs
(`oracle_over_gate` of the golden file, <= 0.51; tests/test_host_prob3_exact.py measures it again).

The other prob3 tests compare the kernels with that oracle or with each other, i.e. with implementations
that share the closed-form eigenvalues, their conditioning and the Lagrange sum; this file reads only
tests/golden/prob3_exact_ref.npz (written by oracle/gen_prob3_exact.py) and needs no mpmath.

Every form is run ONCE per module (`run`); its gate test and the unitarity test read the same matrices.
Each test prints the worst err/gate = |got - exact| / (rtol |exact| + atol), or the worst |sum - 1|, per
form and case before it asserts.  Measured on an MI355X ("prob3 against exact values", has the table per
case): worst err/gate 0.093 propagate_array and prob3_grid, 0.083 planned, 0.053 planned_multi, 0.018 events and
events_multi -- the first three on decay cases; without decay no form exceeds 0.028; worst |row or column sum - 1|
4.9e-13.  Before the Lagrange sums were anchored on a member of the closest pair of eigenvalues (prob3_device.hpp:
layer_amplitude, eigen_terms) these tests gave 0.499 / 0.420 / 0.859 and 5.0e-11 / 3.2e-11 / 8.6e-11, all at 100 TeV.
"""
import ctypes as C

import numpy as np
import pytest

from tests import prob3_exact_cases as T
from tests.conftest import PROB3_ATOL, PROB3_RTOL

pytestmark = pytest.mark.gpu
AC = dict(rtol=PROB3_RTOL, atol=PROB3_ATOL)
UNITARITY = 1e-11


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


@pytest.fixture(scope="module")
def G(K, L):
    """the golden file, plus per Earth the device copies of what the kernels read and one plan"""
    g = T.load()
    np.testing.assert_array_equal(g["energy"], T.ENERGY)
    np.testing.assert_array_equal(g["coszen"], T.COSZEN)
    assert g["P_exact"].shape == (len(g["cases"]), 2, T.N_NODES, 3, 3)
    g["d_energy"] = K.to_device(g["energy"])
    g["d_ev_e"] = K.to_device(np.repeat(g["energy"], T.N_CZ))
    g["d_ev_cz"] = K.to_device(np.tile(g["coszen"], T.N_E))
    for tab in g["earths"].values():
        e, rho, dist = T.node_rows(tab)
        tab["d_density"], tab["d_distance"] = K.to_device(tab["density"]), K.to_device(tab["distance"])
        tab["d_node_density"], tab["d_node_distance"] = K.to_device(rho), K.to_device(dist)
        tab["plan"] = K.GridPlan(tab["d_density"], tab["d_distance"])
        tab["struct"] = L.make_earth(tab["radii"], tab["rhos"], tab["coszen_limit"], tab["r_detector"])
    for i, c in enumerate(g["cases"]):
        c["index"] = i
        c["params"] = L.make_prob3_params(*T.params_of(c))
        c["decay"] = c["decay_flag"] == 1
    return g


def _settle(entries):
    """prints the worst err/gate per form and case, then holds every entry to the gate"""
    worst = {}
    for form, case, sign, got, exact, _ in entries:
        r = T.gate_ratio(got, exact, PROB3_RTOL, PROB3_ATOL)
        key = (form, case["name"])
        worst[key] = max(worst.get(key, 0.0), float(np.where(np.isfinite(r), r, np.inf).max()))
    for form in sorted({k[0] for k in worst}):
        print("%-36s worst err/gate %.3f" % (form, max(v for k, v in worst.items() if k[0] == form)))
    for (form, name), v in worst.items():
        print("    %-36s %-28s err/gate %.3f" % (form, name, v))
    for form, case, sign, got, exact, _ in entries:
        np.testing.assert_allclose(got, exact, err_msg="%s, case %s, nubar %+d" % (form, case["name"], sign), **AC)


def _entry(form, case, sign, got, exact, matrices=True):
    got = np.asarray(got)
    assert got.shape == exact.shape, (form, case["name"], got.shape, exact.shape)
    return (form, case, sign, got, exact, matrices)


def _e_major(a, e_major):
    """[n_nodes][...] in the kernel's node order -> node = iE * N_CZ + jcz"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if e_major:
        return a
    tail = a.shape[1:]
    return np.ascontiguousarray(np.moveaxis(a.reshape((T.N_CZ, T.N_E) + tail), 0, 1)).reshape((T.N_NODES,) + tail)


def _tables(pepmu, e_major):
    """pepmu[2][3][n_nodes][2] -> [sign][node][init 0..1][flav], the layout of P_exact[:, :2, :]"""
    pm = pepmu.cpu().numpy() if hasattr(pepmu, "cpu") else np.asarray(pepmu)
    out = np.empty((2, T.N_NODES, 2, 3))
    for side in range(2):
        for f in range(3):
            out[side, :, :, f] = _e_major(pm[side, f], e_major)
    return out


# ------------------------------------------------------------------ the forms
def _propagate_array_rows_per_element(K, L, G):
    out = []
    for c in G["cases"]:
        tab = G["earths"][c["earth"]]
        for s, nubar in enumerate(T.SIGNS):
            got = K.propagate_array(c["params"], nubar, G["d_ev_e"], tab["d_node_density"], tab["d_node_distance"])
            out.append(_entry("propagate_array rows/element", c, nubar, got.cpu().numpy(), G["P_exact"][c["index"], s]))
    return out


def _propagate_array_shared_row(K, L, G):
    """the shared-row form, one coszen row at a time: the 8 energies of the row"""
    out = []
    for c in G["cases"]:
        tab = G["earths"][c["earth"]]
        for s, nubar in enumerate(T.SIGNS):
            got = np.empty((T.N_E, T.N_CZ, 3, 3))
            for j in range(T.N_CZ):
                got[:, j] = K.propagate_array(c["params"], nubar, G["d_energy"], tab["d_density"][j],
                                              tab["d_distance"][j]).cpu().numpy()
            out.append(_entry("propagate_array shared row", c, nubar, got.reshape(T.N_NODES, 3, 3), G["P_exact"][c["index"], s]))
    return out


def _propagate_array_host(K, L, G):
    """the numpy-in / numpy-out call, once: the case on which the fp64 oracle is closest to the gate"""
    c = G["cases"][int(np.argmax(G["oracle_over_gate"]))]
    e, rho, dist = (np.ascontiguousarray(a) for a in T.node_rows(G["earths"][c["earth"]]))
    got = np.full((T.N_NODES, 3, 3), np.nan)
    L.check(L.lib().pisa_hip_propagate_array_host(C.byref(c["params"]), -1, e.ctypes.data, rho.ctypes.data,
                                                  dist.ctypes.data, T.N_NODES, rho.shape[1], 1, got.ctypes.data))
    return [_entry("propagate_array_host", c, -1, got, G["P_exact"][c["index"], 1])]


def _grid_entries(form, c, e_major, nu, nubar, pepmu, G):
    form = "%s e_major=%d" % (form, e_major)
    tables = _tables(pepmu, e_major)
    out = []
    for s, (sign, got) in enumerate(((1, nu), (-1, nubar))):
        exact = G["P_exact"][c["index"], s]
        out.append(_entry(form, c, sign, _e_major(got, e_major), exact))
        out.append(_entry(form + " pepmu", c, sign, tables[s], exact[:, :2, :], matrices=False))
    return out


def _prob3_grid(K, L, G):
    out = []
    for c in G["cases"]:
        tab = G["earths"][c["earth"]]
        for e_major in (True, False):
            res = K.prob3_grid(c["params"], G["d_energy"], tab["d_density"], tab["d_distance"], e_major=e_major, want_pepmu=True)
            out += _grid_entries("prob3_grid", c, e_major, *res, G)
    return out


def _prob3_grid_planned(K, L, G):
    """one plan per Earth (the vacuum rows have one of their own), reused over the cases: matrices and tables"""
    out = []
    for c in G["cases"]:
        for e_major in (True, False):
            res = K.prob3_grid_planned(c["params"], G["earths"][c["earth"]]["plan"], G["d_energy"], e_major=e_major)
            out += _grid_entries("prob3_grid_planned", c, e_major, *res, G)
    return out


def _prob3_grid_planned_multi(K, L, G):
    """several parameter points in one pair of launches: per Earth the cases without decay in batches of up to
    MAX_POINTS points, the cases with decay in a batch of their own; every point against ITS exact tables"""
    import torch

    out, sizes = [], []
    for earth, tab in G["earths"].items():
        for decay in (False, True):
            group = [c for c in G["cases"] if c["earth"] == earth and c["decay"] == decay]
            for k in range(0, len(group), L.MAX_POINTS):
                batch = group[k:k + L.MAX_POINTS]
                n = len(batch)
                sizes.append(n)
                arr = (L.Prob3Params * n)()
                for i, c in enumerate(batch):
                    C.memmove(C.byref(arr[i]), C.byref(c["params"]), C.sizeof(L.Prob3Params))
                for e_major in (True, False):
                    buf = torch.full((2, 3, T.N_NODES, n, 2), float("nan"), dtype=torch.float64, device="cuda")
                    L.check(L.lib().pisa_hip_prob3_grid_planned_multi(
                        C.cast(arr, C.c_void_p), n, tab["plan"].handle, C.c_void_p(G["d_energy"].data_ptr()), T.N_E,
                        1 if e_major else 0, C.c_void_p(buf.data_ptr()), K._stream()))
                    pm = buf.cpu().numpy()
                    for i, c in enumerate(batch):
                        tables = _tables(pm[:, :, :, i, :], e_major)
                        for s, sign in enumerate(T.SIGNS):
                            out.append(_entry("prob3_grid_planned_multi e_major=%d" % e_major, c, sign, tables[s],
                                              G["P_exact"][c["index"], s][:, :2, :], matrices=False))
    assert sum(sizes) == len(G["cases"]) and max(sizes) > 8 and 1 in sizes     # a wide batch and the batch of one
    return out


def _prob3_events(K, L, G):
    """the events are the (E, coszen) nodes and the kernel rebuilds the layers from the Earth tables itself (its
    geometry is under test too): the direct form (prem12), the staged form (prem12_equal, vacuum), with and
    without a long-range potential, decay through layer_amplitude_decay_poly"""
    import torch

    out = []
    for c in G["cases"]:
        tab = G["earths"][c["earth"]]
        for s, nubar in enumerate(T.SIGNS):
            got = torch.full((T.N_NODES, 3, 3), float("nan"), dtype=torch.float64, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            L.check(L.lib().pisa_hip_prob3_events(
                C.byref(c["params"]), C.byref(tab["struct"]), nubar, C.c_void_p(G["d_ev_e"].data_ptr()),
                C.c_void_p(G["d_ev_cz"].data_ptr()), T.N_NODES, C.c_void_p(got.data_ptr()),
                C.c_void_p(status.data_ptr()), K._stream()))
            assert int(status.item()) == 0, (c["name"], nubar)
            out.append(_entry("prob3_events", c, nubar, got.cpu().numpy(), G["P_exact"][c["index"], s]))
    return out


def _prob3_events_multi(K, L, G):
    """both signs and the three flavours of a case as six event sets of ONE launch: full matrices from one set per
    sign, the (P_e, P_mu) pairs from all"""
    import torch

    out = []
    for c in G["cases"]:
        tab = G["earths"][c["earth"]]
        mats = {sign: torch.full((T.N_NODES, 3, 3), float("nan"), dtype=torch.float64, device="cuda") for sign in T.SIGNS}
        pairs = {(sign, f): torch.full((T.N_NODES, 2), float("nan"), dtype=torch.float64, device="cuda")
                 for sign in T.SIGNS for f in range(3)}
        sets = [L.EventSet(T.N_NODES, G["d_ev_e"].data_ptr(), G["d_ev_cz"].data_ptr(),
                           mats[sign].data_ptr() if f == 1 else None, pairs[sign, f].data_ptr(), sign, f)
                for sign in T.SIGNS for f in range(3)]
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        K.prob3_events_multi(c["params"], tab["struct"], sets, status)
        assert int(status.item()) == 0, c["name"]
        for s, sign in enumerate(T.SIGNS):
            exact = G["P_exact"][c["index"], s]
            out.append(_entry("prob3_events_multi", c, sign, mats[sign].cpu().numpy(), exact))
            got = np.stack([pairs[sign, f].cpu().numpy() for f in range(3)], axis=-1)     # [node][init 0..1][flav]
            out.append(_entry("prob3_events_multi pepmu", c, sign, got, exact[:, :2, :], matrices=False))
    return out


FORMS = {"propagate_array_rows_per_element": _propagate_array_rows_per_element,
         "propagate_array_shared_row": _propagate_array_shared_row,
         "propagate_array_host": _propagate_array_host,
         "prob3_grid": _prob3_grid,
         "prob3_grid_planned": _prob3_grid_planned,
         "prob3_grid_planned_multi": _prob3_grid_planned_multi,
         "prob3_events": _prob3_events,
         "prob3_events_multi": _prob3_events_multi}


@pytest.fixture(scope="module")
def run(K, L, G):
    """run(form): the entries of one form, computed at the first request"""
    done = {}

    def get(form):
        if form not in done:
            done[form] = FORMS[form](K, L, G)
        return done[form]

    return get


@pytest.mark.parametrize("form", list(FORMS))
def test_inside_the_gate_at_every_node(run, G, form):
    entries = run(form)
    if form != "propagate_array_host":           # every case, both signs
        assert {(e[1]["name"], e[2]) for e in entries} == {(c["name"], s) for c in G["cases"] for s in T.SIGNS}
    _settle(entries)


@pytest.mark.parametrize("form", [f for f in FORMS if f != "prob3_grid_planned_multi"])     # (that one writes tables only)
def test_rows_and_columns_sum_to_one_without_decay(run, form):
    """every full matrix a form returns, at every node of every case without decay: within 1e-11"""
    entries = [e for e in run(form) if e[5] and not e[1]["decay"]]
    assert entries
    worst = {}
    for name, case, sign, got, _, _ in entries:
        d = max(float(np.abs(got.sum(axis=-1) - 1.0).max()), float(np.abs(got.sum(axis=-2) - 1.0).max()))
        worst[name, case["name"]] = max(worst.get((name, case["name"]), 0.0), d if np.isfinite(d) else np.inf)
    for (name, cname), v in worst.items():
        print("    %-36s %-28s worst |row or column sum - 1| %.2e" % (name, cname, v))
    for name, case, sign, got, _, _ in entries:
        msg = "%s, case %s, nubar %+d" % (name, case["name"], sign)
        np.testing.assert_allclose(got.sum(axis=-1), 1.0, rtol=0, atol=UNITARITY, err_msg=msg + " (rows)")
        np.testing.assert_allclose(got.sum(axis=-2), 1.0, rtol=0, atol=UNITARITY, err_msg=msg + " (columns)")
