"""The join of the packed prob3 chain kernel (pisa_amd/csrc/prob3_planned.hip: a row's R parts multiplied by its leader,
its L parts by the next wave, `L . (T . R)` behind a second barrier) changes no product and no association: every table
is, byte for byte, what the library of the commit before the two-sided join wrote on the MI355X.

n_cz = 20 over [-1, 1] on PREM 12: rows of >= 14 crossed layers (four waves), shorter rows (two waves) and the ten-row
down-going class.  n_e = 8: only a ragged tile; 64: only a full tile; 72: both.

The expectation is tests/golden/prob3_join_parent.npz, written by scripts/dev/record_prob3_join.py (which takes the
library to record from): the gather tables of n_e = 8 and 72 as arrays, SHA-256 digests of every other table, and the
compiler's version line."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N_CZ = 20
N_ES = (8, 64, 72)
NAMES = ("no", "io", "decay")
MULTI = ("no", "io", "no")      # one kernel variant per batch: no decay point beside the others
STORED_N_E = (8, 72)            # gather tables kept as arrays; everything else as a digest
FIXTURE = "prob3_join_parent.npz"
T4 = 14                         # crossed layers from which a row gets four waves (Prob3PackOpts::t4; below: two)


def energies(n):
    return np.logspace(0.0, np.log10(80.0), 128)[:n]    # tests/test_gpu_prob3_pack.py's


def make_setup(K, oracle):
    from pisa_amd import _lib
    from pisa_amd.utils.resources import find_resource

    edges = np.linspace(-1.0, 1.0, N_CZ + 1)
    lay = oracle.Layers(np.loadtxt(find_resource("osc/PREM_12layer.dat")), 2.0, 20.0)
    lay.setElecFrac(0.4656, 0.4656, 0.4957)
    lay.calcLayers(0.5 * (edges[1:] + edges[:-1]))
    distance = np.asarray(lay.distance, dtype=float).reshape(N_CZ, -1)
    dens = K.to_device(np.asarray(lay.density, dtype=float).reshape(N_CZ, -1))
    dist = K.to_device(distance)
    g = load_golden("prob3_grid_prem12.npz")
    params = {name: _lib.make_prob3_params(g[name + "::dm"], g[name + "::mix"], g[name + "::mat_pot"], int(g[name + "::decay_flag"]),
                                           g[name + "::mat_decay"], g[name + "::lri_pot"]) for name in NAMES}
    return dict(plan=K.GridPlan(dens, dist), params=params, crossed=(distance > 0.0).sum(axis=1))


def one_point(K, setup, name, n_e, e_major):
    """{key: array} of pisa_hip_prob3_grid_planned; the outputs start as NaN, so a node that is not written shows"""
    e = K.to_device(energies(n_e))
    n = n_e * N_CZ
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=e.device)
    nu, nubar, pepmu = K.prob3_grid_planned(setup["params"][name], setup["plan"], e, e_major=e_major, out_nu=nan(n, 3, 3),
                                            out_nubar=nan(n, 3, 3), out_pepmu=nan(2, 3, n, 2))
    key = "%s/%d/%d/" % (name, n_e, e_major)
    return {key + "nu": nu.cpu().numpy(), key + "nubar": nubar.cpu().numpy(), key + "pepmu": pepmu.cpu().numpy()}


def three_points(K, setup, n_e, e_major):
    """{key: array} of pisa_hip_prob3_grid_planned_multi with the points MULTI: tables [sign][flavour][node][point][2]"""
    from pisa_amd import _lib

    e = K.to_device(energies(n_e))
    arr = (_lib.Prob3Params * 3)()
    for i, n in enumerate(MULTI):
        arr[i] = setup["params"][n]
    tables = torch.full((2, 3, n_e * N_CZ, 3, 2), float("nan"), dtype=torch.float64, device=e.device)
    _lib.check(_lib.lib().pisa_hip_prob3_grid_planned_multi(C.cast(arr, C.c_void_p), 3, setup["plan"].handle, C.c_void_p(e.data_ptr()),
                                                            n_e, 1 if e_major else 0, C.c_void_p(tables.data_ptr()), K._stream()))
    return {"multi/%d/%d/pepmu" % (n_e, e_major): tables.cpu().numpy()}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def to_fixture(tables):
    """what the fixture keeps of {key: array}"""
    out = {}
    for key, a in tables.items():
        name, n_e, _, what = key.split("/")
        if what == "pepmu" and name != "multi" and int(n_e) in STORED_N_E:
            out[key] = a
        else:
            out[key + ":sha256"] = np.array(digest(a))
    return out


def toolchain():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        lines = subprocess.run([hipcc, "--version"], capture_output=True, text=True, timeout=60).stdout.splitlines()
    except (OSError, subprocess.TimeoutExpired):
        return "unknown"
    return next((ln.strip() for ln in lines if "HIP version" in ln), lines[0].strip() if lines else "unknown")


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def setup(K, oracle):
    return make_setup(K, oracle)


@pytest.fixture(scope="module")
def golden():
    return load_golden(FIXTURE)


def check(tables, golden):
    bad = []
    for key, want in to_fixture(tables).items():
        assert key in golden.files, key
        got = golden[key]
        same = (str(got) == str(want)) if key.endswith(":sha256") else (got.shape == want.shape and got.tobytes() == want.tobytes())
        if not same:
            bad.append(key)
    if bad:
        recorded, here = str(golden["toolchain"]), toolchain()
        note = "" if recorded == here else (
            "  The fixture was recorded from a library built by another toolchain (%r, here %r): build the commit before the "
            "two-sided join with this toolchain and run scripts/dev/record_prob3_join.py on its library." % (recorded, here))
        pytest.fail("tables differ from the recorded ones: %s.%s" % (", ".join(bad), note))


@pytest.mark.parametrize("e_major", [True, False])
@pytest.mark.parametrize("n_e", N_ES)
@pytest.mark.parametrize("name", NAMES)
def test_one_point_tables_are_the_recorded_bytes(K, setup, golden, name, n_e, e_major):
    tables = one_point(K, setup, name, n_e, e_major)
    assert all(np.isfinite(a).all() for a in tables.values())
    check(tables, golden)


@pytest.mark.parametrize("e_major", [True, False])
@pytest.mark.parametrize("n_e", N_ES)
def test_three_point_tables_are_the_recorded_bytes(K, setup, golden, n_e, e_major):
    tables = three_points(K, setup, n_e, e_major)
    (key, t), = tables.items()
    assert np.isfinite(t).all()
    check(tables, golden)
    # and per point the recorded one-point table
    for i, name in enumerate(MULTI):
        one = "%s/%d/%d/pepmu" % (name, n_e, e_major)
        if one in golden.files:
            assert t[:, :, :, i, :].tobytes() == golden[one].tobytes(), (name, i)
        else:
            assert digest(t[:, :, :, i, :]) == str(golden[one + ":sha256"]), (name, i)
    assert t[:, :, :, 0, :].tobytes() != t[:, :, :, 1, :].tobytes()


def test_the_grid_has_rows_of_four_and_of_two_waves(setup, golden):
    crossed = setup["crossed"]
    print("crossed layers per row:", crossed.tolist())
    assert (crossed >= T4).any(), "no row of four waves"
    assert ((crossed > 0) & (crossed < T4)).any(), "no row of two waves"
    # the down-going class: ten rows that cross the same few layers
    assert (crossed == crossed.min()).sum() >= 10
    # the fixture is the whole set of cases
    assert len(golden.files) == 1 + 3 * len(NAMES) * len(N_ES) * 2 + len(N_ES) * 2
