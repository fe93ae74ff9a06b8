"""The packed chain launch of the planned prob3 grid where an energy tile is ragged (pisa_amd/csrc/prob3_plan.hpp: the
rows of one class side by side in the lanes of a wave, longest rows first): against the
one-kernel grid form at the tolerance of the planned-form tests, node for node against the same energies on full
tiles, and the several-point launch against the one-point one.

n_cz = 20 over [-1, 1] on PREM 12: a ten-row down-going class (groups of 8 + 2 at n_e = 8 and 72) and classes of one
row.  n_e = 8: only a ragged tile; 72: the smallest grid with a full and a ragged tile (r = 8); 96: r = 32, two rows
per wave; 97: r = 33, no packing."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
N_CZ = 20
PLANNED_ATOL = 3e-13    # tests/test_gpu_kernels.py::test_prob3_grid_planned


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def setup(K, oracle):
    from pisa_amd import _lib
    from pisa_amd.utils.resources import find_resource

    edges = np.linspace(-1.0, 1.0, N_CZ + 1)
    lay = oracle.Layers(np.loadtxt(find_resource("osc/PREM_12layer.dat")), 2.0, 20.0)
    lay.setElecFrac(0.4656, 0.4656, 0.4957)
    lay.calcLayers(0.5 * (edges[1:] + edges[:-1]))
    dens = K.to_device(np.asarray(lay.density, dtype=float).reshape(N_CZ, -1))
    dist = K.to_device(np.asarray(lay.distance, dtype=float).reshape(N_CZ, -1))
    g = load_golden("prob3_grid_prem12.npz")
    params = {name: _lib.make_prob3_params(g[name + "::dm"], g[name + "::mix"], g[name + "::mat_pot"], int(g[name + "::decay_flag"]),
                                           g[name + "::mat_decay"], g[name + "::lri_pot"]) for name in ("no", "io", "decay")}
    return dict(dens=dens, dist=dist, plan=K.GridPlan(dens, dist), params=params)


def _energies(n):
    return np.logspace(0.0, np.log10(80.0), 128)[:n] if n <= 128 else np.logspace(0.0, np.log10(80.0), n)


@pytest.mark.parametrize("name", ["no", "decay"])
@pytest.mark.parametrize("n_e", [8, 72, 96, 97])
def test_packed_grid_against_the_one_kernel_form(K, setup, n_e, name):
    e = K.to_device(_energies(n_e))
    p = setup["params"][name]
    for e_major in (True, False):
        nu, nubar, pepmu = K.prob3_grid(p, e, setup["dens"], setup["dist"], e_major=e_major, want_pepmu=True)
        nu2, nubar2, pepmu2 = K.prob3_grid_planned(p, setup["plan"], e, e_major=e_major)
        worst = [float((a - b).abs().max()) for a, b in ((nu, nu2), (nubar, nubar2), (pepmu, pepmu2))]
        print("n_e %d %s e_major %d: largest differences nu %.3g nubar %.3g tables %.3g" % (n_e, name, e_major, *worst))
        assert all(bool(torch.isfinite(t).all()) for t in (nu2, nubar2, pepmu2))
        assert max(worst) < PLANNED_ATOL
        # not vacuous: the oscillogram has structure and every row sums to one without decay
        assert float(nu2.max() - nu2.min()) > 0.5
        if name == "no":
            assert float((nu2.sum(dim=2) - 1.0).abs().max()) < 1e-12


@pytest.mark.parametrize("name", ["no", "decay"])
def test_a_node_does_not_depend_on_its_lane(K, setup, name):
    """the 72 energies as a full tile + a ragged tile of 8 (eight rows per wave), and as the first 72 of 128 energies
    (two full tiles, a row per wave): the same arithmetic per lane, so the same bits"""
    p = setup["params"][name]
    e128 = _energies(128)
    out72 = K.prob3_grid_planned(p, setup["plan"], K.to_device(e128[:72]), e_major=True)
    out128 = K.prob3_grid_planned(p, setup["plan"], K.to_device(e128), e_major=True)
    for a, b, tail in ((out72[0], out128[0], (3, 3)), (out72[1], out128[1], (3, 3))):
        a, b = a.reshape(72, N_CZ, *tail), b.reshape(128, N_CZ, *tail)[:72]
        diff = float((a - b).abs().max())
        print("%s: largest difference between the packed and the full-tile node %.3g" % (name, diff))
        assert diff < PLANNED_ATOL
        assert bool((a == b).all())
    ta, tb = out72[2].reshape(2, 3, 72, N_CZ, 2), out128[2].reshape(2, 3, 128, N_CZ, 2)[:, :, :72]
    assert bool((ta == tb).all())


def test_several_points_on_a_ragged_tile(K, setup):
    """three points in one launch at n_e = 72: per point the tables of the one-point launch, bit for bit"""
    from pisa_amd import _lib

    e = K.to_device(_energies(72))
    names = ("no", "io", "no")
    arr = (_lib.Prob3Params * 3)()
    for i, n in enumerate(names):
        arr[i] = setup["params"][n]
    tables = torch.full((2, 3, 72 * N_CZ, 3, 2), float("nan"), dtype=torch.float64, device=e.device)
    _lib.check(_lib.lib().pisa_hip_prob3_grid_planned_multi(C.cast(arr, C.c_void_p), 3, setup["plan"].handle, C.c_void_p(e.data_ptr()),
                                                            72, 1, C.c_void_p(tables.data_ptr()), K._stream()))
    for i, n in enumerate(names):
        _, _, one = K.prob3_grid_planned(setup["params"][n], setup["plan"], e, e_major=True)
        assert bool((tables[:, :, :, i, :] == one).all()), n
    assert not bool((tables[:, :, :, 0, :] == tables[:, :, :, 1, :]).all())
