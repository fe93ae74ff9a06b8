"""The grow-on-demand device buffer of the trial-ensemble entry points (`DeviceScratch`, csrc/common.hpp): the
preparation buffers of the product form (csrc/ensemble.hip) and of the MC-uncertainty metrics (csrc/ensemble_mc.hip),
and the join buffer of the split reduced profiled form (csrc/profile.hip).

Each entry point is called at a small size, at a size that makes its buffer grow, and at the small size again.  The
first and the third result are equal bit for bit (the buffer that grew in between serves the small call as the first
one did), and the second lies within the gate of its `*_cases.py` module of that module's numpy restatement: G eps S
per entry, G = `g_of` of the kind and S the module's fp64 scale.

SMALL (3, 2, 5): no multiple of any tile, B no multiple of 4.  LARGE (70, 70, 37): more than one tile of 64, a ragged
last tile, more than one chunk of 32 bins.  The profiled call has J = 2 and so few trials that the templates of a strip
are split over workgroups at both sizes: the join buffer is in use.
"""
import numpy as np
import pytest

from tests import ensemble_cases as ec
from tests import ensemble_mc_cases as emc
from tests import profile_cases as pc

pytestmark = pytest.mark.gpu

SMALL, LARGE = (3, 2, 5), (70, 70, 37)
J = 2


def _dev(K, a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(K.device())


def _product_llh(K, shape):
    f = ec.family("poisson", *shape)
    got = K.metric_matrix("llh", _dev(K, f["D"]), _dev(K, f["E"]), form="product").cpu().numpy()
    return got, got, lambda: (ec.product_form("llh", f["D"], f["E"]), ec.scale_fp64("llh", f["D"], f["E"]),
                              ec.g_of("product", "llh"))


def _mcllh_eff(K, shape):
    f = emc.family(emc.family_of("mcllh_eff"), *shape)
    got = K.metric_matrix("mcllh_eff", _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["S2"])).cpu().numpy()
    return got, got, lambda: (emc.direct_form_mc("mcllh_eff", f["D"], f["E"], f["S2"]),
                              emc.scale_mc("mcllh_eff", f["D"], f["E"], f["S2"]), emc.g_of("mcllh_eff"))


def _profiled_chi2_best(K, shape):
    """the gate is applied to (best at the returned arg, at k0 = 1), the comparison of bits to all six outputs"""
    f = pc.family("poisson", *shape, J)
    out = K.profiled_metric_matrix_best("chi2", _dev(K, f["D"]), _dev(K, f["E"]), _dev(K, f["R"]), _dev(K, f["S2"]),
                                        _dev(K, f["ips"]), _dev(K, f["c"]), k0=1)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert not out["status"].any()
    rows = np.arange(shape[0])
    got = np.stack([out["best"], out["at"]], axis=1)

    def restated():
        full = pc.restated("chi2", f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"])
        _, scale = pc.exact_value("chi2", f["D"], f["E"], f["R"], f["S2"], full["eta"].astype(np.longdouble),
                                  f["ips"], f["c"])
        pick = lambda a: np.stack([a[rows, out["arg"]], a[:, 1]], axis=1)   # noqa: E731
        return pick(full["value"]), pick(scale), pc.g_of("chi2")

    bits = np.concatenate([out[k].astype(np.float64).reshape(shape[0], -1)
                           for k in ("best", "arg", "at", "eta_best", "eta_at", "status")], axis=1)
    return got, bits, restated


@pytest.mark.parametrize("entry", [_product_llh, _mcllh_eff, _profiled_chi2_best], ids=lambda f: f.__name__[1:])
def test_small_call_is_unchanged_by_a_call_that_grows_the_buffer(entry):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from pisa_amd import kernels as K

    # an entry -> (the values the gate is applied to, every output, the restatement of the former)
    _, first, _ = entry(K, SMALL)
    second, _, restated = entry(K, LARGE)
    _, third, _ = entry(K, SMALL)
    assert first.tobytes() == third.tobytes()
    want, scale, g = restated()
    worst = ec.check(second, want.astype(np.longdouble), scale, g, entry.__name__[1:])
    print("%s %s: worst %.3f eps S against the restatement (gate %.3g)" % (entry.__name__[1:], LARGE, worst, g))
