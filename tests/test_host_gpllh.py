"""CPU checks of the generalized Poisson-gamma likelihood: the goldens (tests/golden/gpllh_ref.npz, written by
scripts/dev/gen_gpllh_golden.py from the reference's own eq. 91 code) against an independent restatement of eq. 91
in 40-digit arithmetic, the C-ABI surface, and the argument checks that run before any device call."""
import ctypes
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gpllh_ref.npz")
NEW = ("pisa_hip_gpllh_bin_sums", "pisa_hip_gpllh_params", "pisa_hip_generalized_poisson_llh",
       "pisa_hip_finalize_gpllh")


def eq91(k, alphas, betas):
    """arXiv:1902.08831 eq. 91 in 40-digit arithmetic"""
    import mpmath as mp

    with mp.workdps(40):
        a = [mp.mpf(float(x)) for x in alphas]
        b = [mp.mpf(float(x)) for x in betas]
        prefac = mp.mpf(1)
        for ai, bi in zip(a, b):
            prefac *= (bi / (1 + bi)) ** ai
        r = [1 / (1 + bi) for bi in b]
        s = [mp.mpf(0)] + [mp.fsum(ai * ri ** i for ai, ri in zip(a, r)) for i in range(1, k + 1)]
        d = [mp.mpf(1)]
        for i in range(1, k + 1):
            d.append(mp.fsum(s[j] * d[i - j] for j in range(1, i + 1)) / i)
        return prefac * d[k]


def test_goldens_agree_with_an_independent_eq91():
    g = np.load(GOLDEN)
    checked = 0
    for name in g["cases"]:
        ret, branch, data = g[name + "__ret"], g[name + "__branch"], g[name + "__data"]
        a, b, per_bin = g[name + "__alpha"], g[name + "__beta"], g[name + "__per_bin"]
        for i in np.flatnonzero(branch == 2):
            k = int(data[i])
            m = np.isfinite(a[:, i]) & np.isfinite(b[:, i])
            want = eq91(k, a[m, i], b[m, i])
            if np.isnan(ret[i]):       # prefac underflowed to 0 and delta_k overflowed: fast_pgmix gives +1
                assert per_bin[i] == 1.0
                continue
            if want > 1e-290:
                assert abs(float(want) - ret[i]) <= 1e-12 * float(want), (name, i, k, float(want), ret[i])
            else:
                assert ret[i] <= 1e-290 and per_bin[i] == np.log(1e-300)
            checked += 1
    assert checked > 100


def test_goldens_cover_every_branch_and_rule():
    g = np.load(GOLDEN)
    names = list(g["cases"])
    pb = np.concatenate([g[n + "__per_bin"] for n in names])
    br = np.concatenate([g[n + "__branch"] for n in names])
    k = np.concatenate([g[n + "__data"] for n in names])
    assert set(br.tolist()) == {0, 1, 2}
    assert np.any(pb == 1.0) and np.any(pb == np.log(1e-300)) and np.any(pb == np.log(1e-10))
    assert k.max() > 2000 and np.any((br == 1) & (k == 0))
    assert any(np.any(g[n + "__adjust"] != 0) for n in names)
    assert any(np.any(g[n + "__n_mc"] == 0) for n in names)          # pseudo-weights
    assert max(g[n + "__n_mc"].shape[0] for n in names) == 16


def test_new_symbols_in_header_library_and_binding():
    import __graft_entry__ as ge

    ge.build()
    from pisa_amd import _lib

    header = open(os.path.join(ROOT, "include", "pisa_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert "#define PISA_HIP_METRIC_GENERALIZED_POISSON_LLH 9" in header
    from pisa_amd import kernels as K

    assert K.GPLLH_KIND == 9 and "generalized_poisson_llh" not in K.METRIC_KIND


def test_wrong_expected_values_raise_before_any_device_call(monkeypatch):
    from pisa_amd import kernels as K
    from pisa_amd.utils import stats

    def no_device(*a, **k):
        raise AssertionError("device touched")

    monkeypatch.setattr(K, "to_device", no_device)
    monkeypatch.setattr(K, "generalized_poisson_llh", no_device)
    data = np.ones(4)
    with pytest.raises(TypeError):
        stats.generalized_poisson_llh(data, {"weights": None})
    with pytest.raises(KeyError):
        stats.generalized_poisson_llh(data, OrderedDict(weights=None, llh_alphas=None, llh_betas=None))
    with pytest.raises(TypeError):
        stats.generalized_poisson_llh(data, OrderedDict(weights=1, llh_alphas=1, llh_betas=1, n_mc_events=1))
    # ALL_METRICS and Map.metric keep rejecting the name (it is a method of its own, as in the reference)
    from pisa_amd.core.map import ALL_METRICS

    assert "generalized_poisson_llh" not in stats.ALL_METRICS and "generalized_poisson_llh" not in ALL_METRICS


def test_event_lists_and_mean_adjustment():
    from pisa_amd.stages.likelihood.generalized_llh_params import event_lists, mean_adjustment

    masks = [np.array([1, 0, 0, 1]), np.array([0, 2, 0, 0]), np.zeros(4, dtype=np.int64)]
    index, offsets, disjoint = event_lists(masks)
    assert disjoint and index.tolist() == [0, 3, 1] and offsets.tolist() == [0, 2, 3, 3]
    index, offsets, disjoint = event_lists([np.ones(3), np.ones(3)])
    assert not disjoint and index.tolist() == [0, 1, 2, 0, 1, 2] and offsets.tolist() == [0, 3, 6]
    assert mean_adjustment(np.array([0.0, 1.0])) == -(1.0 - 0.5) + 1e-3
    assert mean_adjustment(np.array([1.0, 3.0])) == 0.0
