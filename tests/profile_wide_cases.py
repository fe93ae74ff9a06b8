"""Shared pieces of the tests of the WIDE form of the profiled trial ensembles (csrc/profile_wide_device.hpp,
csrc/profile_wide.hip: `pisa_hip_profiled_metric_matrix_wide`, `..._best_wide`; DESIGN.md §4, "Profiled trial
ensembles: more than 8 parameters") and of the `wide=` paths of pisa_amd/analysis/ensemble.py.  A plain helper module:
the families, the restatements (`profile_cases.solve`, `profile_bounded_cases.solve_bounded`: generic in J, they ARE the
definition of the wide form), the exact references and the gate helpers are imported unchanged; this file adds the
shapes and boxes that cross the edges of the wide mapping, and the measured constants of its gate.

Shapes are (T, K, B, J).  The wide kernel takes one pair per wavefront (T edge: 1 and 2), the bins in chunks of 64
(B edge: 63 / 64 / 65 and 130), the Hessian in 4 x 4 tiles (J edges 1, 8, 9, 16, 17, 31, 32 fill the last tile row
fully, by one and by three), and splits the templates of the reduced output into ranges (K edge: 300 templates).

The gate is the project's: |got - exact| <= G eps S, G = 4 max(1, G_REF_W[kind]) unbounded and
4 max(1, G_REF_WB[kind]) bounded, with the worst ratios of the numpy restatements against the longdouble reference over
the gated wide cases, measured on the CPU by tests/test_host_profiled_wide.py and held against the constants below,
never taken from the device.  Every gated case has status 0 on every pair in the restatement and in the reference
(asserted there).  UNGATED cases are compared as the status families are: status, n_iter and eta with `==` against the
restatement, the value inside the gate around the exact value at the returned eta.

Measured (numpy 2.2): unbounded 0.451 (llh), 0.559 (poisson_llh), 0.833 (chi2), 0.814 (mod_chi2); bounded 0.128, 0.294,
0.405, 0.515: G = 4 for every kind in both forms.  At most 8 Newton steps on any gated pair (MOST_STEPS; max_iter is
32), and every pair of the bounded cases ends with a coordinate on a bound.
"""
import numpy as np

from tests import metric_cases as mc
from tests import profile_bounded_cases as pbc
from tests import profile_cases as pc

MAX_PARAMS = 32
CHUNK = 64                     # PFW_CHUNK: bins per chunk
MAX_ITER = pc.MAX_ITER

# (family, shape): every pair ends with status 0
GATED = (
    ("poisson", (2, 2, 65, 1)),            # J = 1: one tile, three of its four rows empty
    ("poisson", (3, 2, 65, 8)), ("prior", (3, 2, 65, 8)),
    ("poisson", (1, 1, 1, 9)),             # B = 1 with priors on every parameter; T = K = 1
    ("poisson", (2, 3, 3, 9)),             # B = 3 < J
    ("poisson", (3, 2, 40, 9)), ("prior", (3, 2, 40, 9)),
    ("poisson", (3, 2, 64, 16)), ("prior", (3, 2, 64, 16)),
    ("poisson", (2, 3, 63, 17)), ("prior", (2, 3, 63, 17)),
    ("poisson", (2, 2, 65, 31)), ("prior", (2, 2, 65, 31)),
    ("poisson", (2, 2, 130, 32)), ("prior", (2, 2, 130, 32)),
    ("poisson", (8, 300, 12, 12)),         # many templates: the ranges of the reduced output
)
# J > B without a prior on every parameter: the restatement reports NOT_POSDEF on some pairs
UNGATED = (("prior", (66, 2, 20, 32)),)
# (family, box of profile_bounded_cases, shape)
GATED_BOUNDED = (
    ("poisson", "wide", (3, 2, 64, 16)), ("prior", "wide", (3, 2, 64, 16)),
    ("poisson", "narrow", (3, 2, 64, 16)), ("prior", "lower", (3, 2, 64, 16)),
    ("poisson", "narrow", (3, 2, 40, 9)), ("prior", "lower", (3, 2, 40, 9)),
    ("poisson", "lower", (2, 3, 63, 17)),
    ("poisson", "wide", (2, 2, 130, 32)), ("prior", "narrow", (2, 2, 130, 32)),
)

# worst ratio of the fp64 restatements against the exact reference over GATED / GATED_BOUNDED (module docstring)
G_REF_W = {"llh": 0.46, "poisson_llh": 0.56, "chi2": 0.84, "mod_chi2": 0.82}
G_REF_WB = {"llh": 0.13, "poisson_llh": 0.30, "chi2": 0.41, "mod_chi2": 0.52}
MOST_STEPS = 8


def g_of(kind, bounded=False):
    return mc.KERNEL_FACTOR * max(1.0, (G_REF_WB if bounded else G_REF_W)[kind])


def pinned(K, J):
    """the box lower = upper = 0 on every parameter"""
    return np.zeros(J), np.zeros(J)


_RESTATED = {}


def restated(fam, kind, shape, bx=None):
    """the restatement's outputs of a case (`bx`: None, a box of profile_bounded_cases, or "pinned"): computed once,
    shared, read-only"""
    key = (fam, kind, shape, bx)
    if key not in _RESTATED:
        f = pc.family(fam, *shape)
        if bx is None:
            out = pc.restated(kind, f["D"], f["E"], f["R"], f["S2"], f["ips"], f["c"])
        else:
            lower, upper = bounds(bx, shape[1], shape[3])
            out = pbc.restated_bounded(kind, f["D"], f["E"], f["R"], lower, upper, f["S2"], f["ips"], f["c"])
        for v in out.values():
            v.setflags(write=False)
        _RESTATED[key] = out
    return _RESTATED[key]


def bounds(bx, K, J):
    return pinned(K, J) if bx == "pinned" else pbc.box(bx, K, J)
