"""The case table of the production-height average of the prob3 kernels ("Production-height averaging"):
shared by the generator (scripts/dev/gen_prob3_avg_golden.py), the host test (tests/test_host_prob3_avg.py) and the
GPU tests (tests/test_gpu_prob3_avg.py).  A plain helper module (no fixtures, numpy only): the generator builds the
cases from it, the tests read what the generator stored in tests/golden/prob3_avg_exact.npz.

A case is one parameter block with one averaging range on the 12-layer PREM of tests/golden/layers_ref.npz (detector
depth 2 km, production height 20 km), evaluated for both `nubar` signs on 5 energies x 7 coszen, node = iE * 7 + jcz.
Per coszen the first traversed layer (the atmosphere, electron density 0) has the length Lbar = (L_min + L_max) / 2 and
the range dL = L_max - L_min, L_min / L_max being its lengths at production heights 20 -+ range / 2; every other layer
is the nominal row's.  The golden value of a node is the QUADRATURE of the exact layered probability over the first
layer's length (oracle/exact_prob3.py, 40 digits), not the closed form that the kernels and `closed_form` below use.

The gate is the project's number for an fp64 prob3 form against exact values (include/pisa_hip.h,
tests/test_gpu_prob3_exact.py): 1e-11 absolute.
"""
import os

import numpy as np

from tests import prob3_exact_cases as X

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prob3_avg_exact.npz")

ENERGY = np.array([0.1, 0.37, 2.9, 40.0, 1000.0])
COSZEN = np.array([-1.0, -0.6, -0.05, 0.0, 0.05, 0.6, 1.0])
N_E, N_CZ = len(ENERGY), len(COSZEN)
N_NODES = N_E * N_CZ
SIGNS = (1, -1)
DETECTOR_DEPTH, PROP_HEIGHT = 2.0, 20.0
RANGES = (10.0, 38.0)           # km of production height
GATE = 1e-11

HBAR_C_FACTOR = 2.534
TWORTTWOGF = 1.52588e-4


def _nsi_pot():
    """one standard-NSI block: the standard potential plus a Hermitian matrix of entries ~0.2"""
    rs = np.random.RandomState(4321)
    a = (rs.randn(3, 3) + 1j * rs.randn(3, 3)) * 0.2
    return X.STD_POT + (a + a.conj().T) / 2


def blocks():
    """the parameter blocks: STD_NO, STD_IO and one with standard NSI (dicts as prob3_exact_cases._block gives)"""
    return [X._block("std_no"), X._block("std_io", **X.STD_IO), X._block("std_no_nsi", mat_pot=_nsi_pot())]


def cases():
    """[(block, range index)]: every block with every range"""
    return [(b, r) for b in blocks() for r in range(len(RANGES))]


def midpoint_rows(density, dist_nom, dist_lo, dist_hi):
    """rows with the first traversed layer at Lbar, Lbar[n], dL[n], the layer's index [n]: the numpy statement of
    what `Layers.height_average_rows` returns (pisa_amd/stages/osc/layers.py)"""
    density, dist_nom = np.asarray(density, np.float64), np.asarray(dist_nom, np.float64)
    first = np.argmax(dist_nom > 0.0, axis=1)
    rows = np.arange(len(dist_nom))
    lmin, lmax = np.asarray(dist_lo)[rows, first], np.asarray(dist_hi)[rows, first]
    lbar = 0.5 * (lmin + lmax)
    dist = dist_nom.copy()
    dist[rows, first] = lbar
    return dist, lbar, lmax - lmin, first


def chain_product(block, nubar, energy, density, distance):
    """(U, T): the side's mixing matrix and the mass-basis chain product T = A_last .. A_first of one row in fp64
    (numpy eigendecompositions; the reference's layer cache applied), as the kernels hold them"""
    U = block["mix"] if nubar > 0 else block["mix"].conj()
    Ud = U.conj().T
    dm = block["dm"]
    H_vac = U @ np.diag([0.0, dm[1][0], dm[2][0]]).astype(complex) @ Ud
    pot = block["mat_pot"] if nubar > 0 else -block["mat_pot"].conj()
    src = []
    for i in range(len(density)):
        s = -1
        if distance[i] > 0.0:
            s = i
            for j in range(i):
                if distance[j] > 0.0 and abs(density[j] - density[i]) < 1e-5 and abs(distance[j] - distance[i]) < 1e-5:
                    s = j
        src.append(s)
    A, T = {}, None
    for i, s in enumerate(src):
        if s < 0:
            continue
        if s != i:
            A[i] = A[s]
        else:
            H = H_vac / (2 * energy) + 0.5 * density[i] * TWORTTWOGF * pot
            Hm = Ud @ H @ U
            lam, V = np.linalg.eigh(0.5 * (Hm + Hm.conj().T))
            A[i] = (V * np.exp(-1j * lam * (2 * energy * (distance[i] / energy) * HBAR_C_FACTOR))) @ V.conj().T
        T = A[i] if T is None else A[i] @ T
    return U, T


def closed_form(U, T, dm, dl_over_e):
    """the nine averaged probabilities P[a][b] from the chain product of the midpoint row:
    sum_j |D_j|^2 + 2 sum_{j<k} sinc(x_jk) Re(D_j conj D_k),  D_j = (U T)[b][j] conj(U[a][j]),
    x_jk = (dm_j0 - dm_k0) 2.534 (dL / E) / 2"""
    W = U @ T
    m = np.array([0.0, dm[1][0], dm[2][0]])
    P = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            D = W[b, :] * U[a, :].conj()
            acc = np.sum(np.abs(D) ** 2)
            for j in range(3):
                for k in range(j + 1, 3):
                    x = (m[j] - m[k]) * HBAR_C_FACTOR * dl_over_e * 0.5
                    acc += 2.0 * np.sinc(x / np.pi) * (D[j] * D[k].conj()).real
            P[a, b] = acc
    return P


def load():
    """the committed golden file as a dict of arrays; `cases` = [(block, range index)] in the order of P_avg"""
    g = np.load(GOLDEN_FILE, allow_pickle=False)
    d = {k: g[k] for k in g.files}
    names = [str(s) for s in d["block_names"]]
    bl = [dict(name=n, dm=d["dm"][i], mix=d["mix"][i], mat_pot=d["mat_pot"][i], decay_flag=-1, mat_decay=X.ZERO_C.copy(),
               lri_pot=X.ZERO_R.copy()) for i, n in enumerate(names)]
    d["blocks"] = bl
    d["cases"] = [(bl[int(b)], int(r)) for b, r in zip(d["case_block"], d["case_range"])]
    return d
