"""Writes tests/golden/prob3_exact_ref.npz: the exact probabilities (oracle/exact_prob3.py, mpmath at 40
digits, rounded once to fp64) of every case of tests/prob3_exact_cases.py at every node and both signs,
together with everything the GPU test needs to call the kernels (parameter blocks, energies, coszen,
layer rows, Earth tables) and, per case, `oracle_over_gate`: the worst
|P_oracle - P_exact| / (1e-10 |P_exact| + 1e-14) of the fp64 oracle (`oracle.propagate_array`) on the
same rows.  That figure is what makes the gate legitimate for the device: the reference's arithmetic in
fp64 stays inside it on these very inputs.  The script refuses to write a file in which it exceeds 1.

    python oracle/gen_prob3_exact.py [--jobs N] [--check]

Arrays only; needs mpmath and this repository, nothing else.  About 2 600 nodes at ~0.1 s each, spread
over N processes (the result does not depend on N).  `--check` compares with the committed file instead
of writing.
"""
import argparse
import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc                   # noqa: E402
from tests import prob3_exact_cases as T           # noqa: E402

RTOL, ATOL = 1e-10, 1e-14                          # numba_osc_tests.py:82 (tests/conftest.py: PROB3_RTOL / PROB3_ATOL)


def _node(job):
    from oracle import exact_prob3

    params, nubar, energy, density, distance = job
    return exact_prob3.probabilities(*params, nubar, energy, density, distance)


def build(jobs):
    layers_golden = np.load(os.path.join(ROOT, "tests", "golden", "layers_ref.npz"), allow_pickle=False)
    earths = T.earth_tables(orc, layers_golden)
    cases = T.cases()
    work = []
    for c in cases:
        e, rho, dist = T.node_rows(earths[c["earth"]])
        for nubar in T.SIGNS:
            work += [(T.params_of(c), nubar, e[n], rho[n], dist[n]) for n in range(T.N_NODES)]
    with multiprocessing.Pool(jobs) as pool:
        res = pool.map(_node, work, chunksize=8)
    exact = np.array(res, np.float64).reshape(len(cases), len(T.SIGNS), T.N_NODES, 3, 3)
    over = np.zeros(len(cases))
    for i, c in enumerate(cases):
        e, rho, dist = T.node_rows(earths[c["earth"]])
        for s, nubar in enumerate(T.SIGNS):
            P = orc.propagate_array(*T.params_of(c), nubar, e, rho, dist)
            r = T.gate_ratio(P, exact[i, s], RTOL, ATOL)
            over[i] = max(over[i], r.max())
            if r.max() > 1.0:
                n, a, b = np.unravel_index(np.argmax(r), r.shape)
                raise SystemExit("the fp64 oracle misses the gate: case %s nubar %+d E %g coszen %g P[%d][%d] "
                                 "oracle %.17g exact %.17g (%.3g of the gate); change that case's inputs"
                                 % (c["name"], nubar, e[n], T.COSZEN[n % T.N_CZ], a, b, P[n, a, b], exact[i, s, n, a, b],
                                    r.max()))
        print("%-28s oracle_over_gate %.3f" % (c["name"], over[i]), flush=True)
    out = dict(
        case_names=np.array([c["name"] for c in cases]), earth_names=np.array(T.EARTHS),
        case_earth=np.array([T.EARTHS.index(c["earth"]) for c in cases], np.int64),
        dm=np.array([c["dm"] for c in cases]), mix=np.array([c["mix"] for c in cases]),
        mat_pot=np.array([c["mat_pot"] for c in cases]), decay_flag=np.array([c["decay_flag"] for c in cases], np.int64),
        mat_decay=np.array([c["mat_decay"] for c in cases]), lri_pot=np.array([c["lri_pot"] for c in cases]),
        energy=T.ENERGY, coszen=T.COSZEN,
        earth_radii=np.array([earths[e]["radii"] for e in T.EARTHS]), earth_rhos=np.array([earths[e]["rhos"] for e in T.EARTHS]),
        earth_coszen_limit=np.array([earths[e]["coszen_limit"] for e in T.EARTHS]),
        earth_r_detector=np.array([earths[e]["r_detector"] for e in T.EARTHS]),
        density=np.array([earths[e]["density"] for e in T.EARTHS]), distance=np.array([earths[e]["distance"] for e in T.EARTHS]),
        P_exact=exact, oracle_over_gate=over)
    return out


def save(path, arrays):
    """an .npz (np.load reads it) whose bytes depend on the arrays alone: np.savez stamps every member with
    the time of writing"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = build(a.jobs)
    if a.check:
        g = np.load(T.GOLDEN_FILE, allow_pickle=False)
        assert sorted(g.files) == sorted(out), (sorted(g.files), sorted(out))
        for k in out:
            assert g[k].dtype == out[k].dtype and g[k].shape == out[k].shape and g[k].tobytes() == out[k].tobytes(), k
        print("tests/golden/prob3_exact_ref.npz: every array reproduced bit for bit")
        return
    save(T.GOLDEN_FILE, out)
    print("wrote %s (%d bytes)" % (T.GOLDEN_FILE, os.path.getsize(T.GOLDEN_FILE)))


if __name__ == "__main__":
    main()
