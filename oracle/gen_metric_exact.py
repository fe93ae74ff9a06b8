"""Writes tests/golden/metric_exact_ref.npz: for every family of tests/metric_cases.py and every kind it is evaluated
with, the exact per-bin value (oracle/exact_metric.py, mpmath at 80 digits) as a pair of doubles `hi`, `lo`, the
magnitude `m` of the gate and the `flag` of the NaN / -inf outcomes, next to the inputs (`k`, `lam`, `sigma`, `s2`).
Members are named "<family>/<column>" and "<family>/<kind>/<column>".

    python oracle/gen_metric_exact.py [--jobs N] [--check]

Arrays only; needs mpmath and this repository, nothing else.  The result does not depend on N, and the file's bytes
depend on the arrays alone.  `--check` compares with the committed file instead of writing.
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.gen_prob3_exact import save            # noqa: E402  (an .npz without time stamps)
from tests import metric_cases as T                # noqa: E402

CHUNK = 16


def _chunk(job):
    from oracle import exact_metric

    kind, k, lam, s2 = job
    return exact_metric.evaluate(kind, k, lam, s2)


def entry(kind, k, lam, s2, pool=None):
    """dict(hi, lo, m, flag) of one kind on arrays of inputs"""
    jobs = [(kind, k[i:i + CHUNK], lam[i:i + CHUNK], s2[i:i + CHUNK]) for i in range(0, len(k), CHUNK)]
    res = pool.map(_chunk, jobs) if pool is not None else [_chunk(j) for j in jobs]
    hi, lo, m, flag = ([x for r in res for x in r[c]] for c in range(4))
    return dict(hi=np.array(hi, np.float64), lo=np.array(lo, np.float64), m=np.array(m, np.float64),
                flag=np.array(flag, np.int8))


def build(jobs):
    out = {}
    fams = T.families()
    with multiprocessing.Pool(jobs) as pool:
        for f in T.FAMILY_ORDER:
            for c in ("k", "lam", "sigma", "s2"):
                out["%s/%s" % (f, c)] = np.array(fams[f][c])
            for kind in T.kinds_of(f):
                e = entry(kind, fams[f]["k"], fams[f]["lam"], fams[f]["s2"], pool)
                for c, a in e.items():
                    out["%s/%s/%s" % (f, kind, c)] = a
                print("%-14s %-22s %4d bins, %d flagged" % (f, kind, e["hi"].size, int((e["flag"] != 0).sum())), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = build(a.jobs)
    if a.check:
        g = np.load(T.EXACT_FILE, allow_pickle=False)
        assert sorted(g.files) == sorted(out), (sorted(g.files), sorted(out))
        for k in out:
            assert g[k].dtype == out[k].dtype and g[k].shape == out[k].shape and g[k].tobytes() == out[k].tobytes(), k
        print("tests/golden/metric_exact_ref.npz: every array reproduced bit for bit")
        return
    save(T.EXACT_FILE, out)
    print("wrote %s (%d bytes)" % (T.EXACT_FILE, os.path.getsize(T.EXACT_FILE)))


if __name__ == "__main__":
    main()
