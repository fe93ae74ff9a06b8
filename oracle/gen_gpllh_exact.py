"""Writes tests/golden/gpllh_exact.npz: for every call of every family of tests/gpllh_cases.py the exact per-bin log
value of the generalized Poisson-gamma likelihood (arXiv:1902.08831 eq. 91, mpmath at 60 digits; the Poisson branch's
formula on the exact weight sum) as a pair of doubles `hi`, `lo`, the gate's magnitude `m`, the `flag` of the rule
outcomes, the error code `err` and the `branch`, next to the inputs; the exact alpha and beta of the `params` family
and the exact sums of the `bin_sums` family by rational arithmetic.  Members are named "<family>/<call>/<column>".

    python oracle/gen_gpllh_exact.py [--jobs N] [--check]

Arrays only; needs mpmath and this repository, nothing else.  The result does not depend on N, and the file's bytes
depend on the arrays alone.  `--check` compares with the committed file instead of writing.

The flags of the bins marked `edge` (all of `domain_edge`, one bin each of two calls of `total`) are the outcome
classes of the double algorithm (the restatement of tests/gpllh_cases.py), which is what the kernel and the reference's
C code compute there; everywhere else the flags follow from the exact value, and the generator refuses a bin within a
factor 1e5 of the clamp at 1e-300.
"""
import argparse
import math
import multiprocessing
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.gen_prob3_exact import save            # noqa: E402  (an .npz without time stamps)
from tests import gpllh_cases as T                 # noqa: E402

DPS = 60


def pair(x):
    """an mpmath number as hi + lo, two doubles"""
    hi = float(x)
    return hi, float(x - hi)


def eq91(k, alphas, betas):
    """eq. 91 at DPS digits -> (prefac * delta_k, log of it or None if it is 0)"""
    import mpmath as mp

    with mp.workdps(DPS):
        a = [mp.mpf(float(x)) for x in alphas]
        b = [mp.mpf(float(x)) for x in betas]
        prefac = mp.mpf(1)
        for ai, bi in zip(a, b):
            prefac *= (bi / (1 + bi)) ** ai
        r = [1 / (1 + bi) for bi in b]
        rp = [mp.mpf(1)] * len(r)
        s = [mp.mpf(0)]
        for i in range(1, k + 1):
            rp = [x * y for x, y in zip(rp, r)]
            s.append(mp.fdot(a, rp))
        d = [mp.mpf(1)]
        for i in range(1, k + 1):
            d.append(mp.fdot(s[1:i + 1], d[i - 1::-1]) / i)
        p = prefac * d[k]
        return p, (mp.log(p) if p > 0 else None)


def mixture_job(job):
    """(k, alphas, betas), finite containers only -> (hi, lo, log10 of the value or -inf)"""
    import mpmath as mp

    k, a, b = job
    with mp.workdps(DPS):
        p, lp = eq91(k, a, b)
        if lp is None:
            return 0.0, 0.0, -math.inf
        hi, lo = pair(lp)
        return hi, lo, float(lp / mp.log(10))


def poisson_exact(k, w):
    import mpmath as mp

    with mp.workdps(DPS):
        f = sum(Fraction(float(x)) for x in w)
        W = mp.mpf(f.numerator) / f.denominator
        if k == 0:
            hi, lo = pair(-W)
            return hi, lo, float(W) + 1.0
        x = mp.mpf(k)
        v = x * mp.log(W) - W - (x * mp.log(x) - x)
        hi, lo = pair(v)
        return hi, lo, float(x * abs(mp.log(W)) + W + x * mp.log(x) + x + 1)


def classify(call):
    """per bin (branch, flag or None, err, job key or None) by the kernel's rules, before any arithmetic"""
    cap = T.scratch_k_of(call)
    out = []
    for i, kd in enumerate(call["data"].tolist()):
        w, a, b, n = (call[c][:, i] for c in ("w", "alpha", "beta", "n_mc"))
        if not kd >= 0.0:
            out.append((T.BRANCH_NONE, T.F_ERR, T.ERR_NEGATIVE, None))
            continue
        k = int(kd)
        if call["empty"][i]:
            out.append((T.BRANCH_NONE, T.F_SMALL if k > 0 else T.F_ZERO, 0, None))
        elif np.any(~(w >= 0.0)):
            out.append((T.BRANCH_NONE, T.F_ERR, T.ERR_NEGATIVE, None))
        elif np.all(n > 100.0):
            out.append((T.BRANCH_POISSON, None, 0, None))
        else:
            ok = np.isfinite(a) & np.isfinite(b)
            if np.any(ok & (~(a > 0.0) | ~(b > 0.0))) or k > T.bin_cap(kd, cap):
                out.append((T.BRANCH_MIXTURE, T.F_ERR, T.ERR_INVALID, None))
            else:
                out.append((T.BRANCH_MIXTURE, None, 0, (k, tuple(a[ok].tolist()), tuple(b[ok].tolist()))))
    return out


def build(jobs, only=None):
    """only: {(family, call index): bins} to restrict the work to (the host test's sample)"""
    fams = T.families()
    classes, keys = {}, set()
    for f, calls in fams.items():
        for ci, c in enumerate(calls):
            if only is not None and (f, ci) not in only:
                continue
            cl = classify(c)
            classes[(f, ci)] = cl
            for i, x in enumerate(cl):
                if x[3] is not None and (only is None or i in only[(f, ci)]):
                    keys.add(x[3])
    keys = sorted(keys, key=lambda x: (-x[0], x))             # longest first
    if jobs > 1:
        with multiprocessing.Pool(jobs) as pool:
            values = dict(zip(keys, pool.map(mixture_job, keys, chunksize=1)))
    else:
        values = {x: mixture_job(x) for x in keys}
    out = {}
    for (f, ci), cl in classes.items():
        c = fams[f][ci]
        n = c["data"].size
        hi, lo, m = np.zeros(n), np.zeros(n), np.zeros(n)
        flag, err, branch = np.zeros(n, np.int8), np.zeros(n, np.int32), np.zeros(n, np.int8)
        rest_flag = T.call_values(c, np.flatnonzero(c["edge"]))[3]
        for i, (br, fl, er, key) in enumerate(cl):
            branch[i], err[i] = br, er
            if only is not None and i not in only[(f, ci)]:
                continue
            if fl is not None:
                flag[i], hi[i] = fl, T.RULE_VALUE[fl]
            elif br == T.BRANCH_POISSON:
                hi[i], lo[i], m[i] = poisson_exact(int(c["data"][i]), c["w"][:, i])
            else:
                h, l, log10 = values[key]
                m[i] = sum(key[1]) + key[0] + 1.0
                if c["edge"][i]:
                    # the double algorithm's class; hi, lo keep eq. 91's value where the class has none of its own
                    flag[i] = rest_flag[i] if rest_flag[i] != T.F_VALUE else T.F_RESTATED
                    hi[i], lo[i] = (h, l) if flag[i] == T.F_RESTATED else (T.RULE_VALUE[int(flag[i])], 0.0)
                elif log10 > -295.0:
                    hi[i], lo[i] = h, l
                else:
                    assert log10 < -305.0, (f, ci, i, log10, "on the knife edge of the clamp")
                    flag[i], hi[i] = T.F_TINY, T.LOG_TINY
        pre = "%s/%d/" % (f, ci)
        for col in T.INPUT_COLUMNS:
            out[pre + col] = np.array(c[col])
        for col, arr in (("hi", hi), ("lo", lo), ("m", m), ("flag", flag), ("err", err), ("branch", branch)):
            out[pre + col] = arr
        print("%-14s %-16s %3d bins, flags %s" % (f, c["name"], n, sorted(set(flag.tolist()))), flush=True)
    if only is None:
        out.update(params_exact())
        out.update(bin_sums_exact())
    return out


def params_exact():
    """exact alpha = (n + adj) sw^2 / (n sw2), beta = sw / sw2 (with the pseudo-weight where n = 0; var_z = 0:
    alpha = (n + adj) 0.001, beta = 1) of the doubles, by rational arithmetic, as hi + lo"""
    pf = T.params_family()[0]
    out = {"params/" + c: np.array(pf[c]) for c in ("sw", "sw2", "n", "adj")}
    shape = pf["sw"].shape
    cols = {c: np.zeros(shape) for c in ("alpha_hi", "alpha_lo", "beta_hi", "beta_lo")}
    pw = Fraction(T.PSEUDO_WEIGHT)
    for c in range(shape[0]):
        for i in range(shape[1]):
            sw, sw2, n = (Fraction(float(pf[x][c, i])) for x in ("sw", "sw2", "n"))
            adj = Fraction(float(pf["adj"][c]))
            if not n > 0:
                sw, sw2, n = pw, Fraction(T.PSEUDO_WEIGHT * T.PSEUDO_WEIGHT), Fraction(1)
            if sw2 == 0:
                alpha, beta = (n + adj) * pw, Fraction(1)
            else:
                alpha, beta = (n + adj) * sw * sw / (n * sw2), sw / sw2
            for name, v in (("alpha", alpha), ("beta", beta)):
                try:
                    hi = float(v)
                    lo = float(v - Fraction(hi))
                except OverflowError:
                    hi, lo = math.inf, 0.0
                cols[name + "_hi"][c, i], cols[name + "_lo"][c, i] = hi, lo
    out.update({"params/" + k: v for k, v in cols.items()})
    return out


def bin_sums_exact():
    out = {}
    for c in T.bin_sums_family():
        pre = "bin_sums/%s/" % c["name"]
        n_bins = c["offsets"].size - 1
        cols = {k: np.zeros(n_bins) for k in ("sw_hi", "sw_lo", "sw2_hi", "sw2_lo", "abs1", "abs2")}
        for b in range(n_bins):
            x = c["weights"][c["index"][c["offsets"][b]:c["offsets"][b + 1]]]
            if not np.all(np.isfinite(x)):
                cols["sw_hi"][b] = cols["sw2_hi"][b] = np.nan
                continue
            fr = [Fraction(v) for v in x.tolist()]
            for name, terms, ab in (("sw", fr, "abs1"), ("sw2", [v * v for v in fr], "abs2")):
                tot = sum(terms, Fraction(0))
                hi = float(tot)
                cols[name + "_hi"][b], cols[name + "_lo"][b] = hi, float(tot - Fraction(hi))
                cols[ab][b] = float(sum((abs(v) for v in terms), Fraction(0)))
        out[pre + "digest"] = np.frombuffer(T.bin_sums_digest(c), dtype=np.uint8).copy()
        out.update({pre + k: v for k, v in cols.items()})
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
        print("tests/golden/gpllh_exact.npz: every array reproduced bit for bit")
        return
    save(T.EXACT_FILE, out)
    print("wrote %s (%d bytes)" % (T.EXACT_FILE, os.path.getsize(T.EXACT_FILE)))


if __name__ == "__main__":
    main()
