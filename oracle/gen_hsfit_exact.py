"""Writes tests/golden/hsfit_exact_ref.npz: the exact answers of the hypersurface fits of tests/hsfit_cases.py that
are linear weighted least-squares problems (identity link, `linear` and `quadratic` forms only), known
independently of any minimiser.  With the design rows E_n = (1, x, x^2, ...), weights 1 / sigma_n^2 and prior
weights w_i = inv_prior_sigma_i^2,

    N = sum_n E_n E_n^T / sigma_n^2 + diag(w),   c* = N^-1 sum_n E_n y_n / sigma_n^2,   cov* = N^-1,
    L* = sum_n ((E_n . c* - y_n) / sigma_n)^2 + sum_i w_i c*_i^2

are solved in 40-digit arithmetic (mpmath) from the fp64 inputs converted exactly and rounded once to fp64.
Members: "<family>/<variant>/coef" [n_prob, C], ".../cov" [n_prob, C, C], ".../loss" [n_prob] for f_lin plain and
prior and f_ill twin_prior; "f_ill/twin/loss" alone for the twin design, whose Hessian is singular but whose minimum
loss is unique: it is the minimum of the problem with ONE slope on the shared x row.

    python oracle/gen_hsfit_exact.py [--check]

Arrays only; needs mpmath and this repository, nothing else.  The file's bytes depend on the arrays alone.  `--check`
compares with the committed file instead of writing.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.gen_prob3_exact import save            # noqa: E402  (an .npz without time stamps)
from tests import hsfit_cases as T                 # noqa: E402

DIGITS = 40


def design_columns(forms, x):
    """the columns of the design of an identity-link fit of linear / quadratic forms: (parameter, power) per
    coefficient, (None, 0) for the intercept"""
    cols = [(None, 0)]
    for p, f in enumerate(forms):
        assert f in ("linear", "quadratic"), f
        cols += [(p, 1)] + ([(p, 2)] if f == "quadratic" else [])
    return cols


def solve_exact(forms, x, y, sigma, ips):
    """(coef [C], cov [C, C], loss) of one problem, fp64 roundings of the 40-digit solution"""
    import mpmath as mp

    mp.mp.dps = DIGITS
    cols = design_columns(forms, x)
    n_coef = len(cols)
    used = [n for n in range(len(y)) if sigma[n] != 0.0]
    E = [[mp.mpf(1) if p is None else mp.mpf(float(x[p, n])) ** k for p, k in cols] for n in used]
    w = [1 / mp.mpf(float(sigma[n])) ** 2 for n in used]
    yy = [mp.mpf(float(y[n])) for n in used]
    N = mp.matrix(n_coef, n_coef)
    b = mp.matrix(n_coef, 1)
    for i in range(n_coef):
        for j in range(n_coef):
            N[i, j] = mp.fsum(w[n] * E[n][i] * E[n][j] for n in range(len(used)))
        N[i, i] += mp.mpf(float(ips[i])) ** 2
        b[i] = mp.fsum(w[n] * E[n][i] * yy[n] for n in range(len(used)))
    cov = mp.inverse(N)
    c = cov * b
    loss = mp.fsum(w[n] * (mp.fsum(E[n][i] * c[i] for i in range(n_coef)) - yy[n]) ** 2 for n in range(len(used)))
    loss += mp.fsum((mp.mpf(float(ips[i])) * c[i]) ** 2 for i in range(n_coef))
    return (np.array([float(c[i]) for i in range(n_coef)]),
            np.array([[float(cov[i, j]) for j in range(n_coef)] for i in range(n_coef)]), float(loss))


def solve_family(fam, forms=None, x=None, ips=None):
    forms = fam["forms"] if forms is None else forms
    x = fam["x"] if x is None else x
    ips = fam["ips"] if ips is None else ips
    res = [solve_exact(forms, x, fam["y"][:, k], fam["sigma"][:, k], ips) for k in range(fam["y"].shape[1])]
    return dict(coef=np.array([r[0] for r in res]), cov=np.array([r[1] for r in res]), loss=np.array([r[2] for r in res]))


def build():
    out = {}
    for name, fam in (("f_lin/plain", T.f_lin("plain")), ("f_lin/prior", T.f_lin("prior")),
                      ("f_ill/twin_prior", T.f_ill("twin_prior"))):
        for k, a in solve_family(fam).items():
            out["%s/%s" % (name, k)] = a
    twin = T.f_ill("twin")
    out["f_ill/twin/loss"] = solve_family(twin, ("linear",), twin["x"][:1], np.zeros(2))["loss"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    out = build()
    if a.check:
        g = np.load(T.EXACT_FILE, allow_pickle=False)
        assert sorted(g.files) == sorted(out), (sorted(g.files), sorted(out))
        for k in out:
            assert g[k].dtype == out[k].dtype and g[k].shape == out[k].shape and g[k].tobytes() == out[k].tobytes(), k
        print("tests/golden/hsfit_exact_ref.npz: every array reproduced bit for bit")
        return
    save(T.EXACT_FILE, out)
    print("wrote %s (%d bytes)" % (T.EXACT_FILE, os.path.getsize(T.EXACT_FILE)))


if __name__ == "__main__":
    main()
