"""Writes tests/golden/prob3_avg_exact.npz: the production-height average of the exact layered probabilities
(oracle/exact_prob3.py, imported unchanged) on the cases of tests/prob3_avg_cases.py.  Runs on the CPU; needs mpmath
and a C compiler (the CPU oracle's `Layers`).

Per node the golden value is the QUADRATURE

    P_avg[a][b] = (1 / dL) int_{Lbar - dL/2}^{Lbar + dL/2} P[a][b](d_f = l) dl

with `mp.quad` over a few sub-intervals at the module's working precision (DPS + GUARD digits); Lbar and dL are the
fp64 numbers the kernels are given, (L_min + L_max) / 2 and L_max - L_min rounded, so the limits are L_min and L_max
to 1e-14 km.  The integrand is the exact layered probability: the first traversed layer's matrix is the module's
matrix exponential at length l, the product of the layers behind it is formed once per node (they keep the matrices
they have in the midpoint row, the reference's layer cache applied to that row), and at l = Lbar the amplitude is
checked against the module's own `amplitude_mp` of the whole midpoint row.

The closed form is evaluated in mpmath as well and must agree with the quadrature to 1e-30 before anything is
written.  The fp64 inputs are converted exactly, so the mixing matrix is unitary only to 1e-16 and the first layer's
Hamiltonian U^dagger (U diag(dm) U^dagger) U is diagonal only to that order; the closed form is therefore taken on
its eigen-decomposition (mp.eigh): with the eigenvalues l_j and eigenvectors V of that matrix,

    D_j = (U T_rest V)[b][j] exp(-i l_j 2.534 Lbar / E) (V^dagger U^dagger)[j][a],   x_jk = (l_j - l_k) 2.534 (dL / E) / 2,
    P_avg = sum_j |D_j|^2 + 2 sum_{j<k} sinc(x_jk) Re(D_j conj D_k),

which for an exactly unitary U is the formula of DESIGN.md (V = 1, l_j = dm_j0) that the kernels evaluate.

    python scripts/dev/gen_prob3_avg_golden.py [--jobs N]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402

from oracle import exact_prob3 as E  # noqa: E402
from tests import prob3_avg_cases as T  # noqa: E402

AGREE = mp.mpf(10) ** -30
SPAN_PER_PART = 6.0     # radians of the fastest phase per sub-interval of the quadrature


def rows_for(orc, layers_golden):
    """per range: the nominal rows, the midpoint rows, Lbar, dL, L_min, L_max (fp64, from the CPU oracle's Layers)"""
    g = layers_golden
    depth, height, yi, yo, ym = g["prem12::args"]
    assert (depth, height) == (T.DETECTOR_DEPTH, T.PROP_HEIGHT)
    prem = np.array(g["prem12::prem"], dtype=np.float64, copy=True)

    def rows(h):
        lay = orc.Layers(prem, depth, h)
        lay.setElecFrac(yi, yo, ym)
        lay.calcLayers(T.COSZEN)
        return np.array(lay.density).reshape(T.N_CZ, -1), np.array(lay.distance).reshape(T.N_CZ, -1)

    rho, d_nom = rows(height)
    out = []
    for rng in T.RANGES:
        rho_lo, d_lo = rows(height - rng / 2)
        rho_hi, d_hi = rows(height + rng / 2)
        dist, lbar, dl, first = T.midpoint_rows(rho, d_nom, d_lo, d_hi)
        rr = np.arange(T.N_CZ)
        assert np.all(rho[rr, first] == 0.0) and np.all(dl > 0)
        # every other layer does not depend on the production height
        for r2, d2 in ((rho_lo, d_lo), (rho_hi, d_hi)):
            m = np.ones_like(d_nom, bool)
            m[rr, first] = False
            assert np.array_equal(r2, rho) and np.array_equal(d2[m], d_nom[m])
        out.append(dict(density=rho, distance=dist, lbar=lbar, dl=dl, first=first, lmin=d_lo[rr, first], lmax=d_hi[rr, first]))
    return out


def node(args):
    """(P_quad[3][3] rounded once to fp64, |quadrature - closed form| max, error estimate of the quadrature)"""
    block, nubar, energy, density, distance, first, dl64 = args
    with mp.workdps(E.DPS + E.GUARD):
        mix, mat_pot = E._mat(block["mix"]), E._mat(block["mat_pot"])
        dm10, dm20 = mp.mpf(float(block["dm"][1][0])), mp.mpf(float(block["dm"][2][0]))
        En = mp.mpf(float(energy))
        rho = [mp.mpf(float(x)) for x in density]
        dist = [mp.mpf(float(x)) for x in distance]
        # the limits are those of the fp64 numbers the kernels are given: Lbar -+ dL / 2 (L_min and L_max to 1e-14 km)
        dl = mp.mpf(float(dl64))
        lo, hi = dist[first] - dl / 2, dist[first] + dl / 2
        src = E.cache_sources(density, distance)
        assert src[first] == first and all(s != first for i, s in enumerate(src) if i != first)
        assert all(s < 0 for s in src[:first])
        U = mix if nubar > 0 else mix.apply(mp.conj)
        Ud = E._dagger(U)
        diag = mp.matrix(3, 3)
        diag[1, 1], diag[2, 2] = dm10, dm20
        H_vac = U * diag * Ud

        def layer(i, length):
            a = mp.mpf("0.5") * rho[i] * mp.mpf(E.TWORTTWOGF)
            H = H_vac / (2 * En) + (a * mat_pot if nubar > 0 else -a * mat_pot.apply(mp.conj))
            return E.expm((Ud * H * U) * mp.mpc(0, -1) * (2 * En * (length / En) * mp.mpf(E.HBAR_C_FACTOR)))

        A, T_rest = {}, mp.eye(3)
        for i, s in enumerate(src):
            if s < 0 or i == first:
                continue
            A[i] = A[s] if s != i else layer(i, dist[i])
            T_rest = A[i] * T_rest
        left = U * T_rest
        memo = {}

        def probs(length):
            if length not in memo:
                memo[length] = E.probabilities_of(left * layer(first, length) * Ud)
            return memo[length]

        # the restated loop against the module's own amplitude at the midpoint
        zero = mp.matrix(3, 3)
        F_mod = E.amplitude_mp(mix, dm10, dm20, mat_pot, -1, zero, zero, nubar, En, rho, dist, src)
        F_mid = left * layer(first, dist[first]) * Ud
        assert max(abs(F_mod[i, j] - F_mid[i, j]) for i in range(3) for j in range(3)) < mp.mpf(10) ** -45

        span = abs(dm20) * mp.mpf(E.HBAR_C_FACTOR) * dl / En
        parts = max(2, int(mp.ceil(span / SPAN_PER_PART)))
        edges = [lo + dl * k / parts for k in range(parts + 1)]
        quad, q_err = [[None] * 3 for _ in range(3)], mp.mpf(0)
        for a in range(3):
            for b in range(3):
                tot = mp.mpf(0)
                for k in range(parts):
                    v, err = mp.quad(lambda l: probs(l)[a][b], [edges[k], edges[k + 1]], error=True)
                    tot += v
                    q_err = max(q_err, err / dl)
                quad[a][b] = tot / dl

        # closed form on the eigen-decomposition of the first layer's Hamiltonian
        Hm = Ud * H_vac * U
        lam, V = mp.eigh((Hm + E._dagger(Hm)) / 2)
        c = mp.mpf(E.HBAR_C_FACTOR) / En
        lbar = dist[first]
        WL, WR = left * V, E._dagger(V) * Ud
        worst = mp.mpf(0)
        for a in range(3):
            for b in range(3):
                D = [WL[b, j] * mp.expj(-lam[j] * c * lbar) * WR[j, a] for j in range(3)]
                p = sum(abs(d) ** 2 for d in D)
                for j in range(3):
                    for k in range(j + 1, 3):
                        p += 2 * mp.sinc((lam[j] - lam[k]) * c * dl / 2) * mp.re(D[j] * mp.conj(D[k]))
                worst = max(worst, abs(p - quad[a][b]))
        assert worst < AGREE, (block["name"], nubar, energy, float(worst), float(q_err))
        return (np.array([[E._to_f64(x) for x in row] for row in quad]), float(worst), float(q_err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=T.GOLDEN_FILE)
    ap.add_argument("--jobs", type=int, default=max(1, (os.cpu_count() or 2) - 1))
    args = ap.parse_args()
    from oracle import oracle as orc

    orc.build()
    tabs = rows_for(orc, np.load(os.path.join(ROOT, "tests", "golden", "layers_ref.npz"), allow_pickle=False))
    cases = T.cases()
    work = []
    for block, r in cases:
        t = tabs[r]
        for nubar in T.SIGNS:
            for ie in range(T.N_E):
                for j in range(T.N_CZ):
                    work.append((block, nubar, T.ENERGY[ie], t["density"][j], t["distance"][j], int(t["first"][j]),
                                 t["dl"][j]))
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(node, work, chunksize=1)
    P = np.array([r[0] for r in res]).reshape(len(cases), 2, T.N_NODES, 3, 3)
    agree = np.array([r[1] for r in res]).reshape(len(cases), 2, T.N_NODES)
    q_err = np.array([r[2] for r in res]).reshape(len(cases), 2, T.N_NODES)
    bl = T.blocks()
    names = [b["name"] for b in bl]
    np.savez_compressed(
        args.out, energy=T.ENERGY, coszen=T.COSZEN, ranges=np.array(T.RANGES), P_avg=P, closed_form_agreement=agree,
        quad_error=q_err, block_names=np.array(names), dm=np.array([b["dm"] for b in bl]),
        mix=np.array([b["mix"] for b in bl]), mat_pot=np.array([b["mat_pot"] for b in bl]),
        case_block=np.array([names.index(b["name"]) for b, _ in cases]), case_range=np.array([r for _, r in cases]),
        density=np.array([t["density"] for t in tabs]), distance=np.array([t["distance"] for t in tabs]),
        lbar=np.array([t["lbar"] for t in tabs]), dl=np.array([t["dl"] for t in tabs]),
        lmin=np.array([t["lmin"] for t in tabs]), lmax=np.array([t["lmax"] for t in tabs]),
        first=np.array([t["first"] for t in tabs]))
    print("nodes %d  worst |quadrature - closed form| %.2e  worst quadrature error estimate %.2e" % (
        len(res), agree.max(), q_err.max()))


if __name__ == "__main__":
    main()
