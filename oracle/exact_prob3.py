"""The layered three-flavour propagator in exact arithmetic (`mpmath`, 40 digits): what the prob3 kernels
and the fp64 oracle are measured against (tests/golden/prob3_exact_ref.npz, oracle/gen_prob3_exact.py).

TEST INFRASTRUCTURE ONLY.  No closed forms: no cubic, no Lagrange sum, no reduced Hermitian form.  Per
node, with the quantities of numba_osc_kernels.py:121-345, 348-478, 535-653:

    U      = mix for nubar > 0, conj(mix) otherwise
    H_vac  = U diag(0, dm[1][0], dm[2][0]) U^dagger        (+ U mat_decay U^dagger if decay_flag == 1)
    matter = a mat_pot (nu) or -a conj(mat_pot) (nubar), a = 0.5 rho 1.52588e-4;  lri = +-lri_pot 1e9
    H      = H_vac / (2E) + matter + lri,   H_m = U^dagger H U
    A      = expm(-i H_m 2E (L/E) 2.534)                    one layer, by scaling, Taylor series and squaring
    T      = A_last ... A_first over the layers with distance > 0,  F = U T U^dagger,  P[i][j] = |F[j][i]|^2

The reference's Lagrange sum over the eigenvalues of H_m is this matrix exponential.  Its layer cache is a
DEFINITION, not rounding, and is applied: a layer takes the matrix of the LAST earlier layer j (itself of
positive length) with |rho_j - rho| < 1e-5 and |dist_j - dist| < 1e-5.

The fp64 inputs and the three constants of the reference (1.52588e-4, 1e9, 2.534: the fp64 numbers those
literals denote) are converted exactly; every operation runs at `dps` + GUARD digits; the probabilities are
rounded once to fp64.
"""
import numpy as np

try:
    import mpmath as mp
except ImportError as exc:       # the generator and the host test need it; nothing else imports this module
    raise ImportError("oracle/exact_prob3.py needs mpmath") from exc

DPS = 40
GUARD = 15      # the squarings of expm lose log10(2^s) <= 4 digits at the largest phases (a few thousand radians)

TWORTTWOGF = 1.52588e-4
LRI_SCALE = 1e9
HBAR_C_FACTOR = 2.534


def _mat(a):
    a = np.asarray(a)
    return mp.matrix([[mp.mpc(mp.mpf(float(z.real)), mp.mpf(float(z.imag))) for z in row] for row in a.astype(complex)])


def _dagger(m):
    return m.transpose_conj()


def _norm1(m):
    return max(sum(abs(m[i, j]) for i in range(m.rows)) for j in range(m.cols))


def expm(m):
    """exp of a small square matrix at the current working precision: m / 2^s with norm <= 1/2, the Taylor
    series until a term no longer counts, s squarings"""
    n = m.rows
    nrm = _norm1(m)
    s = 0
    if nrm > 0.5:
        s = int(mp.ceil(mp.log(nrm, 2))) + 1
    x = m / mp.mpf(2) ** s
    acc = mp.eye(n)
    term = mp.eye(n)
    tiny = mp.mpf(10) ** (-(mp.mp.dps + 5))
    k = 1
    while True:
        term = term * x / k
        acc = acc + term
        k += 1
        if _norm1(term) < tiny:
            break
    for _ in range(s):
        acc = acc * acc
    return acc


def cache_sources(density, distance):
    """the reference's cache rule (numba_osc_kernels.py:230-249): src[i] = i for a layer that gets its own
    matrix, the LAST earlier j with both differences below 1e-5 for one that copies, -1 for a layer that
    is not traversed.  The comparison is the reference's, on the fp64 rows."""
    density = np.asarray(density, np.float64)
    distance = np.asarray(distance, np.float64)
    src = []
    for i in range(len(density)):
        if not distance[i] > 0.0:
            src.append(-1)
            continue
        idx = i
        for j in range(i):
            if distance[j] > 0.0 and abs(density[j] - density[i]) < 1e-5 and abs(distance[j] - distance[i]) < 1e-5:
                idx = j
        src.append(idx)
    return src


def amplitude_mp(mix, dm10, dm20, mat_pot, decay_flag, mat_decay, lri_pot, nubar, energy, density, distance, src):
    """F = U T U^dagger from mpmath inputs (matrices `mix`, `mat_pot`, `mat_decay`, `lri_pot` in eV; numbers
    `dm10`, `dm20`, `energy`; sequences `density`, `distance`) at the CURRENT working precision; `src` is the
    cache table of `cache_sources`.  The tests of the propagator itself call this with a mixing matrix that
    is unitary to the working precision, which a matrix of fp64 entries is not."""
    E = energy
    U = mix if nubar > 0 else mix.apply(mp.conj)
    Ud = _dagger(U)
    diag = mp.matrix(3, 3)
    diag[1, 1] = dm10
    diag[2, 2] = dm20
    H_vac = U * diag * Ud
    if int(decay_flag) == 1:
        H_vac = H_vac + U * mat_decay * Ud
    lri = lri_pot * mp.mpf(LRI_SCALE)
    A = {}
    T = None
    for i, s in enumerate(src):
        if s < 0:
            continue
        if s != i:
            A[i] = A[s]
        else:
            a = mp.mpf("0.5") * density[i] * mp.mpf(TWORTTWOGF)
            if nubar > 0:
                H = H_vac / (2 * E) + a * mat_pot + lri
            else:
                H = H_vac / (2 * E) - a * mat_pot.apply(mp.conj) - lri
            H_m = Ud * H * U
            A[i] = expm(H_m * mp.mpc(0, -1) * (2 * E * (distance[i] / E) * mp.mpf(HBAR_C_FACTOR)))
        T = A[i] if T is None else A[i] * T
    if T is None:                           # no layer of positive length: the reference reads an empty array
        T = mp.matrix(3, 3)
    return U * T * Ud


def flavour_amplitude(dm, mix, mat_pot, decay_flag, mat_decay, lri_pot, nubar, energy, density, distance, dps=DPS):
    """F = U T U^dagger of fp64 inputs (converted exactly), an mpmath matrix at dps + GUARD digits"""
    with mp.workdps(dps + GUARD):
        dm = np.asarray(dm, np.float64)
        return amplitude_mp(_mat(mix), mp.mpf(float(dm[1][0])), mp.mpf(float(dm[2][0])), _mat(mat_pot), decay_flag,
                            _mat(mat_decay), _mat(lri_pot), nubar, mp.mpf(float(energy)),
                            [mp.mpf(float(x)) for x in density], [mp.mpf(float(x)) for x in distance],
                            cache_sources(density, distance))


def probabilities_of(F):
    """P[i][j] = |F[j][i]|^2 (mpmath numbers, not rounded)"""
    return [[mp.re(F[j, i]) ** 2 + mp.im(F[j, i]) ** 2 for j in range(3)] for i in range(3)]


def probabilities_mp(*args, **kw):
    """P[i][j] = |F[j][i]|^2 as mpmath numbers (not rounded)"""
    F = flavour_amplitude(*args, **kw)
    with mp.workdps(kw.get("dps", DPS) + GUARD):
        return probabilities_of(F)


def probabilities(dm, mix, mat_pot, decay_flag, mat_decay, lri_pot, nubar, energy, density, distance, dps=DPS):
    """the exact probabilities of one node, rounded once to fp64: float64[3][3]"""
    P = probabilities_mp(dm, mix, mat_pot, decay_flag, mat_decay, lri_pot, nubar, energy, density, distance, dps=dps)
    return np.array([[_to_f64(x) for x in row] for row in P], np.float64)


def _to_f64(x):
    """round to nearest even at 53 bits, then convert (exactly)"""
    with mp.workprec(53):
        return float(+x)
