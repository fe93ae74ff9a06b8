"""Shared pieces of the tests of the nuisance-posterior sampler (csrc/posterior_device.hpp, csrc/posterior.hip:
`pisa_hip_posterior_sample` through `kernels.posterior_sample`): the numpy fp64 restatement of the definition, vectorised
over problems and walkers, its marks, the seeded cases and the exactly known targets of the statistical tests.  A plain
helper module (no fixtures); `tests/test_host_posterior.py` pins everything here without a GPU,
`tests/test_gpu_posterior.py` runs the kernel.

The definition ("Trial ensembles: the nuisance posterior").  Problem p has a data row d, a template row
(e, s2, R [J, B], centre c [J], box lo / hi [J]) and W walkers in J dimensions, H = W / 2.

    lp(eta) = -Phi(eta) (llh, poisson_llh), -Phi(eta) / 2 (chi2, mod_chi2); Phi as `profile_cases._sweep` forms it (bins
        ascending, a non-finite datum or expectation skipped, `two_sum`), Phi = s + c, then w (ips_j (eta_j + c_j))^2 in
        ascending j.  -inf: a responding finite bin with !(mu >= 1e-10), an eta_j outside [lo_j, hi_j], a NaN Phi.
    walker w, step s: blocks A = philox(0xC0000000 + w, s, stream, chain_id), B = philox(0xD0000000 + w, s, stream,
        chain_id) under the key of the seed; u_z = unit(A0, A1), u_p = unit(A2, A3), u_a = unit_open(B0, B1).
    z = ((u_z + 1) (u_z + 1)) / 2; partner q = min(int(u_p H), H - 1) of the other half, at c; y = c + z (x - c);
    accept iff lp(y) is neither NaN nor -inf and log(u_a) < (N - 1) log(z) + (lp(y) - lp(x)); N: unpinned coordinates.
    [0, H) move against [H, W), then [H, W) against the new [0, H).  Kept: s >= keep_from, (s - keep_from) % thin == 0.

Everything but `log` is an IEEE operation rounded on its own, the same on both sides, so positions agree bit for bit as
long as every accept decision agrees.  A decision is marked `marginal` where

    |log u_a - rhs| <= MARGIN_EPS eps (|log u_a| + |N - 1| |log z| + S_y + S_x),

S the sum over the kept bins of |m_b| + |d_b log m_b| (the llh kinds) or |phi_b| (the chi2 kinds) plus the prior terms:
the convention of tests/fluctuate_cases.py, with a factor 64 over what a log within `LOG_ULPS` ulps can move (each bin's
term by (LOG_ULPS + 2) eps of its magnitude, see `LOGP_ULPS`).  A proposal within MARGIN_EPS eps of a box edge, or
with a responding bin's mu that close to 1e-10, is marked `edge`.  `first_mark[p]` is the first step of the call at
which problem p has a mark: up to there the device must agree bit for bit.  The seeds of the GPU shapes mark nothing,
which tests/test_host_posterior.py asserts ("another seed rather than a wider window").

A stored lp agrees within LOGP_ULPS eps S for the llh kinds: (LOG_ULPS + 1) eps |d log m| from the log and the
product, eps (|m| + |d log m|) from the two roundings of the subtraction on both sides, eps |Phi| from the last
addition of the compensated chain.  The chi2 kinds call no library function: their lp agrees bit for bit.
"""
import numpy as np

from tests import ensemble_cases as ec
from tests import fluctuate_cases as fc
from tests import fluctuate_method_cases as fm
from tests import profile_cases as pc

EPS = pc.EPS
SMALL_POS = pc.SMALL_POS
KINDS = pc.KINDS
LLH_KINDS = pc.LLH_KINDS
MARGIN_EPS = fc.MARGIN_EPS
LOGP_ULPS = fm.LOG_ULPS + 3
WORD_A, WORD_B = 0xC0000000, 0xD0000000
START_OUTSIDE, BAD_BOUNDS = 8, 16
MAX_WALKERS = 256


def key_of(seed):
    return seed & 0xFFFFFFFF, seed >> 32


def n_keep_of(first_step, n_steps, keep_from=0, thin=1):
    return sum(1 for s in range(first_step, first_step + n_steps) if s >= keep_from and (s - keep_from) % thin == 0)


def problems(kind, D, E, R, S2=None, ips=None, c=None, lo=None, hi=None, t_of=None, k_of=None):
    """the rows of every problem gathered: D [T, B], E / S2 [K, B], R [K, J, B] or [J, B], ips [J], c [K, J], lo / hi
    [J] or [K, J] (None: no bound), t_of / k_of [P] -> dict(kind, d, e, s2 [P, B], R [P, J, B], ips [J], c, lo, hi
    [P, J])"""
    D, E, R = (np.asarray(a, dtype=np.float64) for a in (D, E, R))
    K = E.shape[0]
    R = R if R.ndim == 3 else np.broadcast_to(R[None], (K,) + R.shape)
    J = R.shape[1]
    S2 = np.zeros_like(E) if S2 is None else np.asarray(S2, dtype=np.float64)
    t_of = np.arange(D.shape[0]) if t_of is None else np.asarray(t_of)
    k_of = np.arange(K) if k_of is None else np.asarray(k_of)

    def per_k(a, fill):
        a = np.full((K, J), fill) if a is None else np.asarray(a, dtype=np.float64)
        return np.broadcast_to(a, (K, J))[k_of]

    return dict(kind=kind, d=D[t_of], e=E[k_of], s2=S2[k_of], R=R[k_of],
                ips=np.zeros(J) if ips is None else np.asarray(ips, dtype=np.float64), c=per_k(c, 0.0),
                lo=per_k(lo, -np.inf), hi=per_k(hi, np.inf))


def logp(pr, eta):
    """eta [P, M, J] -> (lp [P, M], S [P, M]: the magnitude of the marks, edge [P, M])"""
    kind, d, e, s2, R = pr["kind"], pr["d"], pr["e"], pr["s2"], pr["R"]
    J = R.shape[1]
    w = pc.w_of(kind)
    with np.errstate(all="ignore"):
        live = (np.isfinite(d) & np.isfinite(e))[:, None, :]
        responds = (R != 0).any(axis=1)[:, None, :]
        mu = np.broadcast_to(e[:, None, :], eta.shape[:2] + e.shape[1:]).copy()
        reach = np.abs(mu)
        for j in range(J):
            t = R[:, None, j, :] * eta[:, :, j, None]
            mu = mu + t
            reach = reach + np.abs(t)
        inside = ~(live & responds & ~(mu >= SMALL_POS)).any(axis=2)
        edge = (live & responds & (np.abs(mu - SMALL_POS) <= MARGIN_EPS * EPS * reach)).any(axis=2)
        m = np.where(mu < SMALL_POS, SMALL_POS, mu)
        dd = d[:, None, :]
        if kind in LLH_KINDS:
            dl = dd * np.log(m)
            phi = m - dl
            mag = np.abs(m) + np.abs(dl)
        else:
            v = s2[:, None, :] + m if kind == "mod_chi2" else m
            rr = dd - m
            phi = rr * (rr / v)
            mag = np.abs(phi)
        phi = np.where(live, phi, 0.0)
        s = np.zeros(eta.shape[:2])
        comp = np.zeros_like(s)
        for b in range(phi.shape[2]):
            s, comp = pc.two_sum(s, comp, phi[:, :, b])
        Phi = s + comp
        S = np.where(live, mag, 0.0).sum(axis=2)
        in_box = np.ones(eta.shape[:2], dtype=bool)
        for j in range(J):
            p = pr["ips"][j] * (eta[:, :, j] + pr["c"][:, None, j])
            pp = w * (p * p)
            Phi = Phi + pp
            S = S + pp
            lo, hi, x = pr["lo"][:, None, j], pr["hi"][:, None, j], eta[:, :, j]
            in_box &= (x >= lo) & (x <= hi)
            for bound in (lo, hi):
                edge |= np.isfinite(bound) & (x != bound) & (
                    np.abs(x - bound) <= MARGIN_EPS * EPS * np.maximum(np.abs(x), np.abs(bound)))
        lp = -Phi if kind in LLH_KINDS else -0.5 * Phi
        lp = np.where(inside & in_box & ~np.isnan(Phi), lp, -np.inf)
    return lp, S, edge


def uniforms(w, s, stream, chain_id, seed):
    """w [H], s a step number, chain_id [P] -> u_z, u_p, u_a [P, H]"""
    key = key_of(seed)
    shape = (len(chain_id), len(w))
    ctr = lambda word: [np.broadcast_to(np.uint64(word) + w.astype(np.uint64)[None, :], shape),   # noqa: E731
                        np.full(shape, s, dtype=np.uint64), np.full(shape, stream, dtype=np.uint64),
                        np.broadcast_to(np.asarray(chain_id, dtype=np.uint64)[:, None], shape)]
    a = fc.philox(ctr(WORD_A), key)
    b = fc.philox(ctr(WORD_B), key)
    return fc.unit(a[0], a[1]), fc.unit(a[2], a[3]), fm.unit_open(b[0], b[1])


def sample(pr, x0, n_steps, seed, stream=0, chain_id=None, first_step=0, keep_from=0, thin=1, marks=True):
    """The chains of every problem -> dict(chain [P, n_keep, W, J], logp [P, n_keep, W], S (of logp), accepted [P, W],
    end [P, W, J], end_logp [P, W], status [P], first_mark [P]: the first step index (of this call) with a marginal or
    edge mark, n_steps where there is none; n_marginal, n_edge, n_decisions)"""
    x = np.array(x0, dtype=np.float64)
    P, W, J = x.shape
    H = W // 2
    assert W % 2 == 0 and 2 <= W <= MAX_WALKERS and W >= 2 * J
    chain_id = np.arange(P) if chain_id is None else np.asarray(chain_id)
    lo, hi = pr["lo"], pr["hi"]
    with np.errstate(invalid="ignore"):
        bad = ~(lo <= hi).all(axis=1)
        n_free = ((lo < hi) | np.isinf(lo) | np.isinf(hi)).sum(axis=1).astype(np.float64)[:, None]
    lp, S, _ = logp(pr, x)
    status = np.where(bad, BAD_BOUNDS, np.where((np.isnan(lp) | (lp == -np.inf)).any(axis=1), START_OUTSIDE, 0))
    status = status.astype(np.int32)
    dead = status != 0
    n_keep = n_keep_of(first_step, n_steps, keep_from, thin)
    chain = np.empty((P, n_keep, W, J))
    kept_lp, kept_S = np.empty((P, n_keep, W)), np.empty((P, n_keep, W))
    accepted = np.zeros((P, W), dtype=np.int32)
    first_mark = np.full(P, n_steps)
    n_marginal = n_edge = 0
    rows = np.arange(P)[:, None]
    i_keep = 0
    for i in range(n_steps):
        s = first_step + i
        for half in (0, 1):
            mov = slice(half * H, half * H + H)
            u_z, u_p, u_a = uniforms(np.arange(half * H, half * H + H), s, stream, chain_id, seed)
            t = u_z + 1.0
            z = (t * t) / 2.0
            q = np.minimum((u_p * float(H)).astype(np.int64), H - 1) + (1 - half) * H
            c = x[rows, q]
            y = c + z[:, :, None] * (x[:, mov] - c)
            lp_y, S_y, edge = logp(pr, y)
            with np.errstate(all="ignore"):
                lhs, lz = np.log(u_a), (n_free - 1.0) * np.log(z)
                rhs = lz + (lp_y - lp[:, mov])
                valid = ~(np.isnan(lp_y) | (lp_y == -np.inf))
                acc = valid & (lhs < rhs) & ~dead[:, None]
                if marks:
                    near = valid & (np.abs(lhs - rhs) <= MARGIN_EPS * EPS * (np.abs(lhs) + np.abs(lz) + S_y
                                                                              + S[:, mov]))
                    near, edge = near & ~dead[:, None], edge & ~dead[:, None]
                    n_marginal += int(near.sum())
                    n_edge += int(edge.sum())
                    hit = (near | edge).any(axis=1)
                    first_mark[hit] = np.minimum(first_mark[hit], i)
            x[:, mov] = np.where(acc[:, :, None], y, x[:, mov])
            lp[:, mov] = np.where(acc, lp_y, lp[:, mov])
            S[:, mov] = np.where(acc, S_y, S[:, mov])
            accepted[:, mov] += acc
        if s >= keep_from and (s - keep_from) % thin == 0:
            chain[:, i_keep], kept_lp[:, i_keep], kept_S[:, i_keep] = x, lp, S
            i_keep += 1
    end, end_lp = x.copy(), lp.copy()
    chain[dead], kept_lp[dead], end[dead], end_lp[dead] = np.nan, np.nan, np.nan, np.nan
    return dict(chain=chain, logp=kept_lp, S=kept_S, accepted=accepted, end=end, end_logp=end_lp, status=status,
                first_mark=first_mark, n_marginal=n_marginal, n_edge=n_edge,
                n_decisions=int((~dead).sum()) * W * n_steps)


def logp_window(kind, S):
    """how far a stored lp may lie from the restatement's (module docstring)"""
    return LOGP_ULPS * EPS * S if kind in LLH_KINDS else np.zeros_like(S)


# ------------------------------------------------------------------------------------------- the seeded cases
SEED = 0x5EED0F1357BD2468
_CASES = {}


def case(kind, P, B, J, W, bounds="box", seed_tag=0):
    """dict(pr: the problems (rows gathered), x0 [P, W, J], and the raw arrays D [T, B], E, S2 [K, B], R [K, J, B], ips,
    c [K, J], lo, hi [K, J] or None, t_of, k_of) of a seeded family: T = 3 data rows and K = 4 templates at 30 to 300
    counts per bin, 10 % cosine responses, unit priors on the odd parameters, one NaN bin and one bin without response
    (where B >= 3).  bounds: "none" (NULL), "box" (+-1.5), "one" (lower bounds only, upper infinite), "pin" (the last
    parameter pinned at 0.25, the others boxed).  The starts are N(0, 0.1) about 0 inside the box."""
    key = (kind, P, B, J, W, bounds, seed_tag)
    if key in _CASES:
        return _CASES[key]
    rs = ec._rs("posterior", kind, P, B, J, W, bounds, seed_tag)
    T, K = 3, 4
    lev = 30.0 + 270.0 * rs.rand(B)
    E = lev[None, :] * (1.0 + 0.05 * np.sin(np.arange(K)[:, None] + 0.3 * np.arange(B)[None, :]))
    R = 0.1 * pc._cosines(K, J, B) * E[:, None, :]
    D = rs.poisson(E[np.arange(T) % K]).astype(np.float64)
    if B >= 3:
        D[:, 1] = np.nan
        R[:, :, 2] = 0.0
    S2 = np.abs(0.3 * E * rs.randn(K, B))
    ips = (np.arange(J) % 2).astype(np.float64)
    c = 0.2 * np.sin(1.0 + np.arange(K)[:, None] + np.arange(J)[None, :])
    lo = hi = None
    if bounds != "none":
        lo = np.full((K, J), -1.5) - 0.1 * np.arange(K)[:, None]
        hi = np.full((K, J), 1.5) if bounds != "one" else np.full((K, J), np.inf)
        if bounds == "pin":
            lo[:, J - 1] = hi[:, J - 1] = 0.25
    t_of = (np.arange(P) * 2) % T
    k_of = (np.arange(P) * 3 + 1) % K
    x0 = 0.1 * rs.randn(P, W, J)
    if bounds == "pin":
        x0[:, :, J - 1] = 0.25
    out = dict(D=D, E=E, S2=S2, R=R, ips=ips, c=c, lo=lo, hi=hi, t_of=t_of.astype(np.int32), k_of=k_of.astype(np.int32),
               x0=x0, pr=problems(kind, D, E, R, S2, ips, c, lo, hi, t_of, k_of))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = out
    return out


def layout(kind, J, W):
    """(problems of a workgroup, the most bins it keeps in LDS): `kernels.posterior_layout`, restated so that the
    cases below exist without the library (tests/test_gpu_posterior.py compares the two)"""
    per = min(128 // (W // 2), 32)
    return per, 4096 // (per * (J + 2 + (kind == "mod_chi2")))


# (kind, P, B, J, W, bounds, n_steps, first_step): every (J, W) of {(1, 2), (1, 16), (3, 34), (8, 16), (8, 256)} --
# H = 17 divides nothing and is no power of two, 256 spans both wavefronts --, B of {1, 63, 64, 65, 257, the LDS stage
# and one more}, P of {1, 5, one more than a workgroup's problems, 70}, all kinds and bounds, steps up to 2^32 - 1
GPU_CASES = (
    ("llh", 1, 1, 1, 2, "box", 64, 0),
    ("poisson_llh", 5, 63, 1, 16, "none", 48, 7),
    ("chi2", 70, 64, 3, 34, "one", 32, 0),
    ("mod_chi2", layout("mod_chi2", 3, 34)[0] + 1, 65, 3, 34, "pin", 32, 1000),
    ("llh", 5, 257, 8, 16, "box", 24, 0),
    ("poisson_llh", layout("poisson_llh", 8, 256)[0] + 1, layout("poisson_llh", 8, 256)[1] + 1, 8, 256, "pin", 16, 0),
    ("chi2", 1, 64, 8, 256, "none", 64, 2 ** 32 - 64),
    ("mod_chi2", layout("mod_chi2", 1, 2)[0] + 1, 3, 1, 2, "one", 64, 0),
    ("llh", layout("llh", 8, 16)[0] + 1, layout("llh", 8, 16)[1], 8, 16, "one", 24, 5),
    ("poisson_llh", 5, layout("poisson_llh", 8, 16)[1] + 1, 8, 16, "box", 24, 5),
)


def gpu_case_id(q):
    return "%s-P%d-B%d-J%d-W%d-%s-n%d-s%d" % q


_WANT = {}


def gpu_want(q):
    """(the case, the restatement's chains with every step kept) of a GPU case: computed once, shared, read-only"""
    if q not in _WANT:
        kind, P, B, J, W, bounds, n_steps, first = q
        f = case(kind, P, B, J, W, bounds)
        _WANT[q] = (f, sample(f["pr"], f["x0"], n_steps, SEED, stream=3, chain_id=np.arange(P) + 11, first_step=first))
    return _WANT[q]


# ------------------------------------------------------------------- exactly known targets (the statistical tests)
def gauss_target(J):
    """Zero response, one bin: the posterior is the Gaussian prior N(-c_j, sigma_j) truncated to the box; coordinate 0
    has the one-sided bound lo = mean - sigma / 2, the others +-4 sigma about their means.  -> (problem arrays, exact
    mean [J], exact variance [J], sigma [J])"""
    from scipy.stats import truncnorm

    sigma = 0.5 + 0.25 * np.arange(J)
    mean = 0.1 * np.arange(J) - 0.2
    lo = mean - 4.0 * sigma
    hi = mean + 4.0 * sigma
    lo[0], hi[0] = mean[0] - 0.5 * sigma[0], np.inf
    a, b = (lo - mean) / sigma, (hi - mean) / sigma
    m, v = truncnorm.stats(a, b, loc=mean, scale=sigma, moments="mv")
    arrays = dict(D=np.array([[7.0]]), E=np.array([[5.0]]), R=np.zeros((1, J, 1)), ips=1.0 / sigma,
                  c=-mean[None, :], lo=lo[None, :], hi=hi[None, :])
    return arrays, np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64), sigma


def poisson_target(d):
    """J = 1, one bin, mu = E + R eta with a flat prior on the box, llh: p(mu) ~ mu^d e^-mu on [mu_lo, mu_hi], a
    truncated gamma law.  -> (problem arrays, exact mean and variance of eta)"""
    from scipy.special import gammainc, gamma

    E, R, lo, hi = 4.0, 2.0, -1.5, 3.0
    mu_lo, mu_hi = E + R * lo, E + R * hi

    def moment(k):      # integral of mu^(d + k) e^-mu over [mu_lo, mu_hi]
        a = d + k + 1.0
        return gamma(a) * (gammainc(a, mu_hi) - gammainc(a, mu_lo))

    m1 = moment(1) / moment(0)
    m2 = moment(2) / moment(0)
    arrays = dict(D=np.array([[float(d)]]), E=np.array([[E]]), R=np.full((1, 1, 1), R), ips=None, c=None,
                  lo=np.array([[lo]]), hi=np.array([[hi]]))
    return arrays, (m1 - E) / R, (m2 - m1 * m1) / (R * R)


# (J, W): tau of the walker-mean series in steps (emcee's estimate, `autocorr_time`), the largest over the parameters
# and the targets, measured with the restatement on the CPU: 32 replicas, 1000 steps dropped, 6000 kept (12000 for
# J = 8).  Gaussian target: 32.5 at (1, 16) with acceptance 0.81, 48.2 at (3, 16) with 0.62, 130.5 at (8, 32) with 0.44;
# one-bin Poisson target at (1, 16): 39.1 (d = 0, acceptance 0.75) and 29.5 (d = 3, 0.80).  DESIGN.md §4 quotes the
# table.  -> (burn-in, kept steps): burn-in >= 10 tau, kept >= 50 tau
TAU = {(1, 16): 39.1, (3, 16): 48.2, (8, 32): 130.5}
LENGTHS = {(1, 16): (400, 2000), (3, 16): (500, 2500), (8, 32): (1400, 6600)}
REPLICAS = 32


def replica_moments(pr_arrays, kind, J, W, burn, keep, center, spread, sampler=None):
    """M = 32 replicas of one problem as one batch (chain ids 0..31) -> per replica the mean and the variance of every
    parameter over the kept steps and the walkers"""
    pr = problems(kind, pr_arrays["D"], pr_arrays["E"], pr_arrays["R"], None, pr_arrays["ips"], pr_arrays["c"],
                     pr_arrays["lo"], pr_arrays["hi"], t_of=np.zeros(REPLICAS, dtype=int),
                     k_of=np.zeros(REPLICAS, dtype=int))
    rs = np.random.RandomState(1234 + J)
    x0 = center + spread * rs.uniform(-0.5, 0.5, size=(REPLICAS, W, J))
    x0 = np.minimum(np.maximum(x0, pr["lo"][:, None, :]), pr["hi"][:, None, :])
    run = sample if sampler is None else sampler
    out = run(pr, x0, burn + keep, SEED + J, stream=9, chain_id=np.arange(REPLICAS), keep_from=burn, marks=False)
    flat = out["chain"].reshape(REPLICAS, keep * W, J)
    return flat.mean(axis=1), flat.var(axis=1), out


def check_moments(got, exact, post_sigma, what):
    """|mean over replicas - exact| <= 5 std over replicas / sqrt(M), and that error <= 0.05 posterior sigma (for a
    variance: 0.05 posterior variance), so that noise cannot pass the test"""
    err = got.std(axis=0, ddof=1) / np.sqrt(REPLICAS)
    print(what, "estimate", got.mean(axis=0), "exact", exact, "error", err)
    assert np.all(err <= 0.05 * post_sigma), (what, err, post_sigma)
    assert np.all(np.abs(got.mean(axis=0) - exact) <= 5.0 * err), (what, got.mean(axis=0), exact, err)



def invalid_calls(lib):
    """(name, the call's return code) for every refusal the header lists, on pointers that are never read"""
    import ctypes

    p = ctypes.c_void_p(4096)             # (any non-NULL address: the checks come before any device access)
    base = dict(kind=0, D=p, E=p, S2=None, R=p, r_stride=0, ips=None, c=None, lo=None, hi=None, b_stride=0, J=2, T=3,
                K=3, B=5, P=3, t_of=None, k_of=None, ids=None, W=8, x0=p, seed=1, stream=0, first=0, n=10, keep_from=0,
                thin=1, n_keep=10, chain=p, logp=p, acc=p, end=None, pstat=p, stat=p)

    def call(**kw):
        a = dict(base, **kw)
        return lib.pisa_hip_posterior_sample(
            a["kind"], a["D"], a["E"], a["S2"], a["R"], a["r_stride"], a["ips"], a["c"], a["lo"], a["hi"],
            a["b_stride"], a["J"], a["T"], a["K"], a["B"], a["P"], a["t_of"], a["k_of"], a["ids"], a["W"], a["x0"],
            a["seed"], a["stream"], a["first"], a["n"], a["keep_from"], a["thin"], a["n_keep"], a["chain"], a["logp"],
            a["acc"], a["end"], a["pstat"], a["stat"], None)

    cases = [("kind 4", dict(kind=4)), ("kind -1", dict(kind=-1)), ("J 0", dict(J=0)), ("J 9", dict(J=9, W=32)),
             ("W odd", dict(W=7)), ("W 0", dict(W=0)), ("W 258", dict(W=258)), ("W < 2 J", dict(W=2)),
             ("thin 0", dict(thin=0)), ("steps beyond 2^32", dict(first=2 ** 32 - 5)), ("first < 0", dict(first=-1)),
             ("no steps", dict(n=0, n_keep=0)), ("P 0", dict(P=0)), ("B 2^31", dict(B=2 ** 31)),
             ("wrong n_keep", dict(n_keep=9)), ("2^40 bytes", dict(P=2 ** 31 - 1, t_of=p, k_of=p, n=2 ** 20,
                                                                    n_keep=2 ** 20, W=256, J=8)),
             ("response stride", dict(r_stride=9)), ("bound stride", dict(lo=p, b_stride=1)),
             ("NULL data", dict(D=None)), ("NULL expected", dict(E=None)), ("NULL response", dict(R=None)),
             ("NULL x0", dict(x0=None)), ("NULL chain", dict(chain=None)), ("NULL logp", dict(logp=None)),
             ("NULL accepted", dict(acc=None)), ("NULL problem status", dict(pstat=None)),
             ("NULL status", dict(stat=None)), ("mod_chi2 without sigma2", dict(kind=3)),
             ("more problems than data rows", dict(P=4, k_of=p)), ("more problems than templates", dict(P=4, t_of=p))]
    return [(name, call(**kw)) for name, kw in cases]



# ------------------------------------------------------------------- the batch evaluator restated in numpy
def _solver_base():
    from tests import observed_cases as oc

    return oc.NumpySolver


class NumpySolver(_solver_base()):
    """`observed_cases.NumpySolver` plus `posterior` (`sample`) and `draw_linear_at` (`truth_cases.block` on given
    truths): the batch evaluator of `posterior_sample` and `truths=` restated in numpy"""

    def posterior(self, kind, data, expected, response, x0, n_steps, seed, t_of=None, k_of=None, sigma2=None,
                  inv_prior_sigma=None, center=None, lower=None, upper=None, stream=0, chain_id=None, first_step=0,
                  keep_from=0, thin=1):
        self.calls.append(("posterior", kind, int(n_steps), int(first_step), int(keep_from), int(thin)))
        D = np.atleast_2d(np.asarray(data, dtype=np.float64))
        P = np.shape(x0)[0]
        if t_of is None:
            t_of = np.zeros(P, dtype=int) if D.shape[0] == 1 else np.arange(P)
        pr = problems(kind, D, expected, response, sigma2, inv_prior_sigma, center, lower, upper, t_of, k_of)
        out = sample(pr, x0, int(n_steps), seed, stream, chain_id, int(first_step), int(keep_from), int(thin),
                     marks=False)
        return {k: out[k] for k in ("chain", "logp", "accepted", "end", "status")}

    def draw_linear_at(self, mu, response, sigma, method, eta, seed, stream, first_trial=0):
        from tests import truth_cases as tc

        eta = np.asarray(eta, dtype=np.float64)
        self.calls.append(("draw_linear_at", method, int(eta.shape[0]), int(stream), int(first_trial)))
        blk = tc.block(np.asarray(mu, dtype=np.float64).ravel(), sigma, np.asarray(response, dtype=np.float64), eta,
                       method, seed, stream, first_trial)
        return dict(data=blk[0], eta=eta, clipped=blk[4])
