// profile_device.hpp -- the per-pair solver of profile.hip: the fit of J <= 8 linearised nuisance displacements eta of
// one template row to one data row, and the metric at the fitted point (definition: DESIGN.md §4, "Profiled trial
// ensembles"; restated step for step in tests/profile_cases.py).
//     mu_b(eta) = E_b + R_0b eta_0 + ... + R_(J-1)b eta_(J-1)                       (ascending j, every product rounded)
//     Phi(eta)  = sum_b phi(d_b, mu_b, s2_b) + w sum_j (ips_j (eta_j + c_j))^2
// phi = mu - d ln mu, w = 1/2 (llh, poisson_llh); phi = (d - mu)^2 / (s2 + mu), w = 1 (chi2 with s2 = 0, mod_chi2).
// A damped Newton iteration from eta = 0.  It is written as a state machine around ONE kind of sweep over the bins
// (`pf_bin`: value, exact gradient and exact Hessian of Phi at the trial point eta_t, every sum one chain in ascending
// bin order) so that the caller owns the loop over the bins: the kernel stages them through LDS a chunk at a time and
// all lanes of a workgroup sweep together, a host program walks plain arrays.  After each sweep `pf_decide` accepts
// the trial point or halves the step, factors the Hessian (left-looking Cholesky, the pivot rule of hsfit.hip),
// forms the next step and tests the Newton decrement against the rounding floor of Phi.  When the pair is done,
// one sweep of `pf_value_bin` forms the reported metric at the last accepted eta the way ens_direct_kernel does.
// The bounded form (`pf_init_bounded`, `pf_decide_bounded`; profile_bounded.hip) is the same state machine with a
// projected step: eta_hat minimises Phi over lo_j <= eta_j <= hi_j ("Profiled trial ensembles: bounds";
// restated in tests/profile_bounded_cases.py).
// This file is the home of Phi for every form of the fit.  The wide form (profile_wide_device.hpp), the covariance
// (`pf_hesse_*` below) and the posterior sampler (posterior_device.hpp) take from here the finite test (`pf_finite`),
// phi / phi' / phi'' of a bin (`pf_phi`), its term of `scale` (`pf_scale_term`), the prior term (`pf_prior`,
// `pf_prior_join`) and the bound set (`pf_bound_set`, which `pf_bind` applies).  `pf_bin` and `pf_decide_any`, the two
// functions the 128 narrow kernels spend their registers in, keep the per-bin arithmetic and the prior lines written
// out: calling the helpers there changes the register allocation of those kernels (profiles/r17_profile_shared/).
// No HIP type or call: the same source compiles for the host with a plain C++ compiler; tests/test_host_profiled.py
// and tests/test_host_profiled_bounded.py run it there, under the sanitizers, against the numpy restatements.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PISA_PF_HD __host__ __device__ __forceinline__
#else
#define PISA_PF_HD inline
#endif

namespace pisa {

constexpr int PF_MAX_PARAMS = 8;           // PISA_HIP_PROFILE_MAX_PARAMS
constexpr int PF_LLH = 0, PF_POISSON_LLH = 1, PF_CHI2 = 2, PF_MOD_CHI2 = 3;   // PISA_HIP_METRIC_*
constexpr int PF_NOT_CONVERGED = 1, PF_BOUNDARY = 2, PF_NOT_POSDEF = 4, PF_START_OUTSIDE = 8;   // PISA_HIP_PROFILE_*
constexpr int PF_BAD_BOUNDS = 16;          // (the bounded form alone)
constexpr double PF_SMALL_POS = 1e-10;     // stats.py:40 (SMALL_POS of metric_device.hpp)
constexpr double PF_EPS = 2.220446049250313e-16;
constexpr double PF_PIVOT_REL = 1e-13;     // HS_PIVOT_REL of hsfit.hip
constexpr int PF_MAX_HALVINGS = 40;        // of one step; beyond it the step is below rounding of eta
// The iteration stops at a squared Newton decrement of 2^-20 of Phi's rounding floor, and the step formed there is
// still applied (unchecked: it moves no term of Phi by a part in 10^10).  Stopping at the floor itself leaves eta
// within sqrt(eps) of the minimum, which Phi cannot see but the llh VALUE can: np.nansum drops the -mu of an empty
// bin, so the reported llh is not stationary at eta_hat and an error of eta enters it in first order.
constexpr double PF_STOP_REL = 9.5367431640625e-07;

template <int KIND>
struct PfKind {
    static constexpr bool is_llh = KIND == PF_LLH || KIND == PF_POISSON_LLH;
    static constexpr double w = is_llh ? 0.5 : 1.0;
};

// (s, c) += x with the rounding error of the addition kept in c: `ens_two_sum` of ensemble.hip
PISA_PF_HD void pf_two_sum(double &s, double &c, double x) {
    const double t = s + x;
    const double bb = t - s;
    c += (s - (t - bb)) + (x - bb);
    s = t;
}

// `metric_bin` of metric_device.hpp for the four fused kinds, operation for operation
template <int KIND>
PISA_PF_HD double pf_metric_bin(double k, double lam, double s2) {
    if (lam < PF_SMALL_POS) lam = PF_SMALL_POS;
    if (KIND == PF_LLH) {
        double v = k * log(lam) - lam;
        v -= k * log(k) - k;   // k == 0 -> NaN, dropped
        return v;
    }
    if (KIND == PF_POISSON_LLH) {
        double v = k * log(lam) - lam;
        v -= lgamma(k + 1);
        return v;
    }
    const double d = k - lam;
    return KIND == PF_CHI2 ? (d * d) / lam : (d * d) / (s2 + lam);
}

// packed lower triangle: (i, j), j <= i
PISA_PF_HD constexpr int pf_at(int i, int j) { return i * (i + 1) / 2 + j; }

template <int J>
struct PfState {
    double eta[J];      // the last accepted point
    double eta_t[J];    // the trial point of the running sweep
    double step[J];     // the Newton step from eta
    double g[J];        // sweep: gradient of Phi at eta_t
    double H[J * (J + 1) / 2];   // sweep: Hessian at eta_t; after `pf_decide` its Cholesky factor
    double phi_s, phi_c, scale;  // sweep: compensated sum of phi_b; sum of |phi_b| + 1 + |phi'_b| (|E_b| + sum_j |R_jb eta_j|)
    double Phi, floor_, alpha;   // at eta: Phi and its rounding floor; the share of `step` of the trial point
    double lam2;                 // at eta: the squared Newton decrement of `step`
    int32_t n_iter, n_halve, status;
    uint32_t on_bound;           // the bounded form: bit j: eta_t[j] == lo[j], bit 8 + j: eta_t[j] == hi[j] (`pf_hold`)
    bool inside, cut, boundary, first, done;
};

template <int J>
PISA_PF_HD void pf_init(PfState<J> &st) {
#pragma unroll
    for (int j = 0; j < J; j++) st.eta[j] = st.eta_t[j] = st.step[j] = 0.0;
    st.Phi = st.floor_ = st.lam2 = 0.0;
    st.alpha = 1.0;
    st.n_iter = st.n_halve = st.status = 0;
    st.on_bound = 0;
    st.cut = st.boundary = st.done = false;
    st.first = true;
}

// x held inside [lo, hi].  Comparisons, not fmin / fmax: a NaN passes through unchanged, and a clamped coordinate
// holds the bound's own double, so that `eta == bound` recognises it.
PISA_PF_HD double pf_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// x [J] held inside the box, and which of its coordinates now equal a bound.  The bounds are read here, where a step
// has just been formed and gradient and Hessian are dead, and nowhere else: `pf_bind` needs the marks alone.
template <int J>
PISA_PF_HD void pf_hold(PfState<J> &st, double *x, const double *lo, const double *hi) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const double l = lo[j], h = hi[j], y = pf_clamp(x[j], l, h);
        if (y == l) m |= 1u << j;
        if (y == h) m |= 0x100u << j;
        x[j] = y;
    }
    st.on_bound = m;
}

// the bounded form ("Profiled trial ensembles: bounds"): the fit starts at 0 held inside the box.  A
// box with a bound that does not satisfy lo <= hi (a NaN among them) is refused: the pair takes no step, eta = 0.
template <int J>
PISA_PF_HD void pf_init_bounded(PfState<J> &st, const double *lo, const double *hi) {
    pf_init<J>(st);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < J; j++)
        if (!(lo[j] <= hi[j])) ok = false;
    if (!ok) {
        st.status |= PF_BAD_BOUNDS;
        st.done = true;
        return;
    }
    pf_hold<J>(st, st.eta_t, lo, hi);
#pragma unroll
    for (int j = 0; j < J; j++) st.eta[j] = st.eta_t[j];
}

template <int J>
PISA_PF_HD void pf_sweep_begin(PfState<J> &st) {
#pragma unroll
    for (int j = 0; j < J; j++) st.g[j] = 0.0;
#pragma unroll
    for (int q = 0; q < J * (J + 1) / 2; q++) st.H[q] = 0.0;
    st.phi_s = st.phi_c = st.scale = 0.0;
    st.inside = true;
}

// mu_b at `eta`; `responds`: some R_jb != 0; `reach`: the sum of the absolute values of the terms of mu_b
template <int J>
PISA_PF_HD double pf_mu(double e, const double *r, const double *eta, bool &responds, double &reach) {
    double mu = e;
    reach = fabs(e);
    responds = false;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const double t = r[j] * eta[j];
        mu = mu + t;
        reach += fabs(t);
        if (r[j] != 0.0) responds = true;
    }
    return mu;
}

// a bin with a non-finite datum or expectation takes no part in any sum (the direct form drops it)
PISA_PF_HD bool pf_finite(double d, double e) { return (d == d) && (e == e) && !isinf(d) && !isinf(e); }

// phi, phi', phi'' of one admitted bin at m: the per-bin arithmetic of Phi for every form but `pf_bin` below
template <int KIND>
PISA_PF_HD void pf_phi(double d, double m, double s2, double &phi, double &p1, double &p2) {
    if (PfKind<KIND>::is_llh) {
        const double q = d / m;
        phi = m - d * log(m);
        p1 = 1.0 - q;
        p2 = q / m;
    } else {
        const double v = KIND == PF_MOD_CHI2 ? s2 + m : m;
        const double rr = d - m, a = rr / v;
        const double u = (KIND == PF_MOD_CHI2 ? d + s2 : d) / v;
        phi = rr * a;
        p1 = -(a * (2.0 + a));
        p2 = 2.0 * (u * u) / v;
    }
}

// the bin's term of `scale` (mu is a rounded sum: Phi sees it through phi')
PISA_PF_HD double pf_scale_term(double phi, double p1, double reach) { return (fabs(phi) + 1.0) + fabs(p1) * reach; }

// one bin of a sweep at eta_t.  A bin with a non-finite datum or expectation takes no part (the direct form drops it).
// OWN COPY of `pf_finite`, `pf_phi` and `pf_scale_term`, operation for operation: with the calls, 7 of the 64 unbounded
// narrow kernels change their count of spilled SGPRs (the inliner orders the blocks of `log` differently).  A change
// of Phi is made in `pf_phi` AND here; tests/test_gpu_profiled_wide.py holds the two together bit for bit.
template <int KIND, int J>
PISA_PF_HD void pf_bin(PfState<J> &st, double d, double e, double s2, const double *r) {
    const bool finite = (d == d) && (e == e) && !isinf(d) && !isinf(e);
    if (!finite) return;
    bool responds;
    double reach;
    const double mu = pf_mu<J>(e, r, st.eta_t, responds, reach);
    if (responds && !(mu >= PF_SMALL_POS)) {
        st.inside = false;
        return;
    }
    const double m = mu < PF_SMALL_POS ? PF_SMALL_POS : mu;   // (a bin without response: a constant of Phi)
    double phi, p1, p2;
    if (PfKind<KIND>::is_llh) {
        const double q = d / m;
        phi = m - d * log(m);
        p1 = 1.0 - q;
        p2 = q / m;
    } else {
        const double v = KIND == PF_MOD_CHI2 ? s2 + m : m;
        const double rr = d - m, a = rr / v;
        const double u = (KIND == PF_MOD_CHI2 ? d + s2 : d) / v;
        phi = rr * a;
        p1 = -(a * (2.0 + a));
        p2 = 2.0 * (u * u) / v;
    }
    pf_two_sum(st.phi_s, st.phi_c, phi);
    st.scale += (fabs(phi) + 1.0) + fabs(p1) * reach;   // (mu is a rounded sum: Phi sees it through phi')
#pragma unroll
    for (int i = 0; i < J; i++) {
        st.g[i] += p1 * r[i];
        const double hi = p2 * r[i];
#pragma unroll
        for (int j = 0; j <= i; j++) st.H[pf_at(i, j)] += hi * r[j];
    }
}

// H -> its lower Cholesky factor in place (left-looking, column by column).  False if a pivot is not positive, not
// finite, or so small a share of its diagonal entry that its sign is rounding's (hs_factor of hsfit.hip).
template <int J>
PISA_PF_HD bool pf_factor(double *H) {
#pragma unroll
    for (int k = 0; k < J; k++) {
        const double diag = H[pf_at(k, k)];
        double piv = diag;
#pragma unroll
        for (int m = 0; m < k; m++) piv -= H[pf_at(k, m)] * H[pf_at(k, m)];
        if (!(piv > PF_PIVOT_REL * diag) || !(piv > 0.0) || isinf(piv)) return false;
        const double lkk = sqrt(piv);
        H[pf_at(k, k)] = lkk;
#pragma unroll
        for (int i = k + 1; i < J; i++) {
            double v = H[pf_at(i, k)];
#pragma unroll
            for (int m = 0; m < k; m++) v -= H[pf_at(i, m)] * H[pf_at(k, m)];
            H[pf_at(i, k)] = v / lkk;
        }
    }
    return true;
}

// step = -(L L^T)^-1 g; returns the squared Newton decrement g^T H^-1 g = |L^-1 g|^2
template <int J>
PISA_PF_HD double pf_solve(const double *L, const double *g, double *step) {
    double z[J];
    double lam2 = 0.0;
#pragma unroll
    for (int i = 0; i < J; i++) {
        double v = g[i];
#pragma unroll
        for (int m = 0; m < i; m++) v -= L[pf_at(i, m)] * z[m];
        z[i] = v / L[pf_at(i, i)];
        lam2 += z[i] * z[i];
    }
#pragma unroll
    for (int i = J - 1; i >= 0; i--) {
        double v = z[i];
#pragma unroll
        for (int m = i + 1; m < J; m++) v -= L[pf_at(m, i)] * z[m];
        z[i] = v / L[pf_at(i, i)];
        step[i] = -z[i];
    }
    return lam2;
}

template <int J>
PISA_PF_HD void pf_trial(PfState<J> &st) {
#pragma unroll
    for (int j = 0; j < J; j++) st.eta_t[j] = st.eta[j] + st.alpha * st.step[j];
}

template <int J>
PISA_PF_HD void pf_trial_bounded(PfState<J> &st, const double *lo, const double *hi) {
    pf_trial<J>(st);
    pf_hold<J>(st, st.eta_t, lo, hi);
}

// The bound set of the projected Newton step at the accepted eta: the coordinates that sit on a bound with the
// gradient pointing out of the box.  They leave the system that `pf_factor` and `pf_solve` see (g_j = 0, row and
// column j of H those of the unit matrix: their step is 0 and `lam2` is the decrement of the free block).  A
// coordinate on a bound whose gradient points inward stays free; if its Newton step points outward the clamp holds it.
// A pinned coordinate (lo == hi) is no variable and belongs to the set whatever its gradient: at an exact fit the
// gradient is 0 in every coordinate, and a pinned one set free there would bring back the singular Hessian it was
// pinned to avoid.
// the bound set as a mask (bit j: coordinate j), from the marks of `pf_hold` and the gradient
template <int J>
PISA_PF_HD uint32_t pf_bound_set(const PfState<J> &st) {
    const uint32_t on = st.on_bound;   // (of the trial point that has just become eta)
    uint32_t bound = 0;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const double gj = st.g[j];
        const bool at_lo = on >> j & 1u, at_hi = on >> (8 + j) & 1u;
        if ((at_lo && at_hi) || (at_lo && gj > 0.0) || (at_hi && gj < 0.0)) bound |= 1u << j;
    }
    return bound;
}

// the bound set leaves the system
template <int J>
PISA_PF_HD void pf_bind(PfState<J> &st) {
    const uint32_t bound = pf_bound_set<J>(st);
#pragma unroll
    for (int i = 0; i < J; i++) {
        if (bound >> i & 1u) st.g[i] = 0.0;
#pragma unroll
        for (int j = 0; j <= i; j++)
            if ((bound >> i | bound >> j) & 1u) st.H[pf_at(i, j)] = i == j ? 1.0 : 0.0;
    }
}

// The prior term of one coordinate at x: p = ips (x + c), returns its share w p^2 of Phi.  `pf_prior_join` adds the
// term's share to the gradient entry and to the diagonal entry of the Hessian.
template <int KIND>
PISA_PF_HD double pf_prior(double ips, double x, double c, double &p) {
    p = ips * (x + c);
    return PfKind<KIND>::w * (p * p);
}

template <int KIND>
PISA_PF_HD void pf_prior_join(double ips, double p, double &g, double &h) {
    g += (2.0 * PfKind<KIND>::w) * (ips * p);
    h += (2.0 * PfKind<KIND>::w) * (ips * ips);
}

// after a sweep at eta_t: the priors join, the trial point is accepted or the step halved; on acceptance the next
// step is formed.  Sets `done` when the pair has its final eta.  BOUNDED: every trial point and the last step are
// held inside [lo, hi] and the step is that of the free block (`pf_bind`); nothing else differs.
// OWN COPY of `pf_prior` and `pf_prior_join` in its first loop (see `pf_bin`: the narrow kernels' registers).
template <int KIND, int J, bool BOUNDED>
PISA_PF_HD void pf_decide_any(PfState<J> &st, const double *ips, const double *c, const double *lo, const double *hi,
                              int32_t max_iter) {
    constexpr double w = PfKind<KIND>::w;
    double phi_t = st.phi_s + st.phi_c;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const double p = ips[j] * (st.eta_t[j] + c[j]);
        const double pp = w * (p * p);
        phi_t += pp;
        st.scale += pp;
        st.g[j] += (2.0 * w) * (ips[j] * p);
        st.H[pf_at(j, j)] += (2.0 * w) * (ips[j] * ips[j]);
    }
    if (st.first) {
        st.first = false;
        if (!st.inside) {   // a responding bin with E < SMALL_POS: eta stays 0
            st.status |= PF_START_OUTSIDE;
            st.done = true;
            return;
        }
    } else if (!(st.inside && (phi_t <= st.Phi + st.floor_ || st.lam2 <= st.floor_))) {
        // (a step whose decrement is below Phi's floor cannot be judged by Phi: it is taken if it stays inside)
        if (!st.inside) st.cut = true;
        if (++st.n_halve > PF_MAX_HALVINGS) {
            st.status |= PF_NOT_CONVERGED;
            st.boundary = st.cut;
            st.done = true;
            return;
        }
        st.alpha *= 0.5;
        if (BOUNDED)
            pf_trial_bounded<J>(st, lo, hi);
        else
            pf_trial<J>(st);
        return;
    }
    // accepted
#pragma unroll
    for (int j = 0; j < J; j++) st.eta[j] = st.eta_t[j];
    st.Phi = phi_t;
    st.floor_ = (0.5 * PF_EPS) * st.scale;
    st.boundary = st.cut;
    if (BOUNDED) pf_bind<J>(st);
    if (!pf_factor<J>(st.H)) {
        st.status |= PF_NOT_POSDEF;
        st.done = true;
        return;
    }
    st.lam2 = pf_solve<J>(st.H, st.g, st.step);
    if (st.lam2 <= PF_STOP_REL * st.floor_) {
#pragma unroll
        for (int j = 0; j < J; j++) st.eta[j] = st.eta[j] + st.step[j];
        if (BOUNDED) pf_hold<J>(st, st.eta, lo, hi);
        st.boundary = false;   // a stationary point inside the domain, however the last step got there
        st.done = true;
        return;
    }
    if (st.n_iter >= max_iter) {
        st.status |= PF_NOT_CONVERGED;
        st.done = true;
        return;
    }
    st.n_iter++;
    st.alpha = 1.0;
    st.n_halve = 0;
    st.cut = false;
    if (BOUNDED)
        pf_trial_bounded<J>(st, lo, hi);
    else
        pf_trial<J>(st);
}

template <int KIND, int J>
PISA_PF_HD void pf_decide(PfState<J> &st, const double *ips, const double *c, int32_t max_iter) {
    pf_decide_any<KIND, J, false>(st, ips, c, nullptr, nullptr, max_iter);
}

template <int KIND, int J>
PISA_PF_HD void pf_decide_bounded(PfState<J> &st, const double *ips, const double *c, const double *lo,
                                  const double *hi, int32_t max_iter) {
    pf_decide_any<KIND, J, true>(st, ips, c, lo, hi, max_iter);
}

template <int J>
PISA_PF_HD int32_t pf_status(const PfState<J> &st) {
    return st.status | (st.boundary ? PF_BOUNDARY : 0);
}

// ------------------------------------------------------------------ the covariance of the displacements at eta
// (profile_hesse.hip; DESIGN.md §4, "Profiled trial ensembles: covariance and pulls"; restated in tests/hesse_cases.py)
constexpr int PF_HELD = 32;                // PISA_HIP_PROFILE_HELD: a coordinate of the bound set has zero rows and columns

// inv (packed lower triangle) = (L L^T)^-1 from the factor L of `pf_factor`: column k is the solution of
// L L^T x = e_k by forward and back substitution, of which the entries i >= k are kept (the forward solution is 0
// above k, and the back substitution of entry i reads the entries below it alone).
template <int J>
PISA_PF_HD void pf_inverse(const double *L, double *inv) {
#pragma unroll
    for (int k = 0; k < J; k++) {
        double z[J];
#pragma unroll
        for (int i = k; i < J; i++) {
            double v = i == k ? 1.0 : 0.0;
#pragma unroll
            for (int m = k; m < i; m++) v -= L[pf_at(i, m)] * z[m];
            z[i] = v / L[pf_at(i, i)];
        }
#pragma unroll
        for (int i = J - 1; i >= k; i--) {
            double v = z[i];
#pragma unroll
            for (int m = i + 1; m < J; m++) v -= L[pf_at(m, i)] * z[m];
            z[i] = v / L[pf_at(i, i)];
            inv[pf_at(i, k)] = z[i];
        }
    }
}

// Before the one sweep of `pf_bin`: the point eta becomes the sweep's point, held inside the box where there is one
// (`boxed`; lo and hi are not read otherwise; a point of the domain inside its box is not moved, and its coordinates
// on a bound are marked).  False, and nothing else, for a box with a bound that does not satisfy lo <= hi:
// PF_BAD_BOUNDS.
template <int J>
PISA_PF_HD bool pf_hesse_begin(PfState<J> &st, const double *eta, const double *lo, const double *hi, bool boxed) {
    pf_init<J>(st);
#pragma unroll
    for (int j = 0; j < J; j++) st.eta_t[j] = eta[j];
    if (boxed) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < J; j++)
            if (!(lo[j] <= hi[j])) ok = false;
        if (!ok) return false;
        pf_hold<J>(st, st.eta_t, lo, hi);
    }
    pf_sweep_begin<J>(st);
    return true;
}

// After the sweep: the prior terms join gradient and Hessian as in `pf_decide_any`, the bound set leaves the system
// (`pf_bind`), the free block is factored (`pf_factor`, its pivot rule) and inverted, and
//     cov = c H^-1,  c = 1 for the llh kinds (Phi is -ln L), c = 2 for the chi2 kinds (Phi is chi2 = -2 ln L + const)
// goes to `cov` (packed lower triangle) with zero rows and columns for the bound set.  Returns the status bits:
// PF_START_OUTSIDE (eta is outside the domain: a responding bin with mu < 1e-10), PF_NOT_POSDEF -- `cov` is not
// written then --, or PF_HELD where the bound set is not empty, else 0.
template <int KIND, int J>
PISA_PF_HD int32_t pf_hesse_end(PfState<J> &st, const double *ips, const double *c, double *cov) {
#pragma unroll
    for (int j = 0; j < J; j++) {
        double p;
        pf_prior<KIND>(ips[j], st.eta_t[j], c[j], p);
        pf_prior_join<KIND>(ips[j], p, st.g[j], st.H[pf_at(j, j)]);
    }
    if (!st.inside) return PF_START_OUTSIDE;
    const uint32_t held = pf_bound_set<J>(st);
    pf_bind<J>(st);
    if (!pf_factor<J>(st.H)) return PF_NOT_POSDEF;
    pf_inverse<J>(st.H, cov);
#pragma unroll
    for (int i = 0; i < J; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            const double v = PfKind<KIND>::is_llh ? cov[pf_at(i, j)] : 2.0 * cov[pf_at(i, j)];
            cov[pf_at(i, j)] = ((held >> i | held >> j) & 1u) ? 0.0 : v;
        }
    }
    return held ? PF_HELD : 0;
}

// ----------------------------------------------------------------------------------- the reported metric at eta
struct PfValue {
    double sum, comp;
    bool differs, negative;
};

PISA_PF_HD void pf_value_begin(PfValue &v) {
    v.sum = v.comp = 0.0;
    v.differs = v.negative = false;
}

// one bin of ens_direct_kernel on the template row mu(eta)
template <int KIND, int J>
PISA_PF_HD void pf_value_bin(PfValue &v, const double *eta, double d, double e, double s2, const double *r) {
    if (!pf_finite(d, e)) return;
    if (d < 0.0 || e < 0.0) v.negative = true;
    bool responds;
    double reach;
    const double lam = pf_mu<J>(e, r, eta, responds, reach);
    if (!(lam == lam) || isinf(lam)) return;
    if (KIND == PF_CHI2) {
        const double lc = lam < PF_SMALL_POS ? PF_SMALL_POS : lam;
        if (!(fabs(d - lc) < 5 * PF_EPS)) v.differs = true;
    }
    const double x = pf_metric_bin<KIND>(d, lam, s2);
    if (x == x) pf_two_sum(v.sum, v.comp, x);
}

// the direct form's entry, then the prior terms in ascending j through the same compensated addition
template <int KIND, int J>
PISA_PF_HD double pf_value_end(const PfValue &v, const double *eta, const double *ips, const double *c) {
    double acc = v.sum + v.comp, comp = 0.0;
    if (KIND == PF_CHI2 && !v.differs) acc = 0.0;
#pragma unroll
    for (int j = 0; j < J; j++) {
        double p;
        const double pp = pf_prior<KIND>(ips[j], eta[j], c[j], p);
        pf_two_sum(acc, comp, PfKind<KIND>::is_llh ? -pp : pp);
    }
    return acc + comp;
}

}  // namespace pisa
