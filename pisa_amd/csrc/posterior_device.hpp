// posterior_device.hpp -- the definition of the nuisance-posterior sampler of posterior.hip, per walker: the
// log-density of the displacements eta of one template row given one data row, the random numbers of a proposal, the
// stretch move and its acceptance ("Trial ensembles: the nuisance posterior"; restated step for step in
// tests/posterior_cases.py).  A Goodman-Weare ensemble sampler (stretch scale a = 2) with emcee's red-blue split.
//
// A problem p: a data row t_p, a template row k_p and W walkers (W even, H = W / 2) in J <= 8 dimensions.
//   log-density  lp(eta) = -Phi(eta) (llh, poisson_llh), -Phi(eta) / 2 (chi2, mod_chi2), Phi the objective of the
//       profile solver (profile_device.hpp) formed as the solver forms it at a trial point: the bins in ascending
//       order, a bin with a non-finite datum or expectation skipped, mu by `pf_mu`, phi of the kind as in `pf_bin`
//       joined by `pf_two_sum`, Phi = phi_s + phi_c, then the prior terms w (ips_j (eta_j + c_j))^2 added in ascending
//       j.  lp = -inf where a responding finite bin has !(mu >= 1e-10), where some eta_j lies outside [lo_j, hi_j],
//       and where Phi is NaN.
//   numbers      Philox4x32-10 of fluctuate_device.hpp under the key of `seed`.  For walker w and the global step
//       number s the blocks A = (0xC0000000 + w, s, stream_id, chain_id) and B = (0xD0000000 + w, s, stream_id,
//       chain_id): u_z = `fl_unit` of A's words 0, 1; u_p = `fl_unit` of A's words 2, 3; u_a = `fl_unit_open` of B's
//       words 0, 1.  (The first word of every other block of the library is <= 2^31 - 2 or 0x80000000 + j, j < 8.)
//   one step     the walkers [0, H) move against the current state of [H, W), then [H, W) against the new state of
//       [0, H).  For a moving walker at x:  z = ((u_z + 1) (u_z + 1)) / 2;  the partner q = min((int)(u_p H), H - 1) of
//       the other half at c;  y_j = c_j + z (x_j - c_j), every operation rounded on its own;  the move is accepted iff
//       lp(y) is neither NaN nor -inf and  log(u_a) < (N - 1) log(z) + (lp(y) - lp(x)),  N the number of coordinates
//       that are not pinned (lo_j < hi_j, or a bound that is infinite).
//   start        every walker's lp is formed at the caller's start; a problem one of whose walkers starts at lp = -inf
//       or NaN is PF_START_OUTSIDE, one with a bound pair that is not lo <= hi PF_BAD_BOUNDS: it does not move.
//   kept         step s is kept iff s >= keep_from and (s - keep_from) % thin == 0.
// The state after a step depends on the rows, the start, (seed, stream_id, chain_id) and the step numbers alone.
// No HIP type or call: the same source compiles for the host with a plain C++ compiler; tests/test_host_posterior.py
// runs it there, under the sanitizers, against the numpy restatement.
#pragma once
#include "fluctuate_device.hpp"
#include "profile_device.hpp"

namespace pisa {

constexpr uint32_t PS_WORD_A = 0xC0000000u;   // first counter word of walker w's block A is PS_WORD_A + w
constexpr uint32_t PS_WORD_B = 0xD0000000u;
constexpr int PS_MAX_WALKERS = 256;

// the sweep of one log-density: the compensated chain of phi_b and whether eta is inside the solver's domain
struct PsSweep {
    double phi_s, phi_c;
    bool inside;
};

PISA_PF_HD void ps_begin(PsSweep &sw) {
    sw.phi_s = sw.phi_c = 0.0;
    sw.inside = true;
}

// one bin at eta: the value of `pf_bin` (`pf_phi`; its derivatives are dropped)
template <int KIND, int J>
PISA_PF_HD void ps_bin(PsSweep &sw, const double *eta, double d, double e, double s2, const double *r) {
    if (!pf_finite(d, e)) return;
    bool responds;
    double reach;
    const double mu = pf_mu<J>(e, r, eta, responds, reach);
    if (responds && !(mu >= PF_SMALL_POS)) {
        sw.inside = false;
        return;
    }
    const double m = mu < PF_SMALL_POS ? PF_SMALL_POS : mu;
    double phi, p1, p2;
    pf_phi<KIND>(d, m, s2, phi, p1, p2);   // (the derivatives are not used)
    pf_two_sum(sw.phi_s, sw.phi_c, phi);
}

// lp at eta after the sweep: the priors join as in `pf_decide_any`; -inf outside the domain or the box, or for a NaN
template <int KIND, int J>
PISA_PF_HD double ps_end(const PsSweep &sw, const double *eta, const double *ips, const double *c, const double *lo,
                         const double *hi) {
    double Phi = sw.phi_s + sw.phi_c, p;
    bool in_box = true;
#pragma unroll
    for (int j = 0; j < J; j++) {
        Phi += pf_prior<KIND>(ips[j], eta[j], c[j], p);
        if (!(eta[j] >= lo[j] && eta[j] <= hi[j])) in_box = false;
    }
    if (!sw.inside || !in_box || Phi != Phi) return -INFINITY;
    return PfKind<KIND>::is_llh ? -Phi : -0.5 * Phi;
}

// false: a bound pair that is not lo <= hi (a NaN among them); `n_free`: the coordinates that are not pinned
template <int J>
PISA_PF_HD bool ps_box(const double *lo, const double *hi, int &n_free) {
    bool ok = true;
    n_free = 0;
#pragma unroll
    for (int j = 0; j < J; j++) {
        if (!(lo[j] <= hi[j])) ok = false;
        if (lo[j] < hi[j] || isinf(lo[j]) || isinf(hi[j])) n_free++;
    }
    return ok;
}

// the three uniforms of walker w at step s
PISA_FL_HD void ps_uniforms(uint32_t w, uint32_t s, uint32_t stream, uint32_t chain, uint32_t k0, uint32_t k1,
                            double &u_z, double &u_p, double &u_a) {
    const FlWords a = fl_philox(PS_WORD_A + w, s, stream, chain, k0, k1);
    const FlWords b = fl_philox(PS_WORD_B + w, s, stream, chain, k0, k1);
    u_z = fl_unit(a.w[0], a.w[1]);
    u_p = fl_unit(a.w[2], a.w[3]);
    u_a = fl_unit_open(b.w[0], b.w[1]);
}

PISA_PF_HD double ps_stretch(double u_z) {
    const double t = u_z + 1.0;
    return (t * t) / 2.0;
}

PISA_PF_HD int ps_partner(double u_p, int H) {
    const int q = (int)(u_p * (double)H);
    return q < H - 1 ? q : H - 1;
}

template <int J>
PISA_PF_HD void ps_propose(const double *x, const double *c, double z, double *y) {
#pragma unroll
    for (int j = 0; j < J; j++) {
        const double dx = x[j] - c[j];
        const double t = z * dx;
        y[j] = c[j] + t;
    }
}

PISA_PF_HD bool ps_accept(double u_a, double z, int n_free, double lp_y, double lp_x) {
    if (lp_y != lp_y || lp_y == -INFINITY) return false;
    const double a = (double)(n_free - 1) * log(z);
    const double rhs = a + (lp_y - lp_x);
    return log(u_a) < rhs;
}

// is step s kept, and the number of kept steps among [first, first + n)
PISA_PF_HD bool ps_kept(int64_t s, int64_t keep_from, int64_t thin) {
    return s >= keep_from && (s - keep_from) % thin == 0;
}

PISA_PF_HD int64_t ps_n_keep(int64_t first, int64_t n, int64_t keep_from, int64_t thin) {
    const int64_t end = first + n;   // (one past the last step)
    int64_t s0 = keep_from;
    if (first > keep_from) s0 = keep_from + (first - keep_from + thin - 1) / thin * thin;
    return s0 >= end ? 0 : (end - s0 + thin - 1) / thin;
}

}  // namespace pisa
