// profile_wide_device.hpp -- the wide form of the per-pair solver of profile_device.hpp: the same fit of linearised
// nuisance displacements, the same damped (or projected) Newton state machine and the same arithmetic, for J up to 32,
// with the work of ONE (trial, template) pair spread over the lanes of a wavefront and the state kept in shared
// memory instead of registers (definition: profile_device.hpp and DESIGN.md §4, "Profiled trial ensembles"; the
// mapping: DESIGN.md §4, "Profiled trial ensembles: more than 8 parameters").
//
// Every accumulator of the serial code is one chain in a fixed order: Phi, `scale`, the entries of g and of H over
// the bins in ascending order, the entries of the Cholesky factor and of both substitutions in ascending m.  Here a
// chain is owned by one lane, which walks it in that order; the per-bin quantities (mu, phi, phi', phi'') come from
// lanes that own bins and are handed over through shared memory.  No floating-point value is ever reduced across
// lanes, and no operation is fused or reordered: at J <= 8 the results are the bits of profile_device.hpp.  The finite
// test, phi / phi' / phi'', the bin's term of `scale` and the prior term are that file's own functions (`pf_finite`,
// `pf_phi`, `pf_scale_term`, `pf_prior`, `pf_prior_join`); what stands here is the wide form's own: the mapping of
// chains to lanes, mu over the staged chunk, the cooperative factor and solve, the judgement of a trial point on the
// scalar lane between their phases, and the executor.
//
// The form of the response (`PFW_LINEAR`, `PFW_LOGLINEAR`) is a template parameter of the two phases whose lanes own
// bins, `pfw_bins` and `pfw_value_bins`, and of nothing else: the log-linear form mu_b = E_b exp(sum_j rho_jb eta_j)
// ("Profiled trial ensembles: the log-linear response") hands the chains another p1, p2 per bin and is
// the same solver from there on.  With the form linear both phases are the code they were before the parameter existed.
//
// Form.  Every cooperative phase is a function of (shared state, lane): it reads what earlier phases wrote and writes
// locations no other lane reads or writes in the same phase.  A driver (`pfw_*` taking an executor X) strings the
// phases together; `x.each(f)` runs f(lane) on every lane and then makes the writes visible: the kernel
// (profile_wide_kernel.hpp) calls f on its own lane and meets the barrier, a host program loops over the lanes.  All
// control flow of a driver depends on shared values read after such a barrier, so it is uniform over the lanes.
// No HIP type or call: tests/test_host_profiled_wide.py compiles this file with a plain C++ compiler and runs it
// under the sanitizers against the numpy restatements.
#pragma once
#include "profile_device.hpp"

namespace pisa {

constexpr int PFW_MAX_PARAMS = 32;         // PISA_HIP_PROFILE_WIDE_MAX_PARAMS
constexpr int PFW_LANES = 64;              // one wavefront per pair
constexpr int PFW_CHUNK = 64;              // bins per chunk: one per lane in the phases whose lanes own bins
constexpr int PFW_LD = PFW_CHUNK + 1;      // doubles between two response rows of the chunk (odd: rows on other banks)
constexpr int PFW_TILE = 4;                // a lane's tile of H is 4 x 4 entries
constexpr int PFW_SCALAR = PFW_LANES - 1;  // the lane of the scalar chains of `pfw_decide` and `pfw_value_end`

// marks of a bin after `pfw_bins` (use) and `pfw_value_bins` (the rest)
constexpr int PFW_SKIP = 0, PFW_USE = 1, PFW_OUTSIDE = 2, PFW_NEGATIVE = 4, PFW_DIFFERS = 8;

constexpr int pfw_padded(int J) { return (J + PFW_TILE - 1) / PFW_TILE * PFW_TILE; }
// doubles of the response chunk behind the state: the rows [J, padded J) are kept zero, so that a tile may read them
constexpr int pfw_chunk_doubles(int J) { return pfw_padded(J) * PFW_LD; }

// The state of one pair (PfState of profile_device.hpp, with the marks of `pf_hold` as one byte per coordinate and
// side), the constants of its template, and the staged chunk of bins.
struct PfwShared {
    double eta[PFW_MAX_PARAMS], eta_t[PFW_MAX_PARAMS], step[PFW_MAX_PARAMS], g[PFW_MAX_PARAMS], z[PFW_MAX_PARAMS];
    double H[PFW_MAX_PARAMS * (PFW_MAX_PARAMS + 1) / 2];
    double ips[PFW_MAX_PARAMS], cen[PFW_MAX_PARAMS], lo[PFW_MAX_PARAMS], hi[PFW_MAX_PARAMS];
    // the chunk: inputs (staged by the caller; bins past the chunk's count are not read) ...
    double cD[PFW_CHUNK], cE[PFW_CHUNK], cS2[PFW_CHUNK];
    // ... and what the lanes that own bins hand to the lanes that own chains
    double p1[PFW_CHUNK], p2[PFW_CHUNK], phi[PFW_CHUNK], sc[PFW_CHUNK];
    int32_t use[PFW_CHUNK];
    double phi_s, phi_c, scale, Phi, floor_, alpha, lam2, value;
    double v_sum, v_comp;
    int32_t n_iter, n_halve, status, act, J, bounded;
    uint8_t at_lo[PFW_MAX_PARAMS], at_hi[PFW_MAX_PARAMS], bound[PFW_MAX_PARAMS];
    uint8_t inside, cut, boundary, first, done, fail, negative, differs;
};

constexpr int PFW_ACT_DONE = 0, PFW_ACT_HALVE = 1, PFW_ACT_ACCEPT = 2;

constexpr int PFW_LINEAR = 0, PFW_LOGLINEAR = 1;   // PISA_HIP_RESPONSE_*: the form of the response

// the response of coordinate j at bin cc of the chunk (`R`: the pfw_chunk_doubles(J) doubles behind the state)
PISA_PF_HD double pfw_r(const double *R, int j, int cc) { return R[j * PFW_LD + cc]; }

// ------------------------------------------------------------------------------------------------ start of a pair
// `pf_init` / `pf_init_bounded`.  The constants ips, cen (and lo, hi where bounded) of the template are in place.
template <class X>
PISA_PF_HD void pfw_init(PfwShared &S, X &x, int J, bool bounded, bool live) {
    x.each([&](int lane) {
        if (lane < J) {
            S.eta[lane] = S.eta_t[lane] = S.step[lane] = 0.0;
            S.at_lo[lane] = S.at_hi[lane] = S.bound[lane] = 0;
        }
        if (lane == PFW_SCALAR) {
            S.J = J;
            S.bounded = bounded;
            S.Phi = S.floor_ = S.lam2 = 0.0;
            S.alpha = 1.0;
            S.n_iter = S.n_halve = S.status = 0;
            S.cut = S.boundary = S.negative = S.differs = 0;
            S.first = 1;
            S.done = live ? 0 : 1;
            if (bounded) {
                bool ok = true;
                for (int j = 0; j < J; j++)
                    if (!(S.lo[j] <= S.hi[j])) ok = false;
                if (!ok) {
                    S.status |= PF_BAD_BOUNDS;
                    S.done = 1;
                }
            }
        }
    });
    if (bounded && !S.done) {
        x.each([&](int lane) {
            if (lane < J) {   // `pf_hold` of the start 0
                const double l = S.lo[lane], h = S.hi[lane], y = pf_clamp(S.eta_t[lane], l, h);
                S.at_lo[lane] = y == l;
                S.at_hi[lane] = y == h;
                S.eta_t[lane] = y;
                S.eta[lane] = y;
            }
        });
    }
}

// ------------------------------------------------------------------------------------------------------- a sweep
// `pf_sweep_begin`
PISA_PF_HD void pfw_sweep_begin(PfwShared &S, int lane) {
    const int J = S.J;
    if (lane < J) S.g[lane] = 0.0;
    for (int q = lane; q < J * (J + 1) / 2; q += PFW_LANES) S.H[q] = 0.0;
    if (lane == PFW_SCALAR) {
        S.phi_s = S.phi_c = S.scale = 0.0;
        S.inside = 1;
    }
}

// The log-linear template of bin cc of the chunk at `eta`: the exponent s from 0 in ascending j with every product
// rounded, then mu = e * exp(s), `exp` and the product rounded once each.  `a`: the sum of |rho_jb eta_j|, formed the
// same way.  A bin responds if e != 0 and some rho_jb != 0; one that does not keeps mu = e exactly (no exp, no product).
PISA_PF_HD double pfw_mu_loglinear(const double *R, const double *eta, int J, int cc, double e, bool &responds,
                                   double &a) {
    double s = 0.0;
    bool any = false;
    a = 0.0;
    for (int j = 0; j < J; j++) {
        const double r = pfw_r(R, j, cc);
        const double t = r * eta[j];
        s = s + t;
        a += fabs(t);
        if (r != 0.0) any = true;
    }
    responds = any && e != 0.0;
    if (!responds) return e;
    const double x = exp(s);
    return e * x;
}

// `pfw_bins` of the log-linear form.  With u = d mu / d eta_j = mu rho_j the bin's share of g_j is (phi' mu) rho_j and
// of H_ij (phi'' mu^2 + phi' mu) rho_i rho_j: the rank-one shape `pfw_chains` takes, with other p1, p2.  A responding
// bin whose mu is not finite (an overflowing exp) or below PF_SMALL_POS is outside the domain; a bin that does not
// respond is a constant of Phi and hands the chains zeros.
template <int KIND>
PISA_PF_HD void pfw_bins_loglinear(PfwShared &S, const double *R, int lane, int nb) {
    if (lane >= nb) return;
    const double d = S.cD[lane], e = S.cE[lane], s2 = S.cS2[lane];
    if (!pf_finite(d, e)) {
        S.use[lane] = PFW_SKIP;
        return;
    }
    bool responds;
    double a;
    const double mu = pfw_mu_loglinear(R, S.eta_t, S.J, lane, e, responds, a);
    if (responds && (!(mu >= PF_SMALL_POS) || isinf(mu))) {
        S.use[lane] = PFW_OUTSIDE;
        return;
    }
    const double m = mu < PF_SMALL_POS ? PF_SMALL_POS : mu;
    double phi, f1, f2;
    pf_phi<KIND>(d, m, s2, phi, f1, f2);
    const double p1 = f1 * m;
    const double p2 = (f2 * m) * m + p1;
    S.use[lane] = PFW_USE;
    S.phi[lane] = phi;
    S.p1[lane] = responds ? p1 : 0.0;
    S.p2[lane] = responds ? p2 : 0.0;
    S.sc[lane] = pf_scale_term(phi, f1, m * (2.0 + a));
}

// Lanes own bins: the part of `pf_bin` that is the bin's own (mu in ascending j with every product rounded, then
// phi, phi', phi'' and the bin's term of `scale`), for bin `lane` of a chunk of nb bins.
template <int KIND, int FORM = PFW_LINEAR>
PISA_PF_HD void pfw_bins(PfwShared &S, const double *R, int lane, int nb) {
    if constexpr (FORM == PFW_LOGLINEAR) {
        pfw_bins_loglinear<KIND>(S, R, lane, nb);
        return;
    }
    if (lane >= nb) return;
    const int J = S.J;
    const double d = S.cD[lane], e = S.cE[lane], s2 = S.cS2[lane];
    if (!pf_finite(d, e)) {
        S.use[lane] = PFW_SKIP;
        return;
    }
    double mu = e, reach = fabs(e);
    bool responds = false;
    for (int j = 0; j < J; j++) {   // `pf_mu`
        const double r = pfw_r(R, j, lane);
        const double t = r * S.eta_t[j];
        mu = mu + t;
        reach += fabs(t);
        if (r != 0.0) responds = true;
    }
    if (responds && !(mu >= PF_SMALL_POS)) {
        S.use[lane] = PFW_OUTSIDE;
        return;
    }
    const double m = mu < PF_SMALL_POS ? PF_SMALL_POS : mu;
    double phi, p1, p2;
    pf_phi<KIND>(d, m, s2, phi, p1, p2);
    S.use[lane] = PFW_USE;
    S.phi[lane] = phi;
    S.p1[lane] = p1;
    S.p2[lane] = p2;
    S.sc[lane] = pf_scale_term(phi, p1, reach);
}

// the number of tiles of the lower triangle, and tile q's block row and column
PISA_PF_HD int pfw_tiles(int J) {
    const int n = pfw_padded(J) / PFW_TILE;
    return n * (n + 1) / 2;
}

PISA_PF_HD void pfw_tile_of(int q, int &bi, int &bj) {
    bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= q) bi++;
    bj = q - bi * (bi + 1) / 2;
}

// Lanes own chains, which continue over the chunks: lanes [0, tiles) a 4 x 4 tile of H each, the next padded J / 4
// lanes four entries of g each, the lane after them Phi, `scale` and `inside`.  Each chain takes the chunk's bins in
// ascending order, as `pf_bin` does, and a bin that takes no part leaves it as it is.  One loop for all lanes, without
// a branch on the lane's role or on the bin's mark: every lane forms the terms of all three kinds of chain on rows of
// its own (the reads of several bins are then in flight together) and keeps the ones it owns.
PISA_PF_HD void pfw_chains(PfwShared &S, const double *R, int lane, int nb) {
    const int J = S.J, tiles = pfw_tiles(J), rows = pfw_padded(J) / PFW_TILE;
    const bool is_tile = lane < tiles, is_g = !is_tile && lane < tiles + rows, is_phi = lane == tiles + rows;
    int bi = 0, bj = 0;
    if (is_tile) pfw_tile_of(lane, bi, bj);
    const int i0 = (is_tile ? bi : is_g ? lane - tiles : 0) * PFW_TILE, j0 = bj * PFW_TILE;
    double acc[PFW_TILE][PFW_TILE], gac[PFW_TILE];
#pragma unroll
    for (int a = 0; a < PFW_TILE; a++) {
        const int i = i0 + a;
        gac[a] = (is_g && i < J) ? S.g[i] : 0.0;
#pragma unroll
        for (int b = 0; b < PFW_TILE; b++) {
            const int j = j0 + b;
            acc[a][b] = (is_tile && i < J && j <= i) ? S.H[pf_at(i, j)] : 0.0;
        }
    }
    double s = S.phi_s, c = S.phi_c, scale = S.scale;
    bool inside = S.inside;
#pragma unroll 4
    for (int cc = 0; cc < nb; cc++) {
        const int u = S.use[cc];
        const bool on = u == PFW_USE;
        if (u == PFW_OUTSIDE) inside = false;
        const double p1 = S.p1[cc], p2 = S.p2[cc];
        double ri[PFW_TILE], rj[PFW_TILE];
#pragma unroll
        for (int a = 0; a < PFW_TILE; a++) ri[a] = pfw_r(R, i0 + a, cc), rj[a] = pfw_r(R, j0 + a, cc);
#pragma unroll
        for (int a = 0; a < PFW_TILE; a++) {
            const double ga = gac[a] + p1 * ri[a];
            gac[a] = on ? ga : gac[a];
            const double hi = p2 * ri[a];
#pragma unroll
            for (int b = 0; b < PFW_TILE; b++) {
                const double ha = acc[a][b] + hi * rj[b];
                acc[a][b] = on ? ha : acc[a][b];
            }
        }
        double s1 = s, c1 = c;
        pf_two_sum(s1, c1, S.phi[cc]);
        const double sc1 = scale + S.sc[cc];
        s = on ? s1 : s, c = on ? c1 : c, scale = on ? sc1 : scale;
    }
#pragma unroll
    for (int a = 0; a < PFW_TILE; a++) {
        const int i = i0 + a;
        if (is_g && i < J) S.g[i] = gac[a];
#pragma unroll
        for (int b = 0; b < PFW_TILE; b++) {
            const int j = j0 + b;
            if (is_tile && i < J && j <= i) S.H[pf_at(i, j)] = acc[a][b];
        }
    }
    if (is_phi) {
        S.phi_s = s, S.phi_c = c, S.scale = scale;
        S.inside = inside;
    }
}

// ------------------------------------------------------------------------------------------ after a sweep: decide
// `pf_hold` of x[lane]
PISA_PF_HD void pfw_hold(PfwShared &S, double *x, int lane) {
    const double l = S.lo[lane], h = S.hi[lane], y = pf_clamp(x[lane], l, h);
    S.at_lo[lane] = y == l;
    S.at_hi[lane] = y == h;
    x[lane] = y;
}

// `pf_trial` / `pf_trial_bounded` of coordinate `lane`
PISA_PF_HD void pfw_trial(PfwShared &S, int lane) {
    if (lane >= S.J) return;
    S.eta_t[lane] = S.eta[lane] + S.alpha * S.step[lane];
    if (S.bounded) pfw_hold(S, S.eta_t, lane);
}

// `pf_factor`, column by column: in column k lane i - k forms the chain of entry (i, k) in ascending m; the pivot's
// lane judges it and writes its root, then the entries below are divided by it.
template <class X>
PISA_PF_HD bool pfw_factor(PfwShared &S, X &x) {
    const int J = S.J;
    for (int k = 0; k < J; k++) {
        x.each([&](int lane) {
            const int i = k + lane;
            if (i >= J) return;
            double v = S.H[pf_at(i, k)];
            const double diag = v;
#pragma unroll 4
            for (int m = 0; m < k; m++) v -= S.H[pf_at(i, m)] * S.H[pf_at(k, m)];
            if (i == k) {
                if (!(v > PF_PIVOT_REL * diag) || !(v > 0.0) || isinf(v))
                    S.fail = 1;
                else
                    S.H[pf_at(k, k)] = sqrt(v);
            } else {
                S.H[pf_at(i, k)] = v;
            }
        });
        if (S.fail) return false;
        if (k + 1 < J)
            x.each([&](int lane) {
                const int i = k + 1 + lane;
                if (i < J) S.H[pf_at(i, k)] = S.H[pf_at(i, k)] / S.H[pf_at(k, k)];
            });
    }
    return true;
}

// `pf_solve`.  Forward: the chain of z_i takes L_im z_m in ascending m, so every lane i > m can take its m-th term as
// soon as z_m stands (each forms z_m = v_m / L_mm itself: the same division, the same bits).  Back: the chain of
// entry i starts with the entry finished last, so one lane walks the whole substitution in the serial order.
template <class X>
PISA_PF_HD void pfw_solve(PfwShared &S, X &x) {
    const int J = S.J;
    x.each([&](int lane) {
        if (lane < J) S.z[lane] = S.g[lane];
        if (lane == PFW_SCALAR) S.lam2 = 0.0;
    });
    for (int m = 0; m < J; m++) {
        x.each([&](int lane) {
            if (lane < m || lane >= J) return;
            const double zm = S.z[m] / S.H[pf_at(m, m)];
            if (lane == m) {
                S.step[m] = zm;   // (z_m, kept apart from the running chains of S.z until the forward pass is over)
                S.lam2 += zm * zm;
            } else {
                S.z[lane] -= S.H[pf_at(lane, m)] * zm;
            }
        });
    }
    x.each([&](int lane) {
        if (lane != 0) return;
        for (int i = 0; i < J; i++) S.z[i] = S.step[i];
        for (int i = J - 1; i >= 0; i--) {
            double v = S.z[i];
#pragma unroll 4
            for (int m = i + 1; m < J; m++) v -= S.H[pf_at(m, i)] * S.z[m];
            S.z[i] = v / S.H[pf_at(i, i)];
            S.step[i] = -S.z[i];
        }
    });
}

// `pf_decide_any` after a sweep at eta_t.  Sets S.done when the pair has its final eta.
template <int KIND, class X>
PISA_PF_HD void pfw_decide(PfwShared &S, X &x, int32_t max_iter) {
    const int J = S.J;
    // the priors join: g and the diagonal of H per coordinate, Phi and `scale` as chains in ascending j; the scalar
    // lane then judges the trial point
    x.each([&](int lane) {
        if (lane < J) {
            double p;
            pf_prior<KIND>(S.ips[lane], S.eta_t[lane], S.cen[lane], p);
            pf_prior_join<KIND>(S.ips[lane], p, S.g[lane], S.H[pf_at(lane, lane)]);
        }
        if (lane != PFW_SCALAR) return;
        double phi_t = S.phi_s + S.phi_c, scale = S.scale;
        for (int j = 0; j < J; j++) {
            double p;
            const double pp = pf_prior<KIND>(S.ips[j], S.eta_t[j], S.cen[j], p);
            phi_t += pp;
            scale += pp;
        }
        S.scale = scale;
        S.fail = 0;
        if (S.first) {
            S.first = 0;
            if (!S.inside) {
                S.status |= PF_START_OUTSIDE;
                S.done = 1;
                S.act = PFW_ACT_DONE;
                return;
            }
        } else if (!(S.inside && (phi_t <= S.Phi + S.floor_ || S.lam2 <= S.floor_))) {
            if (!S.inside) S.cut = 1;
            if (++S.n_halve > PF_MAX_HALVINGS) {
                S.status |= PF_NOT_CONVERGED;
                S.boundary = S.cut;
                S.done = 1;
                S.act = PFW_ACT_DONE;
                return;
            }
            S.alpha *= 0.5;
            S.act = PFW_ACT_HALVE;
            return;
        }
        S.Phi = phi_t;
        S.floor_ = (0.5 * PF_EPS) * scale;
        S.boundary = S.cut;
        S.act = PFW_ACT_ACCEPT;
    });
    if (S.act == PFW_ACT_DONE) return;
    if (S.act == PFW_ACT_HALVE) {
        x.each([&](int lane) { pfw_trial(S, lane); });
        return;
    }
    // accepted; `pf_bind`: the bound set, then the rows and columns it takes out of the system
    x.each([&](int lane) {
        if (lane >= J) return;
        S.eta[lane] = S.eta_t[lane];
        if (S.bounded) {
            const double gj = S.g[lane];
            const bool at_lo = S.at_lo[lane], at_hi = S.at_hi[lane];
            const bool b = (at_lo && at_hi) || (at_lo && gj > 0.0) || (at_hi && gj < 0.0);
            S.bound[lane] = b;
            if (b) S.g[lane] = 0.0;
        }
    });
    if (S.bounded)
        x.each([&](int lane) {
            for (int i = lane; i < J; i += PFW_LANES)
                for (int j = 0; j <= i; j++)
                    if (S.bound[i] | S.bound[j]) S.H[pf_at(i, j)] = i == j ? 1.0 : 0.0;
        });
    if (!pfw_factor(S, x)) {
        x.each([&](int lane) {
            if (lane != PFW_SCALAR) return;
            S.status |= PF_NOT_POSDEF;
            S.done = 1;
        });
        return;
    }
    pfw_solve(S, x);
    if (S.lam2 <= PF_STOP_REL * S.floor_) {
        x.each([&](int lane) {
            if (lane < J) {
                S.eta[lane] = S.eta[lane] + S.step[lane];
                if (S.bounded) pfw_hold(S, S.eta, lane);
            }
            if (lane == PFW_SCALAR) {
                S.boundary = 0;
                S.done = 1;
            }
        });
        return;
    }
    if (S.n_iter >= max_iter) {
        x.each([&](int lane) {
            if (lane != PFW_SCALAR) return;
            S.status |= PF_NOT_CONVERGED;
            S.done = 1;
        });
        return;
    }
    x.each([&](int lane) {
        if (lane != PFW_SCALAR) return;
        S.n_iter++;
        S.alpha = 1.0;
        S.n_halve = 0;
        S.cut = 0;
    });
    x.each([&](int lane) { pfw_trial(S, lane); });
}

PISA_PF_HD int32_t pfw_status(const PfwShared &S) { return S.status | (S.boundary ? PF_BOUNDARY : 0); }

// ----------------------------------------------------------------------------------- the reported metric at eta
PISA_PF_HD void pfw_value_begin(PfwShared &S, int lane) {
    if (lane != PFW_SCALAR) return;
    S.v_sum = S.v_comp = 0.0;
    S.differs = 0;
    S.negative = 0;
}

// lanes own bins: `pf_value_bin` up to the bin's own term (FORM: the template at eta by the form's own function)
template <int KIND, int FORM = PFW_LINEAR>
PISA_PF_HD void pfw_value_bins(PfwShared &S, const double *R, int lane, int nb) {
    if (lane >= nb) return;
    const int J = S.J;
    const double d = S.cD[lane], e = S.cE[lane], s2 = S.cS2[lane];
    int mark = PFW_SKIP;
    if (pf_finite(d, e)) {
        if (d < 0.0 || e < 0.0) mark |= PFW_NEGATIVE;
        double lam = e;
        if constexpr (FORM == PFW_LOGLINEAR) {
            bool responds;
            double a;
            lam = pfw_mu_loglinear(R, S.eta, J, lane, e, responds, a);
        } else {
            for (int j = 0; j < J; j++) {
                const double t = pfw_r(R, j, lane) * S.eta[j];
                lam = lam + t;
            }
        }
        if ((lam == lam) && !isinf(lam)) {
            if (KIND == PF_CHI2) {
                const double lc = lam < PF_SMALL_POS ? PF_SMALL_POS : lam;
                if (!(fabs(d - lc) < 5 * PF_EPS)) mark |= PFW_DIFFERS;
            }
            const double v = pf_metric_bin<KIND>(d, lam, s2);
            if (v == v) {
                mark |= PFW_USE;
                S.phi[lane] = v;
            }
        }
    }
    S.use[lane] = mark;
}

// one lane owns the chain of the value
PISA_PF_HD void pfw_value_chain(PfwShared &S, int lane, int nb) {
    if (lane != PFW_SCALAR) return;
    double s = S.v_sum, c = S.v_comp;
    for (int cc = 0; cc < nb; cc++) {
        const int u = S.use[cc];
        if (u & PFW_NEGATIVE) S.negative = 1;
        if (u & PFW_DIFFERS) S.differs = 1;
        if (u & PFW_USE) pf_two_sum(s, c, S.phi[cc]);
    }
    S.v_sum = s, S.v_comp = c;
}

// `pf_value_end` -> S.value
template <int KIND>
PISA_PF_HD void pfw_value_end(PfwShared &S, int lane) {
    if (lane != PFW_SCALAR) return;
    double acc = S.v_sum + S.v_comp, comp = 0.0;
    if (KIND == PF_CHI2 && !S.differs) acc = 0.0;
    for (int j = 0; j < S.J; j++) {
        double p;
        const double pp = pf_prior<KIND>(S.ips[j], S.eta[j], S.cen[j], p);
        pf_two_sum(acc, comp, PfKind<KIND>::is_llh ? -pp : pp);
    }
    S.value = acc + comp;
}

}  // namespace pisa
