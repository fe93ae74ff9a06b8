// prob3_planned.hip -- the planned (E x coszen) grid evaluation of prob3: fused terms+amplitude
// kernel, two-sided chain kernel, and the host-side plan (pisa_hip_grid_plan_*,
// pisa_hip_prob3_grid_planned).
//
// This translation unit alone is compiled with -ffp-contract=fast (see the Makefile): the
// planned form is equal to the reference's operation order only to rounding anyway (products
// associated in parts, reciprocal quotients), and contraction removes a quarter of its
// instructions, which on these latency-bound kernels is time.  Everything else in the
// library (array / one-kernel grid / event kernels, fused reweight, metric ...) keeps
// -ffp-contract=off.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "prob3_device.hpp"
#include "prob3_plan.hpp"

namespace pisa {

// ------------------------------------------------------- planned grid form
// The work of a grid evaluation is tiny (~0.1 GFLOP); what costs is latency: the
// eigenvalue/projector terms of one (E, density) are a ~15 us dependent chain and a
// row's ordered matrix product is up to 24 dependent 3x3 complex products.  The
// plan (host, once per Earth model / coszen grid) therefore
//   * resolves the reference's layer-matrix cache (numba_osc_kernels.py:236-249)
//     and gives mirrored layers of a row ONE matrix ("pair" = (density, length)),
//   * cuts the pairs of each distinct density into work items of a few pairs,
//   * lists every row's chain as pair indices in path order,
// and an evaluation is two launches:
//   stage A   wave = (distinct density, sign, 64 energies): the terms of (E, rho)
//             -> records terms[sign][density][field][n_e]  (1-3 MB, L2 resident)
//   stage C   workgroup = four waves holding (rows, sign, 64 energies), rows packed by their length (default),
//             or (row, sign, 64 energies) x 2 waves (more rows than the packed form indexes; development
//             library: PISA_HIP_CHAIN_MODE=split): forms each layer matrix
//             A = sum_k phase_k Q_k from the record of the layer's density where it multiplies
//             it (a pair belongs to one row: nothing is computed twice) -- the chain is
//             multiplied from its middle outwards on both sides at once (see
//             prob3_chain_kernel), the row's first two waves join the waves' partial products
//             (LDS), one side each, and the first rotates to the flavour basis and stores P and
//             the gather tables.
// The earlier split is kept as an option of the development library (PISA_HIP_PROB3_FUSED_AMP=0 at plan creation):
//   stage AB  wave = (item of a few pairs of one density, sign, 64 energies): terms in registers,
//             then the item's layer matrices -> amp[sign][pair][18][n_e]; stage C reads them.
//             Stage AB is bound by those stores (20-29 MB per evaluation through HBM).
// Without decay the layer matrices are taken in their SU(3) form (see eigen_terms).
// Stage C associates the product differently from the sequential reference and uses
// fused multiply-adds, so its results agree with prob3_grid_kernel to rounding
// (<= 3e-13 absolute on the probabilities), not bit for bit.
constexpr int CHAIN_GROUPS_DEFAULT = 2;   // waves per row of the unpacked chain launch

// Where a kernel finds the per-evaluation constants.  One parameter point: by value in the
// kernel-argument segment (2.3 KB, scalar loads).  SEVERAL independent parameter points in one launch
// (pisa_hip_prob3_grid_planned_multi: blockIdx.y = 2 * point + sign): an array in device memory, the
// point's block read through the constant address space -- the same scalar loads, from another
// address -- so both forms run the same instructions on the same numbers.
struct ConstsByValue {
    Prob3Consts c;
    static constexpr bool AVG = false;
    __device__ __forceinline__ const Prob3Consts &at(int) const { return c; }
};
struct ConstsByPointer {
    const Prob3Consts *__restrict__ p;
    static constexpr bool AVG = false;
    __device__ __forceinline__ const Prob3Consts &at(int k) const { return p[k]; }
};
// The production-height average (prob3_device.hpp: height_averaged_probs) is a compile-time form of the chain kernel,
// selected by the type of its first argument: the constants as above plus the plan's per-row range of the first
// layer's length.  The plain forms keep their signature and their instructions; the terms kernel takes the base.
template <class Base>
struct WithAvgRange : Base {
    const double *__restrict__ avg_range;   // [n_cz] km, >= 0
    static constexpr bool AVG = true;
};

// host-mapped staging block -> device array of the points' constants (one small launch per batch)
__global__ void __launch_bounds__(256)
prob3_stage_consts_kernel(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst, int n_words) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

template <bool DECAY>
__global__ void __launch_bounds__(64)
prob3_terms_amp_kernel(const Prob3Consts c, const double *__restrict__ energy, int n_e,
                       const double *__restrict__ rho_unique, const int32_t *__restrict__ item_u,
                       const int32_t *__restrict__ item_p0, const int32_t *__restrict__ item_cnt,
                       const double *__restrict__ pair_dist, int n_pairs,
                       double *__restrict__ amp) {
    const int item = blockIdx.x;
    const int side = blockIdx.y;
    const int ie = blockIdx.z * 64 + threadIdx.x;
    if (ie >= n_e) return;
    const double e = energy[ie];
    double rec[PROB3_NF];
    auto store = [&](int f, double v) { rec[f] = v; };
    eigen_terms<DECAY>(c.side[side], c.dm, c.vac_order, e, rho_unique[item_u[item]], store);
    auto load = [&](int f) { return rec[f]; };
    const int p0 = item_p0[item], cnt = item_cnt[item];
    for (int q = 0; q < cnt; q++) {
        mat3 A;
        amplitude_from_terms<DECAY>(load, pair_dist[p0 + q] / e, A);
        const int64_t ns = (int64_t)gridDim.z * 64;  // energy stride: whole tiles, cache-line aligned
        double *o = amp + ((int64_t)(side * n_pairs + p0 + q) * 18) * ns + ie;
        // no decay: rows 0 and 1 of the SU(3) form only (12 of the 18 slots of a pair); the
        // chain kernel completes the third row.  This kernel is bound by these stores.
#pragma unroll
        for (int i = 0; i < (DECAY ? 3 : 2); i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                o[(int64_t)(6 * i + 2 * j) * ns] = A.m[i][j].re;
                o[(int64_t)(6 * i + 2 * j + 1) * ns] = A.m[i][j].im;
            }
    }
}

// Stage A alone: the terms of every (distinct density, sign, energy), field-major so that the
// lanes of a wave (64 energies) read and write contiguously.  Used with the chain kernel's
// AMP mode, which forms each layer matrix from these records where it multiplies it.
template <bool DECAY, class CS>
__global__ void __launch_bounds__(64)
prob3_terms_kernel(const CS cs, const double *__restrict__ energy, int n_e,
                   const double *__restrict__ rho_unique, int n_unique,
                   double *__restrict__ terms) {
    const int u = blockIdx.x;
    const int side = blockIdx.y & 1;
    const int pt = blockIdx.y >> 1;     // parameter point (0 in the one-point form)
    const Prob3Consts &c = cs.at(pt);
    const int ie = blockIdx.z * 64 + threadIdx.x;
    if (ie >= n_e) return;
    const int64_t ns = (int64_t)gridDim.z * 64;
    // fields in pairs, [field / 2][E][2]: the chain kernel reads a record with 16-byte loads
    double *o = terms + ((int64_t)((pt * 2 + side) * n_unique + u) * PROB3_NF) * ns + 2 * (int64_t)ie;
    auto store = [&](int f, double v) { o[(int64_t)(f >> 1) * (2 * ns) + (f & 1)] = v; };
    eigen_terms<DECAY>(c.side[side], c.dm, c.vac_order, energy[ie], rho_unique[u], store);
}

// C = A.B with fused multiply-adds (4 per complex multiply-accumulate instead of 4 mul + 4
// add).  Stage C is a short dependent sequence of 3x3 complex products per wave: instruction
// count is latency.  Only used where the product is already associated differently from the
// sequential reference order (equal to it to rounding either way).
__device__ __forceinline__ void mat_mul_fma(const mat3 &A, const mat3 &B, mat3 &C) {
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double re = A.m[i][0].re * B.m[0][j].re;
            double im = A.m[i][0].re * B.m[0][j].im;
            re = __builtin_fma(-A.m[i][0].im, B.m[0][j].im, re);
            im = __builtin_fma(A.m[i][0].im, B.m[0][j].re, im);
#pragma unroll
            for (int k = 1; k < 3; k++) {
                re = __builtin_fma(A.m[i][k].re, B.m[k][j].re, re);
                im = __builtin_fma(A.m[i][k].re, B.m[k][j].im, im);
                re = __builtin_fma(-A.m[i][k].im, B.m[k][j].im, re);
                im = __builtin_fma(A.m[i][k].im, B.m[k][j].re, im);
            }
            C.m[i][j] = cmake(re, im);
        }
}

// Two-sided form of stage C.  A row's chain, in path order a_0 .. a_{n-1}, is split at its
// middle element m = n/2:   T = (a_{n-1} .. a_{m+1}) . a_m . (a_{m-1} .. a_0).
// Step s pairs the out-going layer a_{m+s} with the in-going layer a_{m-s}; for the mirror
// symmetric paths through the Earth these are the SAME matrix (plan: one pair per distinct
// matrix of a row), so one load feeds two products,  L <- A . L  and  R <- R . A,  which are
// independent of each other (instruction-level parallelism where the one-sided form has a
// single dependent chain).  Wave g of the row takes the g-th part of the steps and leaves its L_g, R_g
// in LDS; the parts are joined as  (L_{G-1} .. (L_1 . L_0)) . (a_m . ((R_0 . R_1) .. R_{G-1})).
// Unpacked launch: wave 0, the leader, multiplies both sides behind the barrier.  Packed launch: the
// two sides on two waves (chain_join_r, chain_join_l) -- the leader multiplies the R parts and a_m . R,
// wave 1 of the row, which gets the leader's L_0 through LDS, the L parts; behind a SECOND barrier
// the leader reads the finished L and closes with  L . (a_m . R): the products, operands and
// association of the one-wave join, so the same bits (tests/test_gpu_prob3_join.py), with three
// products fewer on the critical path of a four-wave row (EXPERIMENTS R16-1).  Valid for any
// sequence (non-mirrored steps just load two matrices); same matrices as the other forms,
// associated differently.
// AMP = 0: layer matrices read from stage AB's `amp`.  AMP = 1 (no decay) / 2 (decay): formed here
// from the stage-A records `terms` of the layer's density (a pair belongs to one row, so nothing
// is computed twice, and the records -- 2 x n_unique x 26 x n_e doubles -- stay in the L2 where
// the amplitudes, 12-18 doubles per pair and energy, had to travel through HBM).
// G = 0: PACKED launch (prob3_plan.hpp decides all of it on the host).  Every workgroup has four waves and holds
// rows by their length -- one long row split over four waves, two medium rows over two waves each, or four short
// rows with a wave each: what bounds this kernel is the dependent sequence of layer matrices per wave of the
// longest rows (13 for a 24-layer row; a step is ~460 vector instructions, ~1 us where a SIMD is shared), and
// four-wave workgroups for EVERY row do not fit the chip at once (244 VGPRs, 63 KB of LDS: two workgroups per CU).
// A 200 x 100 PREM-12 grid has 19 rows of >= 14 layers and 81 shorter ones: 60 row blocks per energy tile.  Its
// fourth tile has 8 live energies; there the rows of one class (same densities in the same order, same mirrored
// steps: 12 classes) share a wave, eight rows side by side, 13 blocks instead of 60: 386 workgroups where 480
// issued a quarter of their instructions for 8 lanes of 64.  The workgroups are launched longest rows first
// over all tiles; the dispatcher puts workgroup 256 + k on the CU of workgroup k, so what a long row shares its
// SIMDs with is decided by this order (EXPERIMENTS R11-1).
// Development build (make EXTRA=-DPISA_CHAIN_STAMPS, scripts/dev/chain_stamps.py): wall-clock stamps of lane 0 of
// every wavefront of the first (point, sign) column of the packed launch at seven points of the kernel, and the XCC,
// shader engine, CU and SIMD it ran on.
#ifdef PISA_CHAIN_STAMPS
__device__ unsigned long long g_chain_stamps[8 * 4096];
#define CSTAMP_SLOT (blockIdx.y + gridDim.y * blockIdx.z)
#define CSTAMP_ON (G == 0 && (threadIdx.x & 63) == 0 && blockIdx.x == 0 && CSTAMP_SLOT < 1024)
#define CSTAMP(k) do { if (CSTAMP_ON) g_chain_stamps[8 * (CSTAMP_SLOT * 4 + (threadIdx.x >> 6)) + (k)] = wall_clock64(); } while (0)
#else
#define CSTAMP(k) do {} while (0)
#endif
template <int G, int AMP, bool AVG>
__device__ __forceinline__ void chain_tail(const Prob3Consts &c, const Prob3Side &S, mat3 &L, mat3 &R, mat3 &T, bool have_l, bool have_r,
                                           const double *s_part, int part_0, int lane, int Gr, int n_steps, int cnt, int mid,
                                           int e_major, int ie, int n_e, int n_cz, int jcz, int side, int n_points, int pt,
                                           double *__restrict__ out, double2 *__restrict__ pepmu, double avg_dl_over_e);

// A wave's partial product in LDS: [L | R][18][lane].  In the packed launch wave w owns slot (w + 3) & 3 -- the
// partners of a leader at wave w are the next slots, and slot 3, wave 0's, has room for an L alone.
constexpr int CHAIN_PART = 2 * 18 * 64;
__device__ __forceinline__ void part_store(double *o, const mat3 &M) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            o[(6 * i + 2 * j) * 64] = M.m[i][j].re;
            o[(6 * i + 2 * j + 1) * 64] = M.m[i][j].im;
        }
}
__device__ __forceinline__ void part_load(const double *o, mat3 &M) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M.m[i][j] = cmake(o[(6 * i + 2 * j) * 64], o[(6 * i + 2 * j + 1) * 64]);
}

// first step of part h of a row's n_steps steps over Gr waves (h = Gr: one past the last step)
template <bool PACKED>
__device__ __forceinline__ int chain_part_begin(int n_steps, int h, int Gr) {
    if constexpr (PACKED) return 1 + ((n_steps * h) >> (Gr >> 1));   // Gr is 1, 2 or 4 (prob3_waves_of)
    else return 1 + (int)(((int64_t)n_steps * h) / Gr);
}

// The join of a packed row over GR = 2 or 4 waves, one side per wave (between the kernel's two barriers), each in the
// order of the one-wave join: the same products on the same operands.
// R side, the leader at wave `wv`:  R <- R . R_h,  h = 1 .. GR-1.  It asks for all of its partners' parts at once and
// multiplies them back to back.
template <int GR>
__device__ __forceinline__ void chain_join_r(mat3 &R, bool &have_r, const double *s_part, int wv, int lane, int n_steps) {
    mat3 P[GR - 1];
#pragma unroll
    for (int h = 1; h < GR; h++) part_load(s_part + ((wv + h + 3) & 3) * CHAIN_PART + 18 * 64 + lane, P[h - 1]);
#pragma unroll
    for (int h = 1; h < GR; h++) {
        if (chain_part_begin<true>(n_steps, h + 1, GR) <= chain_part_begin<true>(n_steps, h, GR)) continue;  // part h had no steps
        if (have_r) { mat3 t; mat_mul_fma(R, P[h - 1], t); R = t; } else { R = P[h - 1]; have_r = true; }
    }
}
// L side, the wave after the leader (it holds L_1):  L <- L_h . L,  h = 1 .. GR-1, from the L_0 the leader left in its
// slot; the product goes to this wave's own slot, where the leader finds it behind the second barrier.  A part has an
// L unless it had no step or its only step was the unpaired last one.  Where every part has one (any row of four
// waves, most of two) this side too asks for its parts at once; else it takes them one at a time -- asking ahead under
// the `have_l` selects takes 257 registers and with them one workgroup per CU (EXPERIMENTS R16-1).
template <int GR>
__device__ __forceinline__ void chain_join_l(const mat3 &L1, double *s_part, int wv, int lane, int n_steps, int cnt, int mid) {
    mat3 L;
    if (n_steps >= GR && mid + chain_part_begin<true>(n_steps, GR - 1, GR) < cnt) {
        mat3 P[GR - 1];   // L_0, L_2 .. L_{GR-1}
#pragma unroll
        for (int h = 0; h < GR; h++)
            if (h != 1) part_load(s_part + ((wv - 1 + h + 3) & 3) * CHAIN_PART + lane, P[h ? h - 1 : 0]);
        mat_mul_fma(L1, P[0], L);
#pragma unroll
        for (int h = 2; h < GR; h++) { mat3 t; mat_mul_fma(P[h - 1], L, t); L = t; }
        part_store(s_part + ((wv + 3) & 3) * CHAIN_PART + lane, L);
        return;
    }
    bool have_l = false;
#pragma unroll
    for (int h = 0; h < GR; h++) {
        const int h0 = chain_part_begin<true>(n_steps, h, GR);
        if (chain_part_begin<true>(n_steps, h + 1, GR) <= h0 || mid + h0 >= cnt) continue;
        mat3 Ph;
        if (h != 1) part_load(s_part + ((wv - 1 + h + 3) & 3) * CHAIN_PART + lane, Ph);
        const mat3 &Lh = h == 1 ? L1 : Ph;
        if (have_l) { mat3 t; mat_mul_fma(Lh, L, t); L = t; } else { L = Lh; have_l = true; }
    }
    if (have_l) part_store(s_part + ((wv + 3) & 3) * CHAIN_PART + lane, L);
}

template <int G, int AMP, class CS = ConstsByValue>
__global__ void __launch_bounds__(G ? 64 * G : 256)
prob3_chain_kernel(const CS cs, int n_e, const int32_t *__restrict__ row_start,
                    const int32_t *__restrict__ row_cnt, const int32_t *__restrict__ row_pairs,
                    int n_cz, int n_pairs, const double *__restrict__ amp, int e_major,
                    double *__restrict__ prob_nu, double *__restrict__ prob_nubar,
                    double2 *__restrict__ pepmu, const double *__restrict__ energy,
                    const int32_t *__restrict__ pair_u, const double *__restrict__ pair_dist,
                    int n_unique, const int32_t *__restrict__ slots, const int2 *__restrict__ lanes, int n_slots,
                    int n_points, int n_tiles) {
    auto MM = [](const mat3 &A_, const mat3 &B_, mat3 &C_) { mat_mul_fma(A_, B_, C_); };
    static_assert(!CS::AVG || AMP == 1, "the production-height average: fused amplitudes without decay only");
    CSTAMP(0);
    // Packed launch: grid = (2 x points, slots): the (point, sign) index runs FASTEST and the slot -- a workgroup's
    // four wave records, which name its energy tile as well (prob3_plan.hpp) -- slowest.  The plan lists the slots
    // longest rows first, so the long rows of every point, sign and tile start first and the short ones come last:
    // what the chip takes beyond one workgroup per CU is the short work.  The fast index is rotated by the slot:
    // consecutive workgroups go to consecutive XCDs, and without the rotation an XCD would see the same few
    // (point, sign) records from all of its CUs at the same moment.
    constexpr bool PACKED = G == 0;
    const int n2 = 2 * n_points;
    const int bx = PACKED ? (int)(blockIdx.y + gridDim.y * blockIdx.z) : (int)blockIdx.x;
    if (PACKED && bx >= n_slots) return;   // (the grid's last y-z plane may be partly empty)
    const int rot = (int)blockIdx.x + bx;
    const int by = !PACKED ? (int)blockIdx.y : ((n2 & (n2 - 1)) == 0 ? (rot & (n2 - 1)) : (rot % n2));
    int bz = PACKED ? 0 : (int)blockIdx.z;
    if (!PACKED) n_tiles = gridDim.z;
    const int pt = by >> 1;     // parameter point (0 in the one-point form)
    const Prob3Consts &c = cs.at(pt);
    // [partial][L|R][18][lane]; packed: a slot per wave, the fourth (wave 0's) an L alone -- 63 KB, two workgroups per CU
    __shared__ double s_part[PACKED ? 3 * CHAIN_PART + 18 * 64 : (G > 1 ? G - 1 : 1) * CHAIN_PART];
    const int lane = threadIdx.x & 63;
    // wave index: uniform within a wave, which the compiler cannot see -- without this the loop
    // bounds derived from it are 'divergent' and every index look-up becomes a vector load
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // row, group of this wave within the row, groups of the row; partial slot of a writer wave
    int jcz = bx, g = wv, Gr = G;
    int k0_blk = 0, cnt_blk = 0;
    // ragged last tile: the wave holds several rows of one class side by side, lane = row-in-group x r + energy.
    // Row, chain start and (per step) layer length are then per lane; density index, chain length, the pattern of
    // mirrored steps and the step bounds are the class's and stay scalar.
    bool ragged = false;
    int jl = 0, k0l = 0, e_in = lane;
    if (PACKED) {
        // (unit | g << 16 | groups << 24 (-1: idle wave), first position and length of the row's chain, energy tile):
        // one 16-byte scalar load instead of the code and then row_start / row_cnt behind it
        const int4 rec = reinterpret_cast<const int4 *>(slots)[bx * 4 + wv];
        const int32_t code = __builtin_amdgcn_readfirstlane(rec.x);
        k0_blk = __builtin_amdgcn_readfirstlane(rec.y);
        cnt_blk = __builtin_amdgcn_readfirstlane(rec.z);
        jcz = code < 0 ? -1 : (code & 0xffff);
        g = code < 0 ? 0 : ((code >> 16) & 0xff);
        Gr = code < 0 ? 1 : ((code >> 24) & 0xff);
        const int32_t tile = __builtin_amdgcn_readfirstlane(rec.w);
        ragged = (tile & PROB3_RAGGED_BIT) != 0;
        bz = tile & ~PROB3_RAGGED_BIT;
        jl = jcz;
        k0l = k0_blk;
        if (ragged && jcz >= 0) {
            const int2 lt = lanes[jcz * 64 + lane];
            jl = lt.x < 0 ? -1 : (lt.x & 0xffff);
            e_in = lt.x < 0 ? 0 : (lt.x >> 16);
            k0l = lt.y;
        }
    } else {
        jl = jcz;
    }
    const int part_w = PACKED ? wv - 1 : g - 1;   // where a wave with g > 0 leaves its partials
    const int part_0 = PACKED ? wv : 0;           // leader: partner h reads slot part_0 + h - 1
    const int side = by & 1;
    const bool decay = AMP == 0 ? c.decay != 0 : AMP == 2;  // full 3x3 matrices stored / formed
    const int ie = bz * 64 + e_in;
    const bool live = ie < n_e && jcz >= 0 && jl >= 0;
    double *out = side == 0 ? prob_nu : prob_nubar;
    const Prob3Side &S = c.side[side];
    const int k0 = PACKED ? k0_blk : (jcz >= 0 ? row_start[jcz] : 0);
    const int cnt = PACKED ? cnt_blk : (jcz >= 0 ? row_cnt[jcz] : 0);
    const int mid = cnt >> 1;
    const int n_steps = mid;  // steps s = 1..mid (out-going side may be one shorter)
    const int s0 = PACKED ? chain_part_begin<true>(n_steps, g, Gr) : 1 + (int)(((int64_t)n_steps * g) / Gr);
    const int s1 = PACKED ? chain_part_begin<true>(n_steps, g + 1, Gr) : 1 + (int)(((int64_t)n_steps * (g + 1)) / Gr);
    const int64_t ns = (int64_t)n_tiles * 64;
    // 1/E once per lane: L/E as a product (one rounding more than the quotient, 1e-16 on a phase)
    const double inv_e = (AMP != 0 && live) ? 1.0 / energy[ie] : 1.0;
    // `pos` = position in the row-pairs list.  In the AMP modes the density index and the length of
    // the layer are read from lists indexed by that position (chain_u / chain_dist) rather than
    // through the pair number: one dependent scalar load less in front of every layer matrix.
    auto load_pair = [&](int pos, mat3 &A) {
        if (AMP != 0) {
            // `amp` holds the stage-A records here
            const double *r = amp + ((int64_t)((pt * 2 + side) * n_unique + pair_u[pos]) * PROB3_NF) * ns + 2 * (int64_t)ie;
            auto load = [&](int f) { return r[(int64_t)(f >> 1) * (2 * ns) + (f & 1)]; };
            const double len = (PACKED && ragged) ? pair_dist[k0l + (pos - k0_blk)] : pair_dist[pos];
            amplitude_from_terms<AMP == 2>(load, len * inv_e, A);
            if (AMP == 1) su3_complete(A);
            return;
        }
        const int k = row_pairs[pos];
        const double *a = amp + ((int64_t)(side * n_pairs + k) * 18) * ns + ie;
#pragma unroll
        for (int i = 0; i < (decay ? 3 : 2); i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                A.m[i][j] = cmake(a[(int64_t)(6 * i + 2 * j) * ns], a[(int64_t)(6 * i + 2 * j + 1) * ns]);
        if (!decay) su3_complete(A);
    };
    mat3 L, R;
    bool have_l = false, have_r = false;
    CSTAMP(1);
#ifdef PISA_CHAIN_STAMPS
    if (CSTAMP_ON)
        g_chain_stamps[8 * (CSTAMP_SLOT * 4 + (threadIdx.x >> 6)) + 7] = (unsigned long long)cnt | ((unsigned long long)g << 16) | ((unsigned long long)Gr << 24) | ((unsigned long long)(s1 - s0) << 32) | (jcz >= 0 ? 1ull << 48 : 0ull) |
            // where the wavefront runs: HW_ID bits 4..15 (SIMD, pipe, CU, shader array, shader engine) and the XCC number
            ((unsigned long long)((__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 4) & 0xfff) << 49) |
            ((unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0x7) << 61);
#endif
    if (live && cnt > 0 && s1 > s0) {
        mat3 A, An;
        load_pair(k0 + mid - s0, A);
        for (int s = s0; s < s1; s++) {
            const int k_in = row_pairs[k0 + mid - s];
            const int k_out = mid + s < cnt ? row_pairs[k0 + mid + s] : -1;
            if (s + 1 < s1) load_pair(k0 + mid - (s + 1), An);  // next in flight
            if (have_r) { mat3 t; MM(R, A, t); R = t; } else { R = A; have_r = true; }
            if (k_out >= 0) {
                if (k_out != k_in) load_pair(k0 + mid + s, A);  // not a mirrored pair (workgroup-uniform)
                if (have_l) { mat3 t; MM(A, L, t); L = t; } else { L = A; have_l = true; }
            }
            A = An;
        }
    }
    CSTAMP(2);
    if (g > 0 && live) {
        double *o = s_part + (size_t)part_w * 2 * 18 * 64 + lane;
        if (have_l && !(PACKED && g == 1)) {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    o[(6 * i + 2 * j) * 64] = L.m[i][j].re;
                    o[(6 * i + 2 * j + 1) * 64] = L.m[i][j].im;
                }
        }
        if (have_r) {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    o[(18 + 6 * i + 2 * j) * 64] = R.m[i][j].re;
                    o[(18 + 6 * i + 2 * j + 1) * 64] = R.m[i][j].im;
                }
        }
    }
    // packed: the leader of a row of several waves hands its L_0 to the wave that joins the L side
    if (PACKED && g == 0 && Gr > 1 && live && have_l) part_store(s_part + ((wv + 3) & 3) * CHAIN_PART + lane, L);
    // the leader forms the middle layer's matrix while it waits for its partners
    mat3 T;
    if (g == 0 && live && cnt > 0) load_pair(k0 + mid, T);
    __syncthreads();
    CSTAMP(3);
    if constexpr (!PACKED) {
        if (g != 0 || !live) return;
        double avg = 0.0;
        if constexpr (CS::AVG) avg = cs.avg_range[jl] * inv_e;
        chain_tail<G, AMP, CS::AVG>(c, S, L, R, T, have_l, have_r, s_part, part_0, lane, Gr, n_steps, cnt, mid, e_major, ie, n_e, n_cz, jl, side,
                                    n_points, pt, out, pepmu, avg);
    } else {
        // The join on two waves: the leader multiplies the R parts and T . R while the next wave of the row multiplies
        // the L parts; every wave of the workgroup meets at the second barrier (idle waves and the partners that have
        // nothing to join pass straight through), and the leader closes with L . (T . R).
        if (live && cnt > 0) {
            if (g == 0) {
                if (Gr == 4) chain_join_r<4>(R, have_r, s_part, wv, lane, n_steps);
                else if (Gr == 2) chain_join_r<2>(R, have_r, s_part, wv, lane, n_steps);
                if (have_r) { mat3 t; MM(T, R, t); T = t; }
                if (Gr == 1 && have_l) { mat3 t; MM(L, T, t); T = t; }
            } else if (g == 1) {
                if (Gr == 4) chain_join_l<4>(L, s_part, wv, lane, n_steps, cnt, mid);
                else chain_join_l<2>(L, s_part, wv, lane, n_steps, cnt, mid);
            }
        }
        __syncthreads();
        if (g != 0 || !live) return;
        // some part has an L as soon as step 1 has an out-going layer
        if (Gr > 1 && n_steps > 0 && mid + 1 < cnt) {
            mat3 t;
            part_load(s_part + ((wv + 1 + 3) & 3) * CHAIN_PART + lane, L);
            MM(L, T, t);
            T = t;
        }
        // joined already: the tail with one wave and no part of its own closes the chain
        double avg = 0.0;
        if constexpr (CS::AVG) avg = cs.avg_range[jl] * inv_e;
        chain_tail<G, AMP, CS::AVG>(c, S, L, R, T, false, false, s_part, 0, lane, 1, n_steps, cnt, mid, e_major, ie, n_e, n_cz, jl, side, n_points, pt,
                                    out, pepmu, avg);
    }
}

// the leader's part of the chain kernel: joins the partial products of its partner waves, closes the chain with the
// mixing matrices and stores the node's probabilities
// AVG: a row with a range of production heights (avg_dl_over_e = dL / E > 0) stores the average over the range of its
// first layer's length instead of |F|^2; a row with range 0 takes the plain expression and gets the plain launch's bits
template <int G, int AMP, bool AVG>
__device__ __forceinline__ void chain_tail(const Prob3Consts &c, const Prob3Side &S, mat3 &L, mat3 &R, mat3 &T, bool have_l, bool have_r,
                                           const double *s_part, int part_0, int lane, int Gr, int n_steps, int cnt, int mid,
                                           int e_major, int ie, int n_e, int n_cz, int jcz, int side, int n_points, int pt,
                                           double *__restrict__ out, double2 *__restrict__ pepmu, double avg_dl_over_e) {
    auto MM = [](const mat3 &A_, const mat3 &B_, mat3 &C_) { mat_mul_fma(A_, B_, C_); };
    // wave 0: T_right = R_0 . R_1 .. (later groups further right), T_left = .. L_1 . L_0
    for (int h = 1; h < Gr; h++) {
        const int h0 = 1 + (int)(((int64_t)n_steps * h) / Gr);
        const int h1 = 1 + (int)(((int64_t)n_steps * (h + 1)) / Gr);
        if (h1 <= h0 || cnt == 0) continue;  // wave-uniform: group h had no steps
        const double *o = s_part + (size_t)(part_0 + h - 1) * 2 * 18 * 64 + lane;
        mat3 Ph;
        // right part of group h always exists when it had steps
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                Ph.m[i][j] = cmake(o[(18 + 6 * i + 2 * j) * 64], o[(18 + 6 * i + 2 * j + 1) * 64]);
        if (have_r) { mat3 t; MM(R, Ph, t); R = t; } else { R = Ph; have_r = true; }
        // its left part exists unless its only step was the unpaired last one
        const bool h_has_l = mid + h0 < cnt;
        if (h_has_l) {
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++)
                    Ph.m[i][j] = cmake(o[(6 * i + 2 * j) * 64], o[(6 * i + 2 * j + 1) * 64]);
            if (have_l) { mat3 t; MM(Ph, L, t); L = t; } else { L = Ph; have_l = true; }
        }
    }
    CSTAMP(4);
    if (cnt > 0) {
        if (have_r) { mat3 t; MM(T, R, t); T = t; }
        if (have_l) { mat3 t; MM(L, T, t); T = t; }
    } else {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) T.m[i][j] = cmake(0.0, 0.0);
    }
    double P[9];
    if (AVG && avg_dl_over_e > 0.0) {
        height_averaged_probs(T, S.U, c.dm, avg_dl_over_e, P);
    } else {
        mat3 t2, Tf;
        MM(T, S.Ud, t2);
        MM(S.U, t2, Tf);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++)
                P[3 * i + j] = Tf.m[j][i].re * Tf.m[j][i].re + Tf.m[j][i].im * Tf.m[j][i].im;
    }
    CSTAMP(5);
    int64_t node = e_major ? (int64_t)ie * n_cz + jcz : (int64_t)jcz * n_e + ie;
    if (n_points > 1) {
        // several points: the gather tables of the points interleaved, [sign][flavour][node][point], so
        // that the multi-point fused kernel fetches an event's pairs of all points in one contiguous run
#pragma unroll
        for (int f = 0; f < 3; f++)
            pepmu[(((int64_t)side * 3 + f) * ((int64_t)n_e * n_cz) + node) * n_points + pt] = make_double2(P[f], P[3 + f]);
        return;
    }
    store_node(P, node, (int64_t)n_e * n_cz, side, out, pepmu);
    CSTAMP(6);
}

#ifdef PISA_CHAIN_STAMPS
extern "C" __attribute__((visibility("default"))) int pisa_hip_debug_chain_stamps(unsigned long long *h_out) {
    return check_hip(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_chain_stamps), sizeof(g_chain_stamps)), "stamps");
}
#endif

static int make_consts(const pisa_hip_prob3_params *p, Prob3Consts &c) {
    if (!p) return PISA_HIP_ERR_INVALID;
    prob3_make_consts(p->dm, p->mix, p->mat_pot, p->mat_decay, p->lri_pot, p->decay_flag, c);
    return PISA_HIP_OK;
}

}  // namespace pisa

using namespace pisa;

// ------------------------------------------------------------ grid plan (host)
struct LaunchLists { int32_t *d_slots, *d_lanes; int n_slots; };   // the packed chain launch for one energy count

struct pisa_hip_grid_plan {
    int n_cz, n_layers, n_unique, n_pairs, n_items, n_chain;
    int32_t *d_item_u;     // [n_items] distinct-density index of the item
    int32_t *d_item_p0;    // [n_items] first pair of the item
    int32_t *d_item_cnt;   // [n_items] pairs of the item (consecutive, same density)
    double *d_pair_dist;   // [n_pairs] (cache-resolved) layer length of each pair
    int32_t *d_row_start;  // [n_cz] first chain entry of the row
    int32_t *d_row_cnt;    // [n_cz] crossed layers of the row
    int32_t *d_row_pairs;  // [n_chain] pair index per crossed layer, in path order
    double *d_rho;         // [n_unique]
    double *d_amp;         // stage-AB amplitudes [2][n_pairs][18][n_e]
    int n_e_alloc;
    int32_t *d_pair_u;     // [n_pairs] distinct-density index of each pair
    int chain_packed;      // 1 (default): packed chain launch; 0 (n_cz > 0xffff; development library, PISA_HIP_CHAIN_MODE=split):
                           // one row per workgroup of CHAIN_GROUPS_DEFAULT waves
    // the packed launch (prob3_plan.hpp): a list per energy count the plan has been used with, and the one of
    // `launch_n_e` (pointers into `launches`)
    std::map<int, LaunchLists> *launches;
    Prob3LayerPlan *layers;
    Prob3PackOpts pack;
    int32_t *d_slots;      // [n_slots][4 waves][4]
    int32_t *d_lanes;      // [n_groups][64][2] rows and chain starts of the lanes of a ragged tile
    int n_slots, launch_n_e;
    int32_t *d_chain_u;    // [n_chain] the same per chain entry (position in d_row_pairs)
    double *d_chain_dist;  // [n_chain] layer length per chain entry
    double *d_terms;       // stage-A records [points][2][n_unique][PROB3_NF][n_e] (AMP mode)
    int n_e_terms;
    int n_pt_terms;        // parameter points d_terms has room for
    // several parameter points in one launch (pisa_hip_prob3_grid_planned_multi)
    Prob3Consts *d_consts;   // [PISA_HIP_MAX_POINTS] the points' constants in device memory
    Prob3Consts *h_consts;   // [MULTI_RING][PISA_HIP_MAX_POINTS] pinned, device-mapped staging blocks
    int consts_slot;
    int fused_amp;         // 1 (default): stage A + chain kernel forming the layer matrices itself;
                           // 0 (development library, PISA_HIP_PROB3_FUSED_AMP=0 when the plan is created): stage AB
                           // stores the layer matrices, the chain kernel reads them
    // host copies for re-cutting the items when n_e changes
    int32_t *h_pair_u;
    int items_for_n_e;
    // production-height average (pisa_hip_grid_plan_set_avg_range): the range of the first layer's length per row
    double *d_avg_range;   // [n_cz] km, or null: the plain launch
    int avg_positive;      // some row has a range > 0
};

static void free_launches(pisa_hip_grid_plan *p) {
    if (!p->launches) return;
    for (auto &kv : *p->launches) {
        (void)hipFree(kv.second.d_slots);
        (void)hipFree(kv.second.d_lanes);
    }
    p->launches->clear();
    p->d_slots = p->d_lanes = nullptr;
    p->n_slots = p->launch_n_e = 0;
}

PISA_API int pisa_hip_grid_plan_destroy(pisa_hip_grid_plan *p) {
    if (!p) return PISA_HIP_OK;
    void *ptrs[] = {p->d_item_u, p->d_item_p0, p->d_item_cnt, p->d_pair_dist, p->d_row_start,
                    p->d_row_cnt, p->d_row_pairs, p->d_rho, p->d_amp, p->d_pair_u, p->d_terms,
                    p->d_chain_u, p->d_chain_dist, p->d_avg_range};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    if (p->d_consts) (void)hipFree(p->d_consts);
    if (p->h_consts) (void)hipHostFree(p->h_consts);
    delete[] p->h_pair_u;
    free_launches(p);
    delete p->launches;
    delete p->layers;
    delete p;
    return PISA_HIP_OK;
}

// Cut the (density-sorted) pairs into items of <= ch consecutive pairs of one density.
// ch is chosen so that stage AB has about 2000 waves: enough to occupy the chip
// with the ~8 us terms chain running once per wave.
static int cut_items(pisa_hip_grid_plan *p, int n_e) {
    const int tiles = (n_e + 63) / 64;
    int ch = (int)(((int64_t)p->n_pairs * 2 * tiles + 2047) / 2048);
    if (ch < 1) ch = 1;
    const int np = p->n_pairs;
    int32_t *iu = new int32_t[np + 1], *ip0 = new int32_t[np + 1], *icnt = new int32_t[np + 1];
    int ni = 0;
    for (int k = 0; k < np;) {
        int e = k;
        while (e < np && e - k < ch && p->h_pair_u[e] == p->h_pair_u[k]) e++;
        iu[ni] = p->h_pair_u[k]; ip0[ni] = k; icnt[ni] = e - k;
        ni++;
        k = e;
    }
    int rc = 0;
    for (void *q : {(void *)p->d_item_u, (void *)p->d_item_p0, (void *)p->d_item_cnt})
        if (q) (void)hipFree(q);
    p->d_item_u = p->d_item_p0 = p->d_item_cnt = nullptr;
    size_t bytes = (size_t)(ni > 0 ? ni : 1) * 4;
    rc = check_hip(hipMalloc(&p->d_item_u, bytes), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&p->d_item_p0, bytes), "hipMalloc");
    if (!rc) rc = check_hip(hipMalloc(&p->d_item_cnt, bytes), "hipMalloc");
    if (!rc && ni > 0) rc = check_hip(hipMemcpy(p->d_item_u, iu, (size_t)ni * 4, hipMemcpyHostToDevice), "h2d");
    if (!rc && ni > 0) rc = check_hip(hipMemcpy(p->d_item_p0, ip0, (size_t)ni * 4, hipMemcpyHostToDevice), "h2d");
    if (!rc && ni > 0) rc = check_hip(hipMemcpy(p->d_item_cnt, icnt, (size_t)ni * 4, hipMemcpyHostToDevice), "h2d");
    delete[] iu; delete[] ip0; delete[] icnt;
    p->n_items = ni;
    p->items_for_n_e = n_e;
    return rc;
}

// The slots of the packed chain launch for n_e energies, on the device.  A list is made the first time a plan sees an
// energy count (two allocations and two blocking copies, before anything of the evaluation is queued -- like d_terms,
// not under stream capture) and kept: a plan used with several energy counts in turn makes each list once.
static int make_launch(pisa_hip_grid_plan *p, int n_e) {
    auto it = p->launches->find(n_e);
    if (it == p->launches->end()) {
        Prob3LaunchPlan l;
        if (!prob3_launch_plan(*p->layers, n_e, p->pack, l)) return PISA_HIP_ERR_INVALID;
        if (p->launches->size() >= 64) free_launches(p);   // (a caller sweeping energy counts: start over)
        LaunchLists d = {nullptr, nullptr, l.n_slots};
        int rc = check_hip(hipMalloc(&d.d_slots, std::max<size_t>(l.slots.size(), 1) * 4), "hipMalloc");
        if (!rc) rc = check_hip(hipMalloc(&d.d_lanes, std::max<size_t>(l.lanes.size(), 2) * 4), "hipMalloc");
        if (!rc && !l.slots.empty()) rc = check_hip(hipMemcpy(d.d_slots, l.slots.data(), l.slots.size() * 4, hipMemcpyHostToDevice), "h2d");
        if (!rc && !l.lanes.empty()) rc = check_hip(hipMemcpy(d.d_lanes, l.lanes.data(), l.lanes.size() * 4, hipMemcpyHostToDevice), "h2d");
        if (rc) {
            if (d.d_slots) (void)hipFree(d.d_slots);
            if (d.d_lanes) (void)hipFree(d.d_lanes);
            return rc;
        }
        it = p->launches->emplace(n_e, d).first;
    }
    p->d_slots = it->second.d_slots;
    p->d_lanes = it->second.d_lanes;
    p->n_slots = it->second.n_slots;
    p->launch_n_e = n_e;
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_grid_plan_create(const double *d_densities, const double *d_distances,
                                       int32_t n_cz, int32_t n_layers,
                                       pisa_hip_grid_plan **out) {
    if (!out || n_cz < 1 || n_layers < 1 || !d_densities || !d_distances) return PISA_HIP_ERR_INVALID;
    if (n_layers > PISA_HIP_MAX_LAYERS) return PISA_HIP_ERR_LAYERS;
    const size_t n = (size_t)n_cz * n_layers;
    std::vector<double> rho(n), dist(n);
    int rc = check_hip(hipMemcpy(rho.data(), d_densities, n * 8, hipMemcpyDeviceToHost), "d2h");
    if (!rc) rc = check_hip(hipMemcpy(dist.data(), d_distances, n * 8, hipMemcpyDeviceToHost), "d2h");
    pisa_hip_grid_plan *p = nullptr;
    if (!rc) {
        p = new pisa_hip_grid_plan();
        memset(p, 0, sizeof(*p));
        p->layers = new Prob3LayerPlan();
        p->launches = new std::map<int, LaunchLists>();
        Prob3LayerPlan &lp = *p->layers;
        prob3_layer_plan(rho.data(), dist.data(), n_cz, n_layers, lp);
        const int np = lp.n_pairs, nc = lp.n_chain;
        p->n_cz = n_cz; p->n_layers = n_layers;
        p->n_unique = lp.n_unique;
        p->n_pairs = np;
        p->n_chain = nc;
        p->h_pair_u = new int32_t[np + 1];
        std::copy(lp.pair_u.begin(), lp.pair_u.end(), p->h_pair_u);
        p->fused_amp = PISA_DEV_INT("PROB3_FUSED_AMP", 1) != 0;
        {
            // packed chain launch (prob3_plan.hpp); the development library can take every part of it back
            const char *m = PISA_DEV_STR("CHAIN_MODE");
            p->chain_packed = (m && strcmp(m, "split") == 0) || n_cz > PROB3_MAX_PACKED_ROWS ? 0 : 1;
            p->pack = Prob3PackOpts();
            p->pack.t4 = PISA_DEV_INT("PACK_T4", p->pack.t4);
            p->pack.t2 = PISA_DEV_INT("PACK_T2", p->pack.t2);
            p->pack.ragged = PISA_DEV_INT("PACK_RAGGED", p->pack.ragged);
            p->pack.sorted = PISA_DEV_INT("PACK_SORTED", p->pack.sorted);
        }
        const size_t npa = np > 0 ? np : 1, nca = nc > 0 ? nc : 1;
        auto upload = [&](auto **dst, const auto &v, size_t n_alloc) {
            using T = typename std::remove_reference<decltype(v)>::type::value_type;
            if (!rc) rc = check_hip(hipMalloc(dst, n_alloc * sizeof(T)), "hipMalloc");
            if (!rc && !v.empty()) rc = check_hip(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice), "h2d");
        };
        upload(&p->d_pair_dist, lp.pair_dist, npa);
        upload(&p->d_pair_u, lp.pair_u, npa);
        upload(&p->d_row_start, lp.row_start, (size_t)n_cz);
        upload(&p->d_row_cnt, lp.row_cnt, (size_t)n_cz);
        upload(&p->d_row_pairs, lp.row_pairs, nca);
        upload(&p->d_chain_u, lp.chain_u, nca);
        upload(&p->d_chain_dist, lp.chain_dist, nca);
        upload(&p->d_rho, lp.rho, (size_t)lp.n_unique);
    }
    if (rc && p) { pisa_hip_grid_plan_destroy(p); p = nullptr; }
    *out = p;
    return rc;
}

// the two launches of the fused-amplitude form for `n_points` parameter points whose constants `cs`
// provides (by value: one point; by pointer: the plan's device array)
// CC: CS itself, or WithAvgRange<CS> for the chain kernel of a plan with a range
template <class CS, class CC>
static int launch_planned_as(const CS &cs, const CC &cc, bool decay, int n_points, pisa_hip_grid_plan *plan, const double *d_energy,
                             int32_t n_e, int32_t e_major, double *d_prob_nu, double *d_prob_nubar, double *d_pepmu,
                             hipStream_t s) {
    const unsigned tiles = (unsigned)((n_e + 63) / 64);
    if (plan->chain_packed && plan->launch_n_e != n_e) {
        int rc = make_launch(plan, n_e);
        if (rc) return rc;
    }
    if (plan->n_e_terms < n_e || plan->n_pt_terms < n_points) {
        if (plan->d_terms) (void)hipFree(plan->d_terms);
        plan->d_terms = nullptr;
        plan->n_e_terms = plan->n_pt_terms = 0;
        size_t bytes = (size_t)n_points * 2 * plan->n_unique * PROB3_NF * ((size_t)tiles * 64) * sizeof(double);
        PISA_TRY_HIP(hipMalloc(&plan->d_terms, bytes));
        plan->n_e_terms = n_e;
        plan->n_pt_terms = n_points;
    }
    dim3 tblock(64), tgrid((unsigned)plan->n_unique, 2u * n_points, tiles);
    if (decay)
        hipLaunchKernelGGL((prob3_terms_kernel<true, CS>), tgrid, tblock, 0, s, cs, d_energy, (int)n_e,
                           plan->d_rho, plan->n_unique, plan->d_terms);
    else
        hipLaunchKernelGGL((prob3_terms_kernel<false, CS>), tgrid, tblock, 0, s, cs, d_energy, (int)n_e,
                           plan->d_rho, plan->n_unique, plan->d_terms);
    PISA_CHECK_LAUNCH("prob3_terms_kernel");
    dim3 cblock(64 * CHAIN_GROUPS_DEFAULT), cgrid((unsigned)plan->n_cz, 2u * n_points, tiles);
#define CHAIN(G, A) hipLaunchKernelGGL((prob3_chain_kernel<G, A, CC>), cgrid, cblock, 0, s, cc, (int)n_e, plan->d_row_start, \
                       plan->d_row_cnt, plan->d_row_pairs, plan->n_cz, plan->n_pairs, plan->d_terms,              \
                       (int)e_major, d_prob_nu, d_prob_nubar, (double2 *)d_pepmu, d_energy, plan->d_chain_u,      \
                       plan->d_chain_dist, plan->n_unique, plan->d_slots, (const int2 *)plan->d_lanes, plan->n_slots, \
                       n_points, (int)tiles)
    if (plan->chain_packed) {
        // (point, sign) fastest, then the slots in the plan's order (y, and z beyond the grid's y limit)
        const unsigned sy = (unsigned)std::min(plan->n_slots, 32768);
        cblock = dim3(256);
        cgrid = dim3(2u * n_points, sy, (unsigned)((plan->n_slots + sy - 1) / (sy > 0 ? sy : 1)));
        if (plan->n_slots == 0) return PISA_HIP_OK;   // (no row: cannot happen, n_cz >= 1)
        if constexpr (CC::AVG) CHAIN(0, 1);
        else if (decay) CHAIN(0, 2); else CHAIN(0, 1);
    } else if constexpr (CC::AVG) CHAIN(CHAIN_GROUPS_DEFAULT, 1);
    else if (decay) CHAIN(CHAIN_GROUPS_DEFAULT, 2);
    else CHAIN(CHAIN_GROUPS_DEFAULT, 1);
#undef CHAIN
    PISA_CHECK_LAUNCH("prob3_chain_kernel");
    return PISA_HIP_OK;
}

// a positive range needs a first layer that is diagonal in the mass basis: no decay, no long-range potential
static bool avg_refused(const pisa_hip_grid_plan *plan, const pisa_hip_prob3_params *p) {
    if (!plan->avg_positive) return false;
    if (p->decay_flag == 1) return true;
    for (int i = 0; i < 9; i++)
        if (p->lri_pot[i] != 0.0) return true;
    return false;
}

// A plan with a range launches the averaging form of the chain kernel (no decay: with decay only an all-zero range
// gets here, and the plain launch is its definition); a plan without one launches exactly the plain kernels.
template <class CS>
static int launch_planned(const CS &cs, bool decay, int n_points, pisa_hip_grid_plan *plan, const double *d_energy,
                          int32_t n_e, int32_t e_major, double *d_prob_nu, double *d_prob_nubar, double *d_pepmu,
                          hipStream_t s) {
    if (plan->d_avg_range && !decay) {
        WithAvgRange<CS> cc{cs, plan->d_avg_range};
        return launch_planned_as(cs, cc, decay, n_points, plan, d_energy, n_e, e_major, d_prob_nu, d_prob_nubar, d_pepmu, s);
    }
    return launch_planned_as(cs, cs, decay, n_points, plan, d_energy, n_e, e_major, d_prob_nu, d_prob_nubar, d_pepmu, s);
}

// The range of the first layer's length per coszen row, for the production-height average (nusquids.py:83-88, 573-606:
// `prop_height_range`; formula in DESIGN.md §4, "Production-height averaging").  NULL clears it.
PISA_API int pisa_hip_grid_plan_set_avg_range(pisa_hip_grid_plan *plan, const double *h_avg_range) {
    if (!plan) return PISA_HIP_ERR_INVALID;
    if (!h_avg_range) {
        // (a launch that reads the array may still be queued)
        if (plan->d_avg_range) {
            PISA_TRY_HIP(hipDeviceSynchronize());
            (void)hipFree(plan->d_avg_range);
        }
        plan->d_avg_range = nullptr;
        plan->avg_positive = 0;
        return PISA_HIP_OK;
    }
    const Prob3LayerPlan &lp = *plan->layers;
    int positive = 0;
    for (int j = 0; j < plan->n_cz; j++) {
        const double r = h_avg_range[j];
        if (!(r >= 0.0) || !std::isfinite(r)) return PISA_HIP_ERR_INVALID;
        if (r == 0.0) continue;
        // the first traversed layer must be free of electrons (the atmosphere)
        if (lp.row_cnt[j] < 1 || lp.rho[lp.chain_u[lp.row_start[j]]] != 0.0) return PISA_HIP_ERR_INVALID;
        positive = 1;
    }
    if (!plan->fused_amp) return PISA_HIP_ERR_INVALID;   // the stored-amplitude option has no averaging form
    if (!plan->d_avg_range) PISA_TRY_HIP(hipMalloc(&plan->d_avg_range, (size_t)plan->n_cz * sizeof(double)));
    else PISA_TRY_HIP(hipDeviceSynchronize());
    PISA_TRY_HIP(hipMemcpy(plan->d_avg_range, h_avg_range, (size_t)plan->n_cz * sizeof(double), hipMemcpyHostToDevice));
    plan->avg_positive = positive;
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_prob3_grid_planned(const pisa_hip_prob3_params *h_params,
                                         pisa_hip_grid_plan *plan, const double *d_energy,
                                         int32_t n_e, int32_t e_major, double *d_prob_nu,
                                         double *d_prob_nubar, double *d_pepmu, void *stream) {
    if (!plan || n_e < 1 || !d_energy) return PISA_HIP_ERR_INVALID;
    ConstsByValue cv;
    Prob3Consts &c = cv.c;
    int rc = make_consts(h_params, c);
    if (rc) return rc;
    if (avg_refused(plan, h_params)) return PISA_HIP_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    const unsigned tiles = (unsigned)((n_e + 63) / 64);
    const int fused_amp = plan->fused_amp;
    dim3 cblock(64 * CHAIN_GROUPS_DEFAULT), cgrid((unsigned)plan->n_cz, 2, tiles);
    if (fused_amp) return launch_planned(cv, c.decay != 0, 1, plan, d_energy, n_e, e_major, d_prob_nu, d_prob_nubar, d_pepmu, s);
    if (plan->n_e_alloc < n_e) {
        if (plan->d_amp) (void)hipFree(plan->d_amp);
        plan->d_amp = nullptr;
        plan->n_e_alloc = 0;
        size_t amp_bytes = (size_t)2 * (plan->n_pairs > 0 ? plan->n_pairs : 1) * 18 * (((size_t)n_e + 63) / 64 * 64) * sizeof(double);
        PISA_TRY_HIP(hipMalloc(&plan->d_amp, amp_bytes));
        plan->n_e_alloc = n_e;
    }
    if (plan->items_for_n_e != n_e && (rc = cut_items(plan, n_e))) return rc;
    dim3 ablock(64), agrid((unsigned)(plan->n_items > 0 ? plan->n_items : 1), 2, tiles);
    if (plan->n_items > 0) {
        if (c.decay)
            hipLaunchKernelGGL(prob3_terms_amp_kernel<true>, agrid, ablock, 0, s, c, d_energy, (int)n_e,
                               plan->d_rho, plan->d_item_u, plan->d_item_p0, plan->d_item_cnt,
                               plan->d_pair_dist, plan->n_pairs, plan->d_amp);
        else
            hipLaunchKernelGGL(prob3_terms_amp_kernel<false>, agrid, ablock, 0, s, c, d_energy, (int)n_e,
                               plan->d_rho, plan->d_item_u, plan->d_item_p0, plan->d_item_cnt,
                               plan->d_pair_dist, plan->n_pairs, plan->d_amp);
    }
    hipLaunchKernelGGL((prob3_chain_kernel<CHAIN_GROUPS_DEFAULT, 0, ConstsByValue>), cgrid, cblock, 0, s, cv, (int)n_e, plan->d_row_start,
                       plan->d_row_cnt, plan->d_row_pairs, plan->n_cz, plan->n_pairs, plan->d_amp,
                       (int)e_major, d_prob_nu, d_prob_nubar, (double2 *)d_pepmu, d_energy, plan->d_pair_u,
                       plan->d_pair_dist, plan->n_unique, nullptr, nullptr, 0, 1, 0);
    PISA_CHECK_LAUNCH("prob3_chain_kernel");
    return PISA_HIP_OK;
}

// Staging blocks for the constants of a batch: the host fills one (pinned, device-mapped) and a small
// kernel copies it into the device array the batch kernels read.  A ring, so that a caller that queues
// a second batch before the first has started does not overwrite what the first copy has yet to read.
constexpr int MULTI_RING = 8;

PISA_API int pisa_hip_prob3_grid_planned_multi(const pisa_hip_prob3_params *h_params, int32_t n_points,
                                               pisa_hip_grid_plan *plan, const double *d_energy,
                                               int32_t n_e, int32_t e_major, double *d_pepmu_points,
                                               void *stream) {
    if (!plan || n_e < 1 || !d_energy || !h_params || !d_pepmu_points || n_points < 1 ||
        n_points > PISA_HIP_MAX_POINTS)
        return PISA_HIP_ERR_INVALID;
    if (!plan->fused_amp) return PISA_HIP_ERR_INVALID;   // the stored-amplitude option has no batch form
    for (int k = 0; k < n_points; k++)
        if (avg_refused(plan, h_params + k)) return PISA_HIP_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    if (!plan->d_consts) {
        PISA_TRY_HIP(hipMalloc(&plan->d_consts, sizeof(Prob3Consts) * PISA_HIP_MAX_POINTS));
        PISA_TRY_HIP(hipHostMalloc(&plan->h_consts, sizeof(Prob3Consts) * PISA_HIP_MAX_POINTS * MULTI_RING,
                                   hipHostMallocMapped));
        plan->consts_slot = 0;
    }
    Prob3Consts *hc = plan->h_consts + (size_t)plan->consts_slot * PISA_HIP_MAX_POINTS;
    plan->consts_slot = (plan->consts_slot + 1) % MULTI_RING;
    bool decay = false;
    for (int k = 0; k < n_points; k++) {
        int rc = make_consts(h_params + k, hc[k]);
        if (rc) return rc;
        if (k == 0) decay = hc[k].decay != 0;
        else if ((hc[k].decay != 0) != decay) return PISA_HIP_ERR_INVALID;   // one kernel variant per batch
    }
    static_assert(sizeof(Prob3Consts) % 8 == 0, "copied in 8-byte words");
    const int n_words = (int)(sizeof(Prob3Consts) / 8) * n_points;
    hipLaunchKernelGGL(prob3_stage_consts_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long *>(hc),
                       reinterpret_cast<unsigned long long *>(plan->d_consts), n_words);
    PISA_CHECK_LAUNCH("prob3_stage_consts_kernel");
    ConstsByPointer cp{plan->d_consts};
    if (n_points == 1) {
        // a batch of one writes the ordinary [sign][flavour][node] tables
        return launch_planned(cp, decay, 1, plan, d_energy, n_e, e_major, nullptr, nullptr, d_pepmu_points, s);
    }
    return launch_planned(cp, decay, (int)n_points, plan, d_energy, n_e, e_major, nullptr, nullptr,
                          d_pepmu_points, s);
}
