// hist.hip -- HBM-bound half of the hot path for gfx950:
//   event_indices           digitise coordinates once (they never change
//                           between evaluations): flat bin / grid-node index
//   lookup_regular          grid -> event gather          (translation.py:417-501)
//   histogram_regular       weighted N-D histogram        (translation.py:90-205)
//   reweight_hist           fused prob3.apply + aeff.apply + hist.apply(sumw2), every event form
//   reweight_hist_multi     the same for several parameter points in one sweep of the events
//   the element-wise stages (apply_osc_weights, weight_chain_multi, apply_aeff)
// The exact accumulator, the argument block, the deposit target, flush_window / flush_rotation and the weight chains
// weight_compact / weight_reference are hist_device.hpp's, shared with the planned sweep that the headline evaluation
// runs (hist_planned.hip); the limbs become fp64 maps in hist_tail.hip.  run_hist takes the instantiation of
// hist_accumulate_kernel from the table hist_forms.
//
// Roofline: HBM.  Per event the indexed fused kernel reads
//   node i32 + bin i32 + nu_flux 2xf64 + weighted_aeff f64 + initial_weights f64
//   = 40 B      (coordinates digitised once at setup, like the reference's own
//                pre-digitised irregular dimensions, utils/hist.py:100-113),
//   24 B in the compact form (static factors folded into the flux pair once),
//   20 B with the two indices in 16 bits each (MODE 7, the default where it applies),
// and the coordinate form reads 8 B x (2 lookup coords + D sample coords) more
// = 72 B (D=3).  The (P_e, P_mu) gather tables (<= 3.8 MB) stay in L2.
#include <stdlib.h>
#include <atomic>
#include <string.h>

#include "hist_host.hpp"

namespace pisa {

#ifdef PISA_HIST_STAMPS
static __device__ unsigned long long g_hist_stamps[8 * 1024];
#endif

// ---------------------------------------------------------------------------
// (Non-temporal streaming loads were measured A/B in one session: this kernel got 5 us SLOWER,
// 92.3 vs 87.4 us, and the whole evaluation did not change; plain loads are used.)

__device__ __forceinline__ bool bin_index(const DevBinning &b, double x, double y, double z,
                                          int64_t &flat) {
    // half-open [min, max) per dimension, bin = (int)((x - min) * norm)
    // (fast_histogram rule; translation.py:417-456 for lookups)
    if (!(x >= b.mins[0] && x < b.maxs[0])) return false;
    int ix = (int)((x - b.mins[0]) * b.norm[0]);
    ix = ix < b.nb[0] ? ix : b.nb[0] - 1;
    flat = ix;
    if (b.ndim > 1) {
        if (!(y >= b.mins[1] && y < b.maxs[1])) return false;
        int iy = (int)((y - b.mins[1]) * b.norm[1]);
        iy = iy < b.nb[1] ? iy : b.nb[1] - 1;
        flat = flat * b.nb[1] + iy;
    }
    if (b.ndim > 2) {
        if (!(z >= b.mins[2] && z < b.maxs[2])) return false;
        int iz = (int)((z - b.mins[2]) * b.norm[2]);
        iz = iz < b.nb[2] ? iz : b.nb[2] - 1;
        flat = flat * b.nb[2] + iz;
    }
    return true;
}

// bin_index without early exits and with the number of dimensions known at compile time: `flat` is
// always a valid index (0 for a point outside), the return value says whether the point is inside --
// same comparisons, same arithmetic (the flat index fits 32 bits: checked by the launcher)
template <int ND>
__device__ __forceinline__ bool bin_index_flat(const DevBinning &b, double x, double y, double z,
                                               int &flat) {
    bool ok = x >= b.mins[0] && x < b.maxs[0];
    int ix = (int)((x - b.mins[0]) * b.norm[0]);
    ix = ix < b.nb[0] ? ix : b.nb[0] - 1;
    int f = ix;
    if (ND > 1) {
        ok = ok && (y >= b.mins[1] && y < b.maxs[1]);
        int iy = (int)((y - b.mins[1]) * b.norm[1]);
        iy = iy < b.nb[1] ? iy : b.nb[1] - 1;
        f = f * b.nb[1] + iy;
    }
    if (ND > 2) {
        ok = ok && (z >= b.mins[2] && z < b.maxs[2]);
        int iz = (int)((z - b.mins[2]) * b.norm[2]);
        iz = iz < b.nb[2] ? iz : b.nb[2] - 1;
        f = f * b.nb[2] + iz;
    }
    flat = ok ? f : 0;
    return ok;
}

__global__ void __launch_bounds__(256)
event_indices_kernel(const DevBinning b, const double *__restrict__ x,
                     const double *__restrict__ y, const double *__restrict__ z, int64_t n,
                     int32_t *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t flat;
    bool in = bin_index(b, x[i], b.ndim > 1 ? y[i] : 0.0, b.ndim > 2 ? z[i] : 0.0, flat);
    out[i] = in ? (int32_t)flat : -1;
}

// The lowest bin that events [start, end) of a container deposit into -- where the LDS window of a binning too large
// for LDS is put; 0 if none deposits.  QUAD: from the index words of the 16-bit form (four events each; q_end: one
// past the last word of the chunk), else from the packed (node, bin) pairs.  Called by every thread of the workgroup.
template <bool QUAD>
__device__ __forceinline__ int window_lowest_bin(const ContDev &C, int64_t start, int64_t end, int64_t q_end, int nthreads) {
    __shared__ int s_lo;
    if (threadIdx.x == 0) s_lo = 0x7fffffff;
    __syncthreads();
    int m = 0x7fffffff;
    if (QUAD) {
        const uint4 *idxq = reinterpret_cast<const uint4 *>(C.idx16);
        for (int64_t i = (start >> 2) + threadIdx.x; i < q_end; i += nthreads) {
            const uint4 v = idxq[i];
            const int b[4] = {(int)(v.x >> 16), (int)(v.y >> 16), (int)(v.z >> 16), (int)(v.w >> 16)};
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (b[k] != 0xffff && b[k] < m) m = b[k];
        }
    } else {
        const int4 *idx4 = reinterpret_cast<const int4 *>(C.node_bin);
        for (int64_t i = (start >> 1) + threadIdx.x; i < (end >> 1); i += nthreads) {
            const int4 v = idx4[i];
            if (v.y >= 0 && v.y < m) m = v.y;
            if (v.w >= 0 && v.w < m) m = v.w;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int other = __shfl_xor(m, d);
        m = other < m ? other : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0x7fffffff) atomicMin(&s_lo, m);
    __syncthreads();
    return s_lo == 0x7fffffff ? 0 : s_lo;
}

// MODE 0: generic histogram (weights or counts; quantities (w, 1))
// MODE 1: fused reweight chain from coordinates (quantities (w, w^2))
// MODE 2: fused reweight chain from pre-digitised indices, 2 events / thread / sweep
// MODE 3: same from the packed 16-byte columns (node,bin) / (aeff,w0) / flux: 40 B per event
// MODE 5: compact form, (node,bin) + the flux pair pre-multiplied by the static per-event
//         factor initial_weights*weighted_aeff: 24 B per event, two loads fewer per pair.
//         w = ((g_e*P_e) + (g_mu*P_mu)) * scale  -- the reference's product with the static
//         factors associated first; differs from MODE 3 by rounding only (<= 3 ulp per weight)
// MODE 7: MODE 5 with the two indices in 16 bits each (grids and binnings below 65535 entries):
//         20 B per event, four events per thread and sweep so that every load stays 16 bytes
// DIMS (MODE 0, 1) = 4 * (dimensions of the calc grid, MODE 1) + (dimensions of the output binning)
template <int MODE, bool LDS_ACC, int DIMS = 0>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
hist_accumulate_kernel(const HistArgs a, unsigned long long *__restrict__ g_limbs,
                       int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_acc[];  // [slab][quantity][bin], integer units
    STAMP(0);
    const int nthreads = blockDim.x;
    int c = 0;
    const int bid = blockIdx.x;
    while (c + 1 < a.n_cont && bid >= a.blk_start[c + 1]) c++;  // workgroup-uniform
    const ContDev &C = a.cont[c];
    const int64_t lb = bid - a.blk_start[c];
    // events of this workgroup where the workgroups of a container do not sweep together: the container's own
    // share (partitioned window order: multiples of 256 events), else the launch's largest share
    const int64_t my_chunk = a.cont_chunk[c] > 0 ? (int64_t)a.cont_chunk[c] * 256 : a.chunk;
    const int64_t start = lb * my_chunk;
    int64_t end = start + my_chunk;
    if (end > C.n) end = C.n;
    // bins held in LDS: all of them, or (a.window > 0, MODE 3 only) the window
    // [bin_lo, bin_lo + window) that starts at the smallest bin of this workgroup's
    // chunk -- a binning too large for LDS still gets LDS accumulation when the
    // events are stored in an order that keeps a chunk inside a few hundred
    // neighbouring bins; deposits outside the window go to the global limbs directly
    const int n_bins = a.window > 0 ? a.window : (int)a.n_bins;
    const int n_acc = NL * 2 * n_bins;
    // replica used by this lane: neighbouring lanes (neighbouring, i.e. correlated,
    // events) add into different copies, which cuts same-address serialisation
    unsigned long long *my_acc = s_acc + (LDS_ACC ? (int)(threadIdx.x & (a.copies - 1)) * n_acc : 0);
    int32_t *s_part = reinterpret_cast<int32_t *>(s_acc + 2 * (size_t)n_acc);   // partitioned order only (host: LDS size)
    unsigned long long *g_out = g_limbs + (int64_t)(a.cont_base + c) * a.n_bins * 2 * NL;
    int bin_lo = 0;

    // MODE 3 sweep order: the workgroups of a container advance through its columns
    // TOGETHER (workgroup j takes pairs j*T + t, stepping by n_wg*T), so that at any
    // moment the chip reads a few contiguous windows of HBM; the LDS window of a large
    // binning needs bin-contiguous chunks and keeps them.  The loads of the first sweep
    // are issued here, before the LDS accumulators are cleared, so that the clearing
    // overlaps the first HBM round trip.
    const bool together = a.window == 0;
    const int64_t n_wg = a.blk_start[c + 1] - a.blk_start[c];
    const int64_t step = together ? n_wg * nthreads : nthreads;
    const int64_t p_end = together ? (C.n >> 1) : (end >> 1);
    int64_t p = (together ? lb * nthreads : (start >> 1)) + threadIdx.x;
    constexpr bool QUAD = MODE == 7;
    bool have = !QUAD && p < p_end;
    int4 ix = make_int4(-1, -1, -1, -1);  // node0, bin0, node1, bin1
    double2 awa = make_double2(0.0, 0.0), awb = awa, fa = awa, fb = awa;
    constexpr bool PACKED = MODE == 3 || MODE == 5;
    constexpr bool COMPACT = MODE == 5;
    // MODE 7: quads of events (columns padded to whole blocks of 64 quads)
    const int64_t q_end = ((together ? C.n : end) + 3) >> 2;
    int64_t q = (together ? lb * nthreads : (start >> 2)) + threadIdx.x;
    bool qhave = QUAD && q < q_end;
    uint4 qx = make_uint4(~0u, ~0u, ~0u, ~0u);
    double2 g0 = awa, g1 = awa;
    if (QUAD && qhave) {
        qx = reinterpret_cast<const uint4 *>(C.idx16)[q];
        const double2 *gq = C.wflux_q + ((q >> 6) * 256 + (q & 63));
        g0 = gq[0]; g1 = gq[64];
    }
    if (PACKED && have) {
        const double2 *col = COMPACT ? C.wflux : C.aeff_w0;
        ix = reinterpret_cast<const int4 *>(C.node_bin)[p];
        awa = col[2 * p]; awb = col[2 * p + 1];
        if (!COMPACT) {
            fa = reinterpret_cast<const double2 *>(C.flux)[2 * p];
            fb = reinterpret_cast<const double2 *>(C.flux)[2 * p + 1];
        }
    }

    STAMP(1);
    if (LDS_ACC) {
        // (partitioned order: two windows -- a chunk may reach into a second partition -- and the partition
        // table in LDS: looking a partition up in global memory is a chain of dependent scalar loads, ~1 us each)
        const bool parts = QUAD && a.window > 0 && C.part_start;
        if (parts)   // behind the two windows (a strided fill: the table has up to PART_MAX + 1 entries whatever the block size)
            for (int k = threadIdx.x; k <= C.n_part; k += nthreads) s_part[k] = C.part_start[k];
        for (int k = threadIdx.x; k < n_acc * (parts ? 2 : a.copies); k += nthreads) s_acc[k] = 0ull;
        if ((PACKED || QUAD) && a.window > 0 && !(QUAD && C.part_start)) {
            bin_lo = window_lowest_bin<QUAD>(C, start, end, q_end, nthreads);
        }
        __syncthreads();
    }
    bool bad = false;
    STAMP(2);

    const DepositTarget<LDS_ACC, false> accumulate{my_acc, n_bins, bin_lo, g_out, a.opts, bad};
    auto flush_win = [&](const unsigned long long *win, int lo, int ncopies) {
        flush_window(win, ncopies, n_bins, n_acc, flush_rotation(lb, n_acc), nthreads, [&](int g, int bin, unsigned long long v) {
            if (lo + bin < (int)a.n_bins) atomicAdd(&g_out[(int64_t)lo * 2 * NL + g], v);   // (a window may reach beyond the last bin)
        });
    };
    // partitioned order: the other LDS window (see the QUAD sweep) and the first bin of what it holds
    int other_lo = -1;

    if (QUAD) {
        const double2 *tab = C.pepmu_own ? C.pepmu_own
                                         : a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes;
        const double scale = C.scale;
        const uint4 *idxq = reinterpret_cast<const uint4 *>(C.idx16);
        const double2 *aw = C.wflux_q;
        int64_t qstep = together ? n_wg * nthreads : nthreads;
        const double2 zero2 = make_double2(0.0, 0.0);
        int64_t q_stop = q_end;
        // Partitioned resident order (binning beyond the LDS accumulators, ContDev::part_start): the chunk is
        // worked through partition by partition, each with the LDS window on that partition's bins -- every
        // deposit is an LDS deposit, nothing is scanned for the window's position, and only a chunk that
        // straddles a partition boundary flushes twice.  Partition boundaries are multiples of 256 events =
        // one wavefront's sweep.
        // A chunk that straddles a partition boundary keeps BOTH partitions' windows in LDS (2 x 63 KiB of the
        // CU's 160): its wavefronts move from one to the other on their own, no barrier, no intermediate flush
        // (in-kernel stamps: flushing, clearing and restarting in between left the straddling workgroups ~10 us
        // behind the others); a third partition in one chunk recycles the older window behind a barrier.
        int part = -1, phase = 0;
        if (LDS_ACC && a.window > 0 && C.part_start) {
            // the caller's table is taken on trust by the sweep below (an entry that decreases, or a last entry short of
            // the container, would end the loop early and DROP events without a trace): checked here, status bit 2
            if (threadIdx.x == 0 && lb == 0 && status) {
                bool ok = s_part[0] == 0 && (int64_t)s_part[C.n_part] * 256 >= C.n;
                for (int k = 0; k < C.n_part; k++) ok = ok && s_part[k] <= s_part[k + 1];
                if (!ok) atomicOr(status, 2);
            }
            part = 0;
            while (part + 1 < C.n_part && (int64_t)s_part[part + 1] * 256 <= start) part++;
        }
      for (;;) {
        if (part >= 0) {
            const int64_t ps = (int64_t)s_part[part] * 256, pe = (int64_t)s_part[part + 1] * 256;
            const int64_t lo = ps > start ? ps : start, hi = pe < end ? pe : end;
            if (phase >= 1) {
                unsigned long long *win = s_acc + (phase & 1) * n_acc;
                if (phase >= 2) {     // (workgroup-uniform: the chunk's geometry)
                    __syncthreads();
                    flush_win(win, other_lo, 1);
                    __syncthreads();
                    for (int k = threadIdx.x; k < n_acc; k += nthreads) win[k] = 0ull;
                    __syncthreads();
                }
                other_lo = bin_lo;
                my_acc = win;
            }
            bin_lo = part * a.window;
            q_stop = (hi + 3) >> 2;
            if (lo > start) {     // a later partition of this chunk: its own first loads
                q = (lo >> 2) + threadIdx.x;
                qhave = q < q_stop;
                if (qhave) {
                    qx = idxq[q];
                    const double2 *gq0 = aw + ((q >> 6) * 256 + (q & 63));
                    g0 = gq0[0]; g1 = gq0[64];
                }
            } else {
                qhave = q < q_stop;
            }
        }
        const int64_t q_lim = q_stop;   // (this partition's end)
        // The pair loop's software pipeline (see below), two half-sweeps per quad: while
        // events 0,1 of the quad are consumed the flux of events 2,3 is in flight, while 2,3
        // are consumed the next quad's indices and the flux of its events 0,1.
        while (qhave) {
            const double2 *gq = aw + ((q >> 6) * 256 + (q & 63));  // lane-contiguous 16-B loads
            {
                const unsigned n0 = qx.x & 0xffffu, n1 = qx.y & 0xffffu;
                const unsigned b0 = qx.x >> 16, b1 = qx.y >> 16;
                double2 p0 = tab[n0 == 0xffffu ? 0 : n0];
                double2 p1 = tab[n1 == 0xffffu ? 0 : n1];
                const double2 g2 = gq[128], g3 = gq[192];
                if (n0 == 0xffffu) p0 = zero2;
                if (n1 == 0xffffu) p1 = zero2;
                double w0 = weight_compact(g0.x, g0.y, p0.x, p0.y, scale);
                double w1 = weight_compact(g1.x, g1.y, p1.x, p1.y, scale);
                if (b0 == 0xffffu) w0 = 0.0;
                if (b1 == 0xffffu) w1 = 0.0;
                accumulate(b0 == 0xffffu ? 0 : (int)b0, w0, w0 * w0);
                accumulate(b1 == 0xffffu ? 0 : (int)b1, w1, w1 * w1);
                g0 = g2; g1 = g3;
            }
            const unsigned n2 = qx.z & 0xffffu, n3 = qx.w & 0xffffu;
            const unsigned b2 = qx.z >> 16, b3 = qx.w >> 16;
            double2 p2 = tab[n2 == 0xffffu ? 0 : n2];
            double2 p3 = tab[n3 == 0xffffu ? 0 : n3];
            const int64_t qn = q + qstep;
            const bool have_n = qn < q_lim;
            const int64_t ql = have_n ? qn : q;  // unconditional loads (the last sweep re-reads its own quad)
            const uint4 qxn = idxq[ql];
            const double2 *gn = aw + ((ql >> 6) * 256 + (ql & 63));
            const double2 g0n = gn[0], g1n = gn[64];
            if (n2 == 0xffffu) p2 = zero2;
            if (n3 == 0xffffu) p3 = zero2;
            double w2 = weight_compact(g0.x, g0.y, p2.x, p2.y, scale);
            double w3 = weight_compact(g1.x, g1.y, p3.x, p3.y, scale);
            if (b2 == 0xffffu) w2 = 0.0;
            if (b3 == 0xffffu) w3 = 0.0;
            accumulate(b2 == 0xffffu ? 0 : (int)b2, w2, w2 * w2);
            accumulate(b3 == 0xffffu ? 0 : (int)b3, w3, w3 * w3);
            qx = qxn; g0 = g0n; g1 = g1n;
            q = qn;
            qhave = have_n;
        }
        if (part < 0) break;
        // next partition of this chunk, if any
        const int64_t pe = (int64_t)s_part[part + 1] * 256;
        if (pe >= end || part + 1 >= C.n_part) break;
        part++;
        phase++;
      }
    } else if (PACKED) {
        // packed columns: (node, bin) int2 and (aeff, w0) double2 per event; every load is 16 B
        const double2 *tab = C.pepmu_own ? C.pepmu_own
                                         : a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes;
        const double scale = C.scale;
        const int4 *idx4 = reinterpret_cast<const int4 *>(C.node_bin);
        const double2 *aw = COMPACT ? C.wflux : C.aeff_w0;
        const double2 *flux2 = reinterpret_cast<const double2 *>(C.flux);
        // Software-pipelined: the five streaming loads of the NEXT pair of events are
        // issued before the current pair is consumed, and the two dependent table
        // gathers of the current pair before them, so a wave always has a full
        // iteration of HBM requests in flight (a thread only runs ~6-10 iterations;
        // without this the idx -> gather -> use chain is exposed every time).
        while (have) {
            // node < 0 (outside the calc grid): read entry 0, then force P = 0
            double2 pa = tab[ix.x < 0 ? 0 : ix.x];
            double2 pb = tab[ix.z < 0 ? 0 : ix.z];
            const int64_t pn = p + step;
            const bool have_n = pn < p_end;
            // unconditional (the last sweep re-reads its own pair, never used): a
            // branch here would make the compiler wait for these loads as well
            const int64_t pl = have_n ? pn : p;
            const int4 ixn = idx4[pl];
            const double2 awan = aw[2 * pl], awbn = aw[2 * pl + 1];
            double2 fan = make_double2(0.0, 0.0), fbn = fan;
            if (!COMPACT) {
                fan = flux2[2 * pl];
                fbn = flux2[2 * pl + 1];
            }
            if (ix.x < 0) pa = make_double2(0.0, 0.0);
            if (ix.z < 0) pb = make_double2(0.0, 0.0);
            // branch-free on purpose (an event outside the binning deposits w = 0,
            // i.e. nothing): a conditional here lets the compiler sink the gathers
            // below the prefetch and wait for all of it
            double wa, wb;
            if (COMPACT) {
                wa = weight_compact(awa.x, awa.y, pa.x, pa.y, scale);
                wb = weight_compact(awb.x, awb.y, pb.x, pb.y, scale);
            } else {
                wa = weight_reference(awa.y, fa.x, fa.y, pa.x, pa.y, awa.x, scale);
                wb = weight_reference(awb.y, fb.x, fb.y, pb.x, pb.y, awb.x, scale);
            }
            if (ix.y < 0) wa = 0.0;
            if (ix.w < 0) wb = 0.0;
            accumulate(ix.y < 0 ? bin_lo : ix.y, wa, wa * wa);
            accumulate(ix.w < 0 ? bin_lo : ix.w, wb, wb * wb);
            ix = ixn; awa = awan; awb = awbn; fa = fan; fb = fbn;
            p = pn;
            have = have_n;
        }
        if ((end & 1) && threadIdx.x == 0 && end > start) {  // odd tail of the container
            const int64_t i = end - 1;
            const int2 ix1 = C.node_bin[i];
            if (ix1.y >= 0) {
                double2 pp = ix1.x >= 0 ? tab[ix1.x] : make_double2(0.0, 0.0);
                double2 x = aw[i];
                double w;
                if (COMPACT) {
                    w = weight_compact(x.x, x.y, pp.x, pp.y, scale);
                } else {
                    double2 f = flux2[i];
                    w = weight_reference(x.y, f.x, f.y, pp.x, pp.y, x.x, scale);
                }
                accumulate(ix1.y, w, w * w);
            }
        }
    } else if (MODE == 2) {
        // (P_e, P_mu) of this container's class, one 16-B gather per event
        const double2 *tab = a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes;
        const double scale = C.scale;
        const int64_t p0 = start >> 1, p1 = end >> 1;  // whole pairs (start is even)
        const int2 *node2 = reinterpret_cast<const int2 *>(C.node);
        const int2 *bin2 = reinterpret_cast<const int2 *>(C.bin);
        const double2 *aeff2 = reinterpret_cast<const double2 *>(C.aeff);
        const double2 *w02 = reinterpret_cast<const double2 *>(C.w0);
        const double2 *flux2 = reinterpret_cast<const double2 *>(C.flux);
        for (int64_t i = p0 + threadIdx.x; i < p1; i += nthreads) {
            const int2 nd = node2[i];
            const int2 bn = bin2[i];
            const double2 ae = aeff2[i];
            const double2 w0 = w02[i];
            const double2 f0 = flux2[2 * i], f1 = flux2[2 * i + 1];
            double2 pa = make_double2(0.0, 0.0), pb = make_double2(0.0, 0.0);
            if (nd.x >= 0) pa = tab[nd.x];
            if (nd.y >= 0) pb = tab[nd.y];
            if (bn.x >= 0) {
                const double w = weight_reference(w0.x, f0.x, f0.y, pa.x, pa.y, ae.x, scale);
                accumulate(bn.x, w, w * w);
            }
            if (bn.y >= 0) {
                const double w = weight_reference(w0.y, f1.x, f1.y, pb.x, pb.y, ae.y, scale);
                accumulate(bn.y, w, w * w);
            }
        }
        if ((end & 1) && threadIdx.x == 0 && end > start) {  // odd tail of the container
            const int64_t i = end - 1;
            const int nd = C.node[i], bn = C.bin[i];
            if (bn >= 0) {
                double2 pp = nd >= 0 ? tab[nd] : make_double2(0.0, 0.0);
                double2 f = flux2[i];
                const double w = weight_reference(C.w0[i], f.x, f.y, pp.x, pp.y, C.aeff[i], scale);
                accumulate(bn, w, w * w);
            }
        }
    } else {
        const double *prob = MODE == 1 ? a.prob[C.side] : nullptr;
        const int po_e = 0 * 3 + C.flav;   // P[e  -> flav]
        const int po_mu = 1 * 3 + C.flav;  // P[mu -> flav]
        if (MODE == 1) {
            // SURVEY section 8(d)'s unit of work: 72 B per event in eight column streams, both
            // digitisations in the kernel.  All streaming loads of an event are issued before anything
            // depends on one of them and nothing branches in between (an event outside the calc grid
            // gathers node 0 and multiplies by 0): one HBM round trip + one gather per sweep.  With the
            // lookup's early exits between the loads a sweep was three to four dependent round trips
            // (204 us for 10^7 events).
            constexpr int GD = DIMS >> 2, OD = DIMS & 3;
            constexpr bool g2 = GD > 1;
            const double2 *__restrict__ flux2 = reinterpret_cast<const double2 *>(C.flux);
            const double cscale = C.scale;
            // The gather is what this kernel waits for when it goes to the full matrices: 2.9 MB of
            // 72-byte records that the 720 MB column stream keeps pushing out of the L2 (all gathers
            // forced to one node: 202 -> 139 us for 10^7 events); the compact tables, 320 KB per class
            // and one 16-byte gather per event, are used whenever the caller provides them.
            const double2 *__restrict__ tab =
                a.pepmu ? a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes : nullptr;
            auto event = [&](double gx, double gy, double2 f, double w0, double ae, double x, double y, double z) {
                // grid -> event lookup of prob_e, prob_mu (container.py:981-1012,
                // translation.py:427-438): 0 outside the grid
                int node;
                const bool in = bin_index_flat<GD>(a.grid, gx, gy, 0.0, node);
                double pe, pmu;
                if (tab) {   // compact (P_e, P_mu) table of this container's class: one 16-byte gather
                    const double2 pp = tab[node];
                    pe = pp.x;
                    pmu = pp.y;
                } else {     // two 8-byte gathers from the 72-byte-stride P[node][3][3] table
                    pe = prob[9 * node + po_e];
                    pmu = prob[9 * node + po_mu];
                }
                pe = in ? pe : 0.0;
                pmu = in ? pmu : 0.0;
                double w = w0 * ((f.x * pe) + (f.y * pmu));   // prob3.py:622
                w = w * (ae * cscale);                        // aeff.py:87
                int bin;
                if (bin_index_flat<OD>(a.outb, x, y, z, bin)) accumulate(bin, w, w * w);
            };
            // every column 16-byte aligned (checked per workgroup, uniform): two consecutive events per
            // thread and sweep with 16-byte loads, the workgroups of a container sweeping its columns
            // together like the packed forms
            uintptr_t bits = (uintptr_t)C.gx | (uintptr_t)C.flux | (uintptr_t)C.w0 | (uintptr_t)C.aeff | (uintptr_t)C.s[0];
            if (g2) bits |= (uintptr_t)C.gy;
            if (OD > 1) bits |= (uintptr_t)C.s[1];
            if (OD > 2) bits |= (uintptr_t)C.s[2];
            if ((bits & 15) == 0) {
                const double2 *__restrict__ gx2 = reinterpret_cast<const double2 *>(C.gx);
                const double2 *__restrict__ gy2 = reinterpret_cast<const double2 *>(C.gy);
                const double2 *__restrict__ w02 = reinterpret_cast<const double2 *>(C.w0);
                const double2 *__restrict__ ae2 = reinterpret_cast<const double2 *>(C.aeff);
                const double2 *__restrict__ x2 = reinterpret_cast<const double2 *>(C.s[0]);
                const double2 *__restrict__ y2 = reinterpret_cast<const double2 *>(C.s[1]);
                const double2 *__restrict__ z2 = reinterpret_cast<const double2 *>(C.s[2]);
                const double2 zero = make_double2(0.0, 0.0);
                const int64_t n_wg1 = a.blk_start[c + 1] - a.blk_start[c];
                for (int64_t i = lb * nthreads + threadIdx.x; i < (C.n >> 1); i += n_wg1 * nthreads) {
                    const double2 gx = gx2[i];
                    const double2 gy = g2 ? gy2[i] : zero;
                    const double2 f0 = flux2[2 * i], f1 = flux2[2 * i + 1];
                    const double2 w0 = w02[i], ae = ae2[i];
                    const double2 x = x2[i];
                    const double2 y = OD > 1 ? y2[i] : zero;
                    const double2 z = OD > 2 ? z2[i] : zero;
                    event(gx.x, gy.x, f0, w0.x, ae.x, x.x, y.x, z.x);
                    event(gx.y, gy.y, f1, w0.y, ae.y, x.y, y.y, z.y);
                }
                if ((C.n & 1) && lb == 0 && threadIdx.x == 0) {  // odd tail of the container
                    const int64_t i = C.n - 1;
                    event(C.gx[i], g2 ? C.gy[i] : 0.0, flux2[i], C.w0[i], C.aeff[i], C.s[0][i],
                          OD > 1 ? C.s[1][i] : 0.0, OD > 2 ? C.s[2][i] : 0.0);
                }
            } else {
                for (int64_t i = start + threadIdx.x; i < end; i += nthreads)
                    event(C.gx[i], g2 ? C.gy[i] : 0.0, flux2[i], C.w0[i], C.aeff[i], C.s[0][i],
                          OD > 1 ? C.s[1][i] : 0.0, OD > 2 ? C.s[2][i] : 0.0);
            }
        } else {
            // MODE 0, generic histogram (DIMS = dimensions of the binning): like the coordinate form,
            // pairs of events with 16-byte loads in the together sweep when the columns allow it
            constexpr int OD = DIMS & 3;
            const bool weighted = C.w0 != nullptr;
            auto event = [&](double w, double x, double y, double z) {
                int bin;
                if (bin_index_flat<OD>(a.outb, x, y, z, bin)) accumulate(bin, w, 1.0);
            };
            uintptr_t bits = (uintptr_t)C.w0 | (uintptr_t)C.s[0];
            if (OD > 1) bits |= (uintptr_t)C.s[1];
            if (OD > 2) bits |= (uintptr_t)C.s[2];
            if ((bits & 15) == 0) {
                const double2 *__restrict__ w2 = reinterpret_cast<const double2 *>(C.w0);
                const double2 *__restrict__ x2 = reinterpret_cast<const double2 *>(C.s[0]);
                const double2 *__restrict__ y2 = reinterpret_cast<const double2 *>(C.s[1]);
                const double2 *__restrict__ z2 = reinterpret_cast<const double2 *>(C.s[2]);
                const double2 zero = make_double2(0.0, 0.0), one = make_double2(1.0, 1.0);
                const int64_t n_wg1 = a.blk_start[c + 1] - a.blk_start[c];
                for (int64_t i = lb * nthreads + threadIdx.x; i < (C.n >> 1); i += n_wg1 * nthreads) {
                    const double2 w = weighted ? w2[i] : one;
                    const double2 x = x2[i];
                    const double2 y = OD > 1 ? y2[i] : zero;
                    const double2 z = OD > 2 ? z2[i] : zero;
                    event(w.x, x.x, y.x, z.x);
                    event(w.y, x.y, y.y, z.y);
                }
                if ((C.n & 1) && lb == 0 && threadIdx.x == 0) {  // odd tail
                    const int64_t i = C.n - 1;
                    event(weighted ? C.w0[i] : 1.0, C.s[0][i], OD > 1 ? C.s[1][i] : 0.0, OD > 2 ? C.s[2][i] : 0.0);
                }
            } else {
                for (int64_t i = start + threadIdx.x; i < end; i += nthreads)
                    event(weighted ? C.w0[i] : 1.0, C.s[0][i], OD > 1 ? C.s[1][i] : 0.0, OD > 2 ? C.s[2][i] : 0.0);
            }
        }
    }
    if (bad && status) atomicOr(status, 1);
    STAMP(3);

#ifdef PISA_DEV_PROBES
    if (a.opts & 4) return;
#endif
    if (LDS_ACC) {
        __syncthreads();
        STAMP(4);
        flush_win(my_acc == s_acc || a.copies > 1 ? s_acc : s_acc + n_acc, bin_lo, a.copies);
        if (other_lo >= 0) flush_win(my_acc == s_acc ? s_acc + n_acc : s_acc, other_lo, 1);
    }
    STAMP(5);
}


// ---------------------------------------------------------------------------
// SEVERAL PARAMETER POINTS IN ONE SWEEP OF THE EVENTS (pisa_hip_reweight_hist_multi).
// A fit with a finite-difference minimiser asks for n + 1 independent points per gradient
// (pisa/analysis/analysis.py:2493-2670 driven by settings/minimizer/l-bfgs-b_*; the reference's own
// benchmark protocol, pisa/scripts/benchmark_pipeline_performance.py:196-223, times independent points
// as well).  The 20 B per event of the 16-bit index form do not depend on the point: this kernel reads
// them ONCE, fetches the event's (P_e, P_mu) pairs of all KP points in one contiguous run of the
// interleaved tables [sign][flavour][node][point], and deposits KP weights into KP sets of LDS
// accumulators.  Per point the weight and its exact three-digit deposit are the single-point kernel's
// (`deposit_units`), so the limbs of every point hold the same sums as a pisa_hip_reweight_hist call
// at that point (tests/test_gpu_multipoint.py, tests/test_gpu_exact_accumulator.py).
constexpr int MULTI_KP_MAX = 8;   // points per launch (a larger batch is split into passes)

struct MultiCont {
    int64_t n;
    const uint32_t *idx16;
    const double2 *wflux_q;
    int32_t flav, side;
};

struct MultiArgs {
    int32_t n_cont, cont_base;
    int32_t n_bins, k_stride;   // k_stride: points interleaved in the tables
    int64_t n_nodes;
    int64_t limb_stride;        // limbs of one point (in 8-byte words)
    const double2 *pepmu;       // tables + index of this launch's first point
    MultiCont cont[MAX_CONT];
    int32_t blk_start[MAX_CONT + 1];
    int32_t pad;
    double scale[MULTI_KP_MAX][MAX_CONT];   // aeff scale per (point, container)
};

template <int KP>
__global__ void __launch_bounds__(1024)
hist_accumulate_multi_kernel(const MultiArgs a, unsigned long long *__restrict__ g_limbs,
                             int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_units[];  // [point][slab][quantity][bin], integer units
    const int nthreads = blockDim.x;
    int c = 0;
    const int bid = blockIdx.x;
    while (c + 1 < a.n_cont && bid >= a.blk_start[c + 1]) c++;  // workgroup-uniform
    const MultiCont &C = a.cont[c];
    const int64_t lb = bid - a.blk_start[c];
    const int n_bins = a.n_bins;
    const int n_acc = NL * 2 * n_bins;
    // the workgroups of a container sweep its columns together (see hist_accumulate_kernel)
    const int64_t n_wg = a.blk_start[c + 1] - a.blk_start[c];
    const int64_t qstep = n_wg * nthreads;
    const int64_t q_end = (C.n + 3) >> 2;
    int64_t q = lb * nthreads + threadIdx.x;
    const uint4 *idxq = reinterpret_cast<const uint4 *>(C.idx16);
    const uint4 none = make_uint4(~0u, ~0u, ~0u, ~0u);
    const double2 zero2 = make_double2(0.0, 0.0);
    const double2 *tab = a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes * a.k_stride;
    const int ks = a.k_stride;
    // A wavefront takes 256 consecutive events per sweep (a quad per lane).  In the engine's resident
    // order (engine.deposit_block_order) such a block either holds depositing events or none at all, so
    // "does any lane of this wavefront have an event inside the binning" is the wave-uniform question
    // that decides whether the block's flux pairs and table entries are needed at all.
    auto any_in = [](const uint4 &v) {
        const bool in = ((v.x >> 16) != 0xffffu) | ((v.y >> 16) != 0xffffu) | ((v.z >> 16) != 0xffffu) |
                        ((v.w >> 16) != 0xffffu);
        return __any(in) != 0;
    };
    auto gather = [&](unsigned word, double2 (&p)[KP]) {
        // node 0xffff (outside the calc grid): entry 0 is read and replaced by P = 0 when it is used
        const unsigned node = word & 0xffffu;
        const double2 *tp = tab + (int64_t)(node == 0xffffu ? 0u : node) * ks;
#pragma unroll
        for (int k = 0; k < KP; k++) p[k] = tp[k];
    };
    auto load_flux = [&](int64_t qq, double2 (&gg)[4]) {
        const double2 *gq = C.wflux_q + ((qq >> 6) * 256 + (qq & 63));
        gg[0] = gq[0]; gg[1] = gq[64]; gg[2] = gq[128]; gg[3] = gq[192];
    };
    // Software pipeline over the sweeps i = 0, 1, ... of this thread (what a wavefront waits for is
    // memory -- 16 wavefronts per CU, nothing else to switch to): while sweep i is deposited, the index
    // words of sweep i + 2, the flux pairs of sweep i + 1 and the table entries of the NEXT event are in
    // flight.  qx / g / p: sweep i (p: its first event); qx1: sweep i + 1.
    uint4 qx = none, qx1 = none;
    double2 g[4] = {zero2, zero2, zero2, zero2};
    double2 p[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) p[k] = zero2;
    bool have = q < q_end;
    if (have) qx = idxq[q];
    if (q + qstep < q_end) qx1 = idxq[q + qstep];
    bool in0 = any_in(qx);
    if (in0) {
        load_flux(q, g);
        gather(qx.x, p);
    }
    for (int k = threadIdx.x; k < n_acc * KP; k += nthreads) s_units[k] = 0ull;
    __syncthreads();
    double sc[KP];
#pragma unroll
    for (int k = 0; k < KP; k++) sc[k] = a.scale[k][c];
    bool bad = false;
    const int zero = 0;   // (DepositTarget: no window, no options)
    while (have) {
        const int64_t q1 = q + qstep, q2 = q1 + qstep;
        uint4 qx2 = none;
        if (q2 < q_end) qx2 = idxq[q2];
        const bool in1 = any_in(qx1);      // (lanes beyond the end hold `none`)
        double2 gn[4] = {zero2, zero2, zero2, zero2};
        if (in1) load_flux(q1, gn);
        if (in0) {
            const unsigned w4[5] = {qx.x, qx.y, qx.z, qx.w, qx1.x};
            double2 pn[KP];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                // table entries of the next event (for e = 3: the first event of the next sweep)
                if (e < 3 || in1) gather(w4[e + 1], pn);
                const unsigned node = w4[e] & 0xffffu, bin = w4[e] >> 16;
                if (bin != 0xffffu) {     // outside the binning: w = 0 for every point, nothing to deposit
#pragma unroll
                    for (int k = 0; k < KP; k++) {
                        // outside the calc grid: P = 0; the products are still formed, as in the single-point
                        // kernel (a non-finite flux is flagged there too)
                        const double2 pk = node != 0xffffu ? p[k] : zero2;
                        const double w = weight_compact(g[e].x, g[e].y, pk.x, pk.y, sc[k]);
                        // (the digits of both quantities: LDS only, addressed from the bin's accumulator of slab 0)
                        unsigned long long *const acc = s_units + k * n_acc + (int)bin, *const no_limbs = nullptr;
                        DepositTarget<true, true>{acc, n_bins, zero, no_limbs, zero, bad}(0, w, w * w);
                    }
                }
#pragma unroll
                for (int k = 0; k < KP; k++) p[k] = pn[k];
            }
        } else if (in1) {
            gather(qx1.x, p);
        }
        qx = qx1; qx1 = qx2;
#pragma unroll
        for (int e = 0; e < 4; e++) g[e] = gn[e];
        in0 = in1;
        q = q1;
        have = q < q_end;
    }
    if (bad && status) atomicOr(status, 1);
    __syncthreads();
    // slab accumulators -> integer units, added to the points' global limbs (flush_window)
    const int rot = flush_rotation(lb, n_acc);
#pragma unroll 1
    for (int k = 0; k < KP; k++) {
        unsigned long long *g_out = g_limbs + (int64_t)k * a.limb_stride + (int64_t)(a.cont_base + c) * n_bins * 2 * NL;
        flush_window(s_units + k * n_acc, 1, n_bins, n_acc, rot, nthreads,
                     [&](int g, int, unsigned long long v) { atomicAdd(&g_out[g], v); });
    }
}

__global__ void __launch_bounds__(256)
hist_average_kernel(int64_t n_bins, double *__restrict__ hist, const double *__restrict__ cnt) {
    int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bins) return;
    double v = hist[b] / cnt[b];  // translation.py:118-127: x/0 -> nan -> 0
    if (!(v == v)) v = 0.0;
    if (isinf(v)) v = v > 0 ? 1.7976931348623157e308 : -1.7976931348623157e308;
    hist[b] = v;
}

__global__ void __launch_bounds__(256)
lookup_regular_kernel(const DevBinning b, const double *__restrict__ x,
                      const double *__restrict__ y, const double *__restrict__ z, int64_t n,
                      const double *__restrict__ flat_hist, int width, double *__restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t node;
    bool in = bin_index(b, x[i], b.ndim > 1 ? y[i] : 0.0, b.ndim > 2 ? z[i] : 0.0, node);
    for (int w = 0; w < width; w++) out[i * width + w] = in ? flat_hist[node * width + w] : 0.0;
}

__global__ void __launch_bounds__(256)
apply_osc_weights_kernel(const double *__restrict__ flux, const double *__restrict__ pe,
                         const double *__restrict__ pmu, int64_t n, double *__restrict__ w) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double2 f = reinterpret_cast<const double2 *>(flux)[i];
    w[i] = w[i] * ((f.x * pe[i]) + (f.y * pmu[i]));
}

// the same with the two probabilities read at an element stride (columns of one table, e.g. the (P_e, P_mu) pairs
// of the gather tables: stride 2)
__global__ void __launch_bounds__(256)
apply_osc_weights_strided_kernel(const double *__restrict__ flux, const double *__restrict__ pe,
                                 const double *__restrict__ pmu, int64_t stride, int64_t n, double *__restrict__ w) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double2 f = reinterpret_cast<const double2 *>(flux)[i];
    w[i] = w[i] * ((f.x * pe[i * stride]) + (f.y * pmu[i * stride]));
}

// The reference's event-wise (or bin-wise) weight chain of several containers in ONE launch:
//   weights = copy(initial_weights)                        toy_event_generator.py:101-104 / the loaders
//   weights *= flux[:,0]*prob_e + flux[:,1]*prob_mu        prob3.py:621-622
//   weights *= weighted_aeff * scale                       aeff.py:87
// each step rounded to fp64 exactly as the one-step kernels above do (this file is compiled with contraction off).
constexpr int CHAIN_MAX_SETS = 24;
struct ChainArgs {
    pisa_hip_chain_set set[CHAIN_MAX_SETS];
};

__global__ void __launch_bounds__(256)
weight_chain_multi_kernel(const ChainArgs a) {
    const pisa_hip_chain_set &S = a.set[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    double w = S.d_initial_weights[i];
    if (S.d_nu_flux) {
        const double2 f = reinterpret_cast<const double2 *>(S.d_nu_flux)[i];
        w = w * ((f.x * S.d_prob_e[i * S.prob_stride]) + (f.y * S.d_prob_mu[i * S.prob_stride]));
    }
    if (S.d_weighted_aeff) w = w * (S.d_weighted_aeff[i] * S.aeff_scale);
    S.d_weights[i] = w;
}

__global__ void __launch_bounds__(256)
apply_aeff_kernel(const double *__restrict__ aeff, double scale, int64_t n,
                  double *__restrict__ w) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    w[i] = w[i] * (aeff[i] * scale);
}

// The instantiations of hist_accumulate_kernel: (mode, dimensions of the calc grid, of the output binning) -> kernel with
// LDS accumulators, kernel without (none: modes 3, 5 and 7 always have all bins or a window of them in LDS, run_hist).
typedef void (*hist_kernel_t)(const HistArgs, unsigned long long *, int32_t *);
static const struct HistForm { int mode, gd, od; hist_kernel_t lds, no_lds; } hist_forms[] = {
    {7, 0, 0, hist_accumulate_kernel<7, true>, nullptr},
    {5, 0, 0, hist_accumulate_kernel<5, true>, nullptr},
    {3, 0, 0, hist_accumulate_kernel<3, true>, nullptr},
    {2, 0, 0, hist_accumulate_kernel<2, true>, hist_accumulate_kernel<2, false>},
    {1, 1, 1, hist_accumulate_kernel<1, true, 4 * 1 + 1>, hist_accumulate_kernel<1, false, 4 * 1 + 1>},
    {1, 1, 2, hist_accumulate_kernel<1, true, 4 * 1 + 2>, hist_accumulate_kernel<1, false, 4 * 1 + 2>},
    {1, 1, 3, hist_accumulate_kernel<1, true, 4 * 1 + 3>, hist_accumulate_kernel<1, false, 4 * 1 + 3>},
    {1, 2, 1, hist_accumulate_kernel<1, true, 4 * 2 + 1>, hist_accumulate_kernel<1, false, 4 * 2 + 1>},
    {1, 2, 2, hist_accumulate_kernel<1, true, 4 * 2 + 2>, hist_accumulate_kernel<1, false, 4 * 2 + 2>},
    {1, 2, 3, hist_accumulate_kernel<1, true, 4 * 2 + 3>, hist_accumulate_kernel<1, false, 4 * 2 + 3>},
    {0, 0, 1, hist_accumulate_kernel<0, true, 1>, hist_accumulate_kernel<0, false, 1>},
    {0, 0, 2, hist_accumulate_kernel<0, true, 2>, hist_accumulate_kernel<0, false, 2>},
    {0, 0, 3, hist_accumulate_kernel<0, true, 3>, hist_accumulate_kernel<0, false, 3>},
};

static int run_hist(const ContDev *conts, int n_cont, int mode, const DevBinning *grid,
                    int64_t n_nodes, const double *prob_nu, const double *prob_nubar,
                    const double *pepmu, const DevBinning &outb, int64_t n_bins,
                    long long *d_limbs, int32_t *d_status, hipStream_t s, bool clear_first = true,
                    bool second_quantity = true) {
    if (n_bins > (1 << 28)) return PISA_HIP_ERR_INVALID;
    int64_t lds_bytes = lds_acc_bytes(n_bins);
    bool lds = lds_bytes <= LDS_ACC_BYTES_MAX;
    int window = 0;
    if (!lds && (mode == 3 || mode == 5 || mode == 7)) {
        // binning too large for LDS: accumulate a window of it (see the kernel)
        // a multiple of 32 bins: the LDS bank pair of an accumulator is then (bin - bin_lo) mod 32
        // whatever the slab and quantity, which the bank-aware event order relies on
        window = (int)(LDS_ACC_BYTES_MAX / lds_acc_bytes(1)) / 32 * 32;
        lds_bytes = lds_acc_bytes(window);
        lds = true;
    }
    // two replicas: level with one for events in the LDS-bank-aware order (no same-address
    // deposits left to spread) and with four for node-sorted events (49.6 / 53 / 49 us)
    // events in arbitrary order (modes 0 and 1: no bank-aware order, neighbouring lanes often in the
    // same bin): up to eight replicas, as LDS allows
    const int copies = window ? 1 : hist_copies(PISA_DEV_INT("HIST_COPIES", mode <= 1 ? 8 : 2), lds_bytes);
    if (clear_first)
        PISA_TRY_HIP(hipMemsetAsync(d_limbs, 0, (size_t)n_cont * n_bins * 2 * NL * 8, s));
    for (int base = 0; base < n_cont; base += MAX_CONT) {
        int nc = n_cont - base < MAX_CONT ? n_cont - base : MAX_CONT;
        HistArgs a;
        a.n_cont = nc;
        a.cont_base = base;
        a.n_bins = n_bins;
        a.n_nodes = n_nodes;
        if (grid) a.grid = *grid; else a.grid = outb;
        a.outb = outb;
        a.prob[0] = prob_nu;
        a.prob[1] = prob_nubar;
        a.pepmu = reinterpret_cast<const double2 *>(pepmu);
        a.opts = (PISA_DEV_INT("HIST_DBG", 0) & ~1) | (second_quantity ? 0 : 1);
        int64_t nev[MAX_CONT];
        for (int c = 0; c < nc; c++) {
            a.cont[c] = conts[base + c];
            nev[c] = conts[base + c].n;
            a.cont[c].dep_blocks = nullptr;   // (the planned sweep's: hist_planned.hip)
            a.cont[c].n_dep = a.cont[c].reserved = 0;
            // the partitioned order is used where its partitions are this launch's LDS windows
            if (!(window > 0 && mode == 7 && a.cont[c].part_width == window)) a.cont[c].part_start = nullptr;
        }
        const int threads = hist_threads();
        const int nblocks = plan_blocks(nev, nc, threads, a.chunk, a.blk_start);
        if (nblocks <= 0) continue;
        for (int c = 0; c < nc; c++) {
            a.cont_chunk[c] = 0;
            const int64_t nwg_c = a.blk_start[c + 1] - a.blk_start[c];
            // partitioned window order: equal shares of whole 256-event blocks per workgroup of the container
            if (a.cont[c].part_start && nwg_c > 0) {
                const int64_t blocks = (nev[c] + 255) / 256;
                a.cont_chunk[c] = (int32_t)((blocks + nwg_c - 1) / nwg_c);
            }
        }
        dim3 grid_dim((unsigned)nblocks), block(threads);
        size_t shmem = lds ? (size_t)lds_bytes * copies : 0;
        a.copies = lds ? copies : 1;
        a.window = window;
        bool parts = false;
        for (int c = 0; c < nc; c++) parts = parts || a.cont[c].part_start != nullptr;
        if (parts) {
            // partitioned order: two LDS windows per workgroup (a chunk may reach into a second partition);
            // beyond the default 64 KiB of dynamic LDS, asked for once per device
            const size_t want = (size_t)lds_bytes * 2 + (PART_MAX + 1) * sizeof(int32_t);   // + the partition table
            static std::atomic<uint64_t> attr_set{0};
            int dev = 0;
            PISA_TRY_HIP(hipGetDevice(&dev));
            const uint64_t bit = 1ull << (dev & 63);
            bool ok = (int64_t)want <= device_lds_bytes() - 256;
            if (ok && !(attr_set.load(std::memory_order_acquire) & bit)) {
                ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&hist_accumulate_kernel<7, true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(device_lds_bytes() - 256)) == hipSuccess;
                if (ok) attr_set.fetch_or(bit, std::memory_order_release);
            }
            if (ok) {
                shmem = want;
            } else {      // no room for two windows on this part: the general window path
                for (int c = 0; c < nc; c++) { a.cont[c].part_start = nullptr; a.cont_chunk[c] = 0; }
            }
        }
        unsigned long long *out = reinterpret_cast<unsigned long long *>(d_limbs);
        if (g_prof_start) PISA_TRY_HIP(hipEventRecord(g_prof_start, s));
        // (dimensions as template parameters: uniform branches and 64-bit index arithmetic otherwise, 1 080 instructions per pair)
        const int form = mode == 7 || mode == 5 || mode == 3 || mode == 2 || mode == 1 ? mode : 0;
        const int gd = form == 1 ? a.grid.ndim : 0, od = form <= 1 ? a.outb.ndim : 0;
        if (form == 1 && (gd < 1 || gd > 2 || od < 1 || od > 3 || n_nodes >= (1LL << 31) / 9)) return PISA_HIP_ERR_INVALID;
        if (form == 0 && (od < 1 || od > 3)) return PISA_HIP_ERR_INVALID;
        for (const HistForm &f : hist_forms)
            if (f.mode == form && f.gd == gd && f.od == od)
                hipLaunchKernelGGL(lds || !f.no_lds ? f.lds : f.no_lds, grid_dim, block, shmem, s, a, out, d_status);
        PISA_CHECK_LAUNCH("hist_accumulate_kernel");
        if (g_prof_stop) PISA_TRY_HIP(hipEventRecord(g_prof_stop, s));
    }
    return PISA_HIP_OK;
}

}  // namespace pisa

using namespace pisa;

#ifdef PISA_HIST_STAMPS   // (the general kernel's stamps: scripts/dev/hist_stamps.py ... general)
PISA_API int pisa_hip_debug_hist_stamps_general(unsigned long long *h_out) {
    return check_hip(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_hist_stamps), sizeof(g_hist_stamps)), "stamps");
}
#endif

PISA_API int pisa_hip_hist_workgroups(const int64_t *h_n_events, int32_t n_containers, int32_t *h_workgroups) {
    if (!h_n_events || !h_workgroups || n_containers < 1) return PISA_HIP_ERR_INVALID;
    for (int base = 0; base < n_containers; base += MAX_CONT) {
        const int nc = n_containers - base < MAX_CONT ? n_containers - base : MAX_CONT;
        int64_t chunk = 0;
        int32_t blk_start[MAX_CONT + 1];
        plan_blocks(h_n_events + base, nc, HIST_THREADS, chunk, blk_start);
        for (int c = 0; c < nc; c++) h_workgroups[base + c] = blk_start[c + 1] - blk_start[c];
    }
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_hist_window_bins(int64_t n_bins) {
    if (n_bins < 1) return -1;
    if (lds_acc_bytes(n_bins) <= LDS_ACC_BYTES_MAX) return 0;
    return (int)(LDS_ACC_BYTES_MAX / lds_acc_bytes(1)) / 32 * 32;
}

PISA_API int pisa_hip_profile_events(void *start_event, void *stop_event) {
    g_prof_start = reinterpret_cast<hipEvent_t>(start_event);
    g_prof_stop = reinterpret_cast<hipEvent_t>(stop_event);
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_event_indices(const pisa_hip_binning *h_binning,
                                    const double *const *h_d_sample, int64_t n,
                                    int32_t *d_index, void *stream) {
    DevBinning b;
    int64_t n_bins;
    int rc = make_dev_binning(h_binning, b, n_bins);
    if (rc) return rc;
    if (n < 0 || !h_d_sample || n_bins > 0x7fffffffLL) return PISA_HIP_ERR_INVALID;
    if (n == 0) return PISA_HIP_OK;
    if (!d_index) return PISA_HIP_ERR_INVALID;
    for (int k = 0; k < b.ndim; k++)
        if (!h_d_sample[k]) return PISA_HIP_ERR_INVALID;
    dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(event_indices_kernel, grid, block, 0, as_stream(stream), b, h_d_sample[0],
                       b.ndim > 1 ? h_d_sample[1] : nullptr, b.ndim > 2 ? h_d_sample[2] : nullptr,
                       n, d_index);
    PISA_CHECK_LAUNCH("event_indices_kernel");
    return PISA_HIP_OK;
}

static int reweight_hist_impl(const pisa_hip_container *h_containers, int32_t n_containers,
                              const pisa_hip_binning *h_calc_grid, const double *d_prob_nu,
                              const double *d_prob_nubar, const double *d_pepmu,
                              const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                              int32_t *d_status, void *stream, bool clear_first) {
    if (!h_containers || n_containers < 1 || n_containers > 1024 || !d_limbs)
        return PISA_HIP_ERR_INVALID;
    DevBinning grid, outb;
    int64_t n_nodes, n_bins;
    int rc = make_dev_binning(h_calc_grid, grid, n_nodes);
    if (rc) return rc;
    if (grid.ndim > 2) return PISA_HIP_ERR_INVALID;
    if ((rc = make_dev_binning(h_out_binning, outb, n_bins))) return rc;
    ContDev *conts = new ContDev[n_containers];
    bool any_table = d_pepmu != nullptr;
    for (int c = 0; c < n_containers; c++) any_table = any_table || h_containers[c].d_pepmu;
    bool all_indexed = d_pepmu != nullptr;
    bool all_packed = any_table;
    bool all_compact = any_table;
    // the 16-bit index form needs 16-bit node / bin numbers; where it does not apply its columns
    // are ignored (the other forms, if given, are used)
    const bool ok16 = n_nodes < 0xffff && n_bins < 0xffff;
    bool all_idx16 = any_table && ok16;
    for (int c = 0; c < n_containers; c++) {
        const pisa_hip_container &h = h_containers[c];
        ContDev &d = conts[c];
        const bool compact = h.d_node_bin && h.d_weighted_flux;
        const bool c16 = ok16 && h.d_node_bin16 && h.d_weighted_flux_q;  // stands alone
        bool packed = h.d_node_bin && (h.d_aeff_w0 || h.d_weighted_flux);
        bool indexed = packed || (h.d_node && h.d_bin);
        bool bad = h.n_events < 0 || h.flav < 0 || h.flav > 2 || (h.nubar != 1 && h.nubar != -1);
        if (h.n_events > 0) {
            const bool has_tab = d_pepmu || h.d_pepmu;
            bad = bad || (!h.d_nu_flux && !((compact || c16) && has_tab));
            if (!((packed || c16) && has_tab)) bad = bad || !h.d_weighted_aeff || !h.d_initial_weights;
            if (!((indexed || c16) && has_tab)) {
                bad = bad || !h.d_grid_x || (grid.ndim > 1 && !h.d_grid_y);
                for (int k = 0; k < outb.ndim; k++) bad = bad || !h.d_sample[k];
                bad = bad || (h.nubar > 0 ? !d_prob_nu : !d_prob_nubar);
            }
            all_indexed = all_indexed && indexed && (h.d_node && h.d_bin);
            all_packed = all_packed && packed && has_tab && h.d_aeff_w0 && h.d_nu_flux;
            all_compact = all_compact && compact && has_tab;
            all_idx16 = all_idx16 && c16 && has_tab;
        }
        if (bad) { delete[] conts; return PISA_HIP_ERR_INVALID; }
        d.n = h.n_events;
        d.gx = h.d_grid_x; d.gy = h.d_grid_y; d.flux = h.d_nu_flux; d.aeff = h.d_weighted_aeff;
        d.w0 = h.d_initial_weights;
        for (int k = 0; k < 3; k++) d.s[k] = h.d_sample[k];
        d.node = h.d_node; d.bin = h.d_bin;
        d.node_bin = reinterpret_cast<const int2 *>(h.d_node_bin);
        d.aeff_w0 = reinterpret_cast<const double2 *>(h.d_aeff_w0);
        d.pepmu_own = reinterpret_cast<const double2 *>(h.d_pepmu);
        d.wflux = reinterpret_cast<const double2 *>(h.d_weighted_flux);
        d.idx16 = h.d_node_bin16;
        d.wflux_q = reinterpret_cast<const double2 *>(h.d_weighted_flux_q);
        d.part_start = (h.d_part_start && h.n_part >= 1 && h.n_part <= PART_MAX && h.part_width > 0) ? h.d_part_start : nullptr;
        d.n_part = h.n_part;
        d.part_width = h.part_width;
        d.scale = h.scale;
        d.flav = h.flav;
        d.side = h.nubar > 0 ? 0 : 1;
    }
    rc = run_hist(conts, n_containers, all_idx16 ? 7 : all_compact ? 5 : (all_packed ? 3 : (all_indexed ? 2 : 1)), &grid, n_nodes, d_prob_nu, d_prob_nubar,
                  d_pepmu, outb, n_bins, (long long *)d_limbs, d_status, as_stream(stream), clear_first);
    delete[] conts;
    return rc;
}

PISA_API int pisa_hip_reweight_hist(const pisa_hip_container *h_containers, int32_t n_containers,
                                    const pisa_hip_binning *h_calc_grid, const double *d_prob_nu,
                                    const double *d_prob_nubar, const double *d_pepmu,
                                    const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                                    int32_t *d_status, void *stream) {
    return reweight_hist_impl(h_containers, n_containers, h_calc_grid, d_prob_nu, d_prob_nubar,
                              d_pepmu, h_out_binning, d_limbs, d_status, stream, true);
}

PISA_API int pisa_hip_reweight_hist_acc(const pisa_hip_container *h_containers,
                                        int32_t n_containers, const pisa_hip_binning *h_calc_grid,
                                        const double *d_prob_nu, const double *d_prob_nubar,
                                        const double *d_pepmu,
                                        const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                                        int32_t *d_status, void *stream) {
    return reweight_hist_impl(h_containers, n_containers, h_calc_grid, d_prob_nu, d_prob_nubar,
                              d_pepmu, h_out_binning, d_limbs, d_status, stream, false);
}


template <int KP>
static int launch_multi(const MultiArgs &a, int nblocks, size_t shmem, unsigned long long *out,
                        int32_t *d_status, hipStream_t s) {
    // LDS beyond the default 64 KiB has to be asked for once per kernel AND device
    static std::atomic<uint64_t> attr_set{0};
    int dev = 0;
    PISA_TRY_HIP(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (shmem > 64 * 1024 && !(attr_set.load(std::memory_order_acquire) & bit)) {
        const int64_t limit = device_lds_bytes() - 256;
        if ((int64_t)shmem > limit) return PISA_HIP_ERR_INVALID;
        PISA_TRY_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&hist_accumulate_multi_kernel<KP>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL((hist_accumulate_multi_kernel<KP>), dim3((unsigned)nblocks), dim3(HIST_THREADS), shmem, s,
                       a, out, d_status);
    PISA_CHECK_LAUNCH("hist_accumulate_multi_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_multi_points_per_pass(int64_t n_bins) {
    if (n_bins < 1) return 0;
    int64_t lds_max = 128 * 1024;
    if (lds_max > device_lds_bytes() - 256) lds_max = device_lds_bytes() - 256;   // a part with 64 KiB LDS: fewer points per pass
    int64_t kp = lds_max / lds_acc_bytes(n_bins);
    if (kp > MULTI_KP_MAX) kp = MULTI_KP_MAX;
    return kp < 2 ? 0 : (int)kp;   // one point per pass is the single-point path's job
}

PISA_API int pisa_hip_reweight_hist_multi(const pisa_hip_container *h_containers, int32_t n_containers,
                                          const pisa_hip_binning *h_calc_grid, const double *d_pepmu_points,
                                          int32_t n_points, const double *h_scales,
                                          const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                                          int32_t clear_first, int32_t *d_status, void *stream) {
    if (!h_containers || n_containers < 1 || n_containers > 1024 || !d_limbs || !d_pepmu_points ||
        n_points < 1 || n_points > PISA_HIP_MAX_POINTS)
        return PISA_HIP_ERR_INVALID;
    DevBinning grid, outb;
    int64_t n_nodes, n_bins;
    int rc = make_dev_binning(h_calc_grid, grid, n_nodes);
    if (rc) return rc;
    if ((rc = make_dev_binning(h_out_binning, outb, n_bins))) return rc;
    if (n_nodes >= 0xffff || n_bins >= 0xffff) return PISA_HIP_ERR_INVALID;
    const int kp_max = pisa_hip_multi_points_per_pass(n_bins);
    if (kp_max < 1) return PISA_HIP_ERR_INVALID;   // binning beyond the LDS accumulators: point by point
    for (int c = 0; c < n_containers; c++) {
        const pisa_hip_container &h = h_containers[c];
        if (h.n_events < 0 || h.flav < 0 || h.flav > 2 || (h.nubar != 1 && h.nubar != -1)) return PISA_HIP_ERR_INVALID;
        // the 16-bit index form with the shared grid tables only
        if (h.n_events > 0 && (!h.d_node_bin16 || !h.d_weighted_flux_q || h.d_pepmu)) return PISA_HIP_ERR_INVALID;
    }
    hipStream_t s = as_stream(stream);
    const int64_t limb_stride = (int64_t)n_containers * n_bins * 2 * NL;
    if (clear_first) PISA_TRY_HIP(hipMemsetAsync(d_limbs, 0, (size_t)n_points * limb_stride * 8, s));
    const int n_pass = (n_points + kp_max - 1) / kp_max;
    for (int pass = 0, k0 = 0; pass < n_pass; pass++) {
        const int kp = (n_points - k0 + (n_pass - pass) - 1) / (n_pass - pass);   // passes of equal size
        // workgroups: what is resident at once.  From two points on the kernel needs more than 64 VGPRs,
        // a CU holds ONE 1024-thread workgroup, and a second round of workgroups would only add a tail
        const int64_t target_blocks = device_cus();
        for (int base = 0; base < n_containers; base += MAX_CONT) {
            const int nc = n_containers - base < MAX_CONT ? n_containers - base : MAX_CONT;
            MultiArgs a;
            memset(&a, 0, sizeof(a));
            a.n_cont = nc;
            a.cont_base = base;
            a.n_bins = (int32_t)n_bins;
            a.k_stride = n_points;
            a.n_nodes = n_nodes;
            a.limb_stride = limb_stride;
            a.pepmu = reinterpret_cast<const double2 *>(d_pepmu_points) + k0;
            int64_t nev[MAX_CONT];
            for (int c = 0; c < nc; c++) {
                const pisa_hip_container &h = h_containers[base + c];
                a.cont[c].n = h.n_events;
                a.cont[c].idx16 = h.d_node_bin16;
                a.cont[c].wflux_q = reinterpret_cast<const double2 *>(h.d_weighted_flux_q);
                a.cont[c].flav = h.flav;
                a.cont[c].side = h.nubar > 0 ? 0 : 1;
                nev[c] = h.n_events;
                for (int k = 0; k < kp; k++)
                    a.scale[k][c] = h_scales ? h_scales[(size_t)(k0 + k) * n_containers + base + c] : h.scale;
            }
            int64_t chunk;
            const int nblocks = plan_blocks_balanced(nev, nc, HIST_THREADS, target_blocks, chunk, a.blk_start);
            if (nblocks <= 0) continue;
            const size_t shmem = (size_t)lds_acc_bytes(n_bins) * kp;
            unsigned long long *out = reinterpret_cast<unsigned long long *>(d_limbs) + (int64_t)k0 * limb_stride;
            if (g_prof_start) PISA_TRY_HIP(hipEventRecord(g_prof_start, s));
            switch (kp) {
            case 1: rc = launch_multi<1>(a, nblocks, shmem, out, d_status, s); break;
            case 2: rc = launch_multi<2>(a, nblocks, shmem, out, d_status, s); break;
            case 3: rc = launch_multi<3>(a, nblocks, shmem, out, d_status, s); break;
            case 4: rc = launch_multi<4>(a, nblocks, shmem, out, d_status, s); break;
            case 5: rc = launch_multi<5>(a, nblocks, shmem, out, d_status, s); break;
            case 6: rc = launch_multi<6>(a, nblocks, shmem, out, d_status, s); break;
            case 7: rc = launch_multi<7>(a, nblocks, shmem, out, d_status, s); break;
            default: rc = launch_multi<8>(a, nblocks, shmem, out, d_status, s); break;
            }
            if (rc) return rc;
            if (g_prof_stop) PISA_TRY_HIP(hipEventRecord(g_prof_stop, s));
        }
        k0 += kp;
    }
    return PISA_HIP_OK;
}

// Generic histogram.  Its scratch (limbs, counts, status word) lives in a grow-only buffer per host
// thread: three hipMalloc / hipFree pairs per call cost more than the kernels (72 us for a call that
// moves 80 MB).  The call still ends with a stream synchronisation -- it returns the status.
static thread_local char *g_hist_scratch = nullptr;
static thread_local size_t g_hist_scratch_bytes = 0;

PISA_API int pisa_hip_histogram_regular(const pisa_hip_binning *h_binning,
                                        const double *const *h_d_sample, int64_t n,
                                        const double *d_weights, int32_t averaged, double *d_hist,
                                        void *stream) {
    DevBinning outb;
    int64_t n_bins;
    int rc = make_dev_binning(h_binning, outb, n_bins);
    if (rc) return rc;
    if (n < 0 || !d_hist || !h_d_sample) return PISA_HIP_ERR_INVALID;
    for (int k = 0; k < outb.ndim; k++)
        if (n > 0 && !h_d_sample[k]) return PISA_HIP_ERR_INVALID;
    hipStream_t s = as_stream(stream);
    const size_t limb_bytes = (size_t)n_bins * 2 * NL * 8, cnt_bytes = (size_t)n_bins * 8;
    const size_t need = limb_bytes + cnt_bytes + 256;
    if (need > g_hist_scratch_bytes) {
        if (g_hist_scratch) (void)hipFree(g_hist_scratch);
        g_hist_scratch = nullptr;
        g_hist_scratch_bytes = 0;
        rc = check_hip(hipMalloc(&g_hist_scratch, need), "hipMalloc");
        if (rc) return rc;
        g_hist_scratch_bytes = need;
    }
    long long *limbs = reinterpret_cast<long long *>(g_hist_scratch);
    double *cnt = reinterpret_cast<double *>(g_hist_scratch + limb_bytes);
    int32_t *st = reinterpret_cast<int32_t *>(g_hist_scratch + limb_bytes + cnt_bytes);
    rc = check_hip(hipMemsetAsync(st, 0, 4, s), "memset");
    if (!rc) {
        ContDev c;
        c.n = n; c.gx = c.gy = c.flux = c.aeff = nullptr; c.w0 = d_weights;
        for (int k = 0; k < 3; k++) c.s[k] = k < outb.ndim ? h_d_sample[k] : nullptr;
        c.node = c.bin = nullptr;
        c.node_bin = nullptr; c.aeff_w0 = nullptr; c.pepmu_own = nullptr; c.wflux = nullptr;
        c.idx16 = nullptr; c.wflux_q = nullptr;
        c.scale = 1.0; c.flav = 0; c.side = 0;
        // the per-bin counts (second quantity) are needed for the average only
        rc = run_hist(&c, 1, 0, nullptr, 0, nullptr, nullptr, nullptr, outb, n_bins, limbs, st, s, true,
                      averaged != 0);
    }
    if (!rc) rc = pisa_hip_hist_finalize((const int64_t *)limbs, 1, n_bins, d_hist, cnt, st, s);
    if (!rc && averaged) {
        dim3 block(256), grid((unsigned)((n_bins + 255) / 256));
        hipLaunchKernelGGL(hist_average_kernel, grid, block, 0, s, n_bins, d_hist, cnt);
        rc = check_hip(hipGetLastError(), "hist_average_kernel");
    }
    int32_t h_st = 0;
    if (!rc) rc = check_hip(hipMemcpyAsync(&h_st, st, 4, hipMemcpyDeviceToHost, s), "d2h");
    if (!rc) rc = check_hip(hipStreamSynchronize(s), "sync");
    if (!rc && h_st) rc = PISA_HIP_ERR_OVERFLOW;
    return rc;
}

PISA_API int pisa_hip_lookup_regular(const pisa_hip_binning *h_binning,
                                     const double *const *h_d_sample, int64_t n,
                                     const double *d_flat_hist, int32_t width, double *d_out,
                                     void *stream) {
    DevBinning b;
    int64_t n_bins;
    int rc = make_dev_binning(h_binning, b, n_bins);
    if (rc) return rc;
    if (n < 0 || width < 1 || !h_d_sample) return PISA_HIP_ERR_INVALID;
    if (n == 0) return PISA_HIP_OK;
    if (!d_flat_hist || !d_out) return PISA_HIP_ERR_INVALID;
    for (int k = 0; k < b.ndim; k++)
        if (!h_d_sample[k]) return PISA_HIP_ERR_INVALID;
    dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(lookup_regular_kernel, grid, block, 0, as_stream(stream), b, h_d_sample[0],
                       b.ndim > 1 ? h_d_sample[1] : nullptr, b.ndim > 2 ? h_d_sample[2] : nullptr,
                       n, d_flat_hist, (int)width, d_out);
    PISA_CHECK_LAUNCH("lookup_regular_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_apply_osc_weights(const double *d_nu_flux, const double *d_prob_e,
                                        const double *d_prob_mu, int64_t n, double *d_weights,
                                        void *stream) {
    if (n < 0) return PISA_HIP_ERR_INVALID;
    if (n == 0) return PISA_HIP_OK;
    if (!d_nu_flux || !d_prob_e || !d_prob_mu || !d_weights) return PISA_HIP_ERR_INVALID;
    dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(apply_osc_weights_kernel, grid, block, 0, as_stream(stream), d_nu_flux,
                       d_prob_e, d_prob_mu, n, d_weights);
    PISA_CHECK_LAUNCH("apply_osc_weights_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_apply_osc_weights_strided(const double *d_nu_flux, const double *d_prob_e,
                                                const double *d_prob_mu, int64_t prob_stride, int64_t n,
                                                double *d_weights, void *stream) {
    if (n < 0 || prob_stride < 1) return PISA_HIP_ERR_INVALID;
    if (n == 0) return PISA_HIP_OK;
    if (!d_nu_flux || !d_prob_e || !d_prob_mu || !d_weights) return PISA_HIP_ERR_INVALID;
    dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(apply_osc_weights_strided_kernel, grid, block, 0, as_stream(stream), d_nu_flux,
                       d_prob_e, d_prob_mu, prob_stride, n, d_weights);
    PISA_CHECK_LAUNCH("apply_osc_weights_strided_kernel");
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_weight_chain_multi(const pisa_hip_chain_set *h_sets, int32_t n_sets, void *stream) {
    if (!h_sets || n_sets < 1 || n_sets > 4096) return PISA_HIP_ERR_INVALID;
    for (int k = 0; k < n_sets; k++) {
        const pisa_hip_chain_set &h = h_sets[k];
        if (h.n < 0 || (h.n > 0 && (!h.d_initial_weights || !h.d_weights)) ||
            (h.n > 0 && h.d_nu_flux && (!h.d_prob_e || !h.d_prob_mu || h.prob_stride < 1)))
            return PISA_HIP_ERR_INVALID;
    }
    for (int base = 0; base < n_sets; base += CHAIN_MAX_SETS) {
        const int nc = n_sets - base < CHAIN_MAX_SETS ? n_sets - base : CHAIN_MAX_SETS;
        ChainArgs a;
        int64_t n_max = 0;
        for (int k = 0; k < nc; k++) { a.set[k] = h_sets[base + k]; n_max = std::max(n_max, h_sets[base + k].n); }
        if (n_max == 0) continue;
        dim3 block(256), grid((unsigned)((n_max + 255) / 256), (unsigned)nc);
        hipLaunchKernelGGL(weight_chain_multi_kernel, grid, block, 0, as_stream(stream), a);
        PISA_CHECK_LAUNCH("weight_chain_multi_kernel");
    }
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_apply_aeff(const double *d_weighted_aeff, double scale, int64_t n,
                                 double *d_weights, void *stream) {
    if (n < 0) return PISA_HIP_ERR_INVALID;
    if (n == 0) return PISA_HIP_OK;
    if (!d_weighted_aeff || !d_weights) return PISA_HIP_ERR_INVALID;
    dim3 block(256), grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(apply_aeff_kernel, grid, block, 0, as_stream(stream), d_weighted_aeff,
                       scale, n, d_weights);
    PISA_CHECK_LAUNCH("apply_aeff_kernel");
    return PISA_HIP_OK;
}
