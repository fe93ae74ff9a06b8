// hist_device.hpp -- what every accumulate kernel shares (hist.hip: the general forms and the multi-point kernel,
// hist_planned.hip: the planned sweep) and the rounding of their sums (hist_tail.hip): the exact accumulator, the
// argument block, the flush of the LDS accumulators, the weight chains.
//
// ORDER-INDEPENDENT ACCUMULATION.  Every summand x = +-m 2^e is cut EXACTLY into the (at most
// three) 32-bit digits it occupies in a fixed-point number of NL 32-bit slabs with LSB 2^-116
// (`deposit_units`); the digits are added with integer LDS atomics (ds_add_u64) into slab
// accumulators [slab][quantity][bin], which give the same sum whatever the event order.  At
// the end of a workgroup the slab accumulators are added to the global limb array with integer
// atomics (associative => the result is independent of workgroup scheduling, workgroup count
// and GPU count).  The limbs [container][bin][quantity][6] can be SUM-all-reduced across ranks
// as int64 and are rounded ONCE (round-to-nearest-even) to fp64 by hist_finalize.
// Range: |x| < 2^76, resolution 2^-116; outside -> status flag.
#pragma once
#include "common.hpp"

namespace pisa {

constexpr int NL = PISA_HIP_ACC_LIMBS;  // slabs ("limbs") per accumulator
constexpr int FX_LSB = 116;             // value = sum limb_j * 2^(32j - 116)
constexpr int MAX_CONT = 16;            // containers per launch (kernarg budget)
constexpr int PART_MAX = 255;           // partitions of a container's resident order (pisa_hip_container::d_part_start)
constexpr int HIST_THREADS = 1024;
constexpr int64_t LDS_ACC_BYTES_MAX = 64 * 1024;

// The exact decomposition in integer arithmetic: x = +-m * 2^(ex-1075), m the 53-bit significand,
// is truncated to a multiple of 2^-116 and cut into the (at most three) 32-bit digits it occupies,
//   digit[jj] = (|x| / 2^-116 >> 32 jj) & 0xffffffff,  jj = j, j-1, j-2,  j = slab of the leading bit,
// each handed to add(jj, +-digit) as a signed 64-bit count of units 2^(32jj-116).  Integer additions are
// associative, so sums of these counts are exact in any order as long as they fit 64 bits (2^31 events
// per accumulator).  Two 64-bit shifts: a third of the instructions of the rounded add/subtract pairs that
// cut a summand in csrc/kde.hip (`deposit` there), which is what bounds the multi-point kernel.  Every
// histogram kernel -- single point, planned, several points, generic -- cuts with these two functions,
// so all of them hold the same exact sums.  |x| < 2^-116 deposits nothing; digits below slab 0 are dropped
// (truncation towards zero: x contributes sign(x) floor(|x| 2^116) units; tests/test_gpu_exact_accumulator.py).
// LDS and global integer atomics with their own memory scopes: apart from being what is meant, the
// different scopes keep the optimiser from merging an `in LDS ? ... : ...` pair of atomics into one
// atomic on a generic pointer (which this compiler then fails to select).
__device__ __forceinline__ void lds_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (the LDS accumulator at a 32-bit LDS byte address: the planned sweep forms its addresses as integers)
typedef __attribute__((address_space(3))) unsigned long long *lds_u64;
__device__ __forceinline__ void lds_add_at(unsigned at, unsigned long long v) {
    (void)__hip_atomic_fetch_add((lds_u64)(uintptr_t)at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void glb_add(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class F>
__device__ __forceinline__ bool deposit_units_general(double x, F &&add) {
    const unsigned hi = (unsigned)__double2hiint(x);
    const int ex = (hi >> 20) & 0x7ff;
    if (ex == 0x7ff) return false;        // Inf / NaN
    const int t = ex - 1023 + FX_LSB;     // position of the leading bit above the LSB of the format
    if (t < 0) return true;               // below 2^-116 (incl. zero / subnormals)
    const int j = t >> 5;
    if (j >= NL) return false;            // |x| >= 2^76
    const int sh = t & 31;                // position of the leading bit inside digit j
    const unsigned long long m =
        ((unsigned long long)((hi & 0xfffffu) | 0x100000u) << 32) | (unsigned)__double2loint(x);
    const unsigned long long low = m << (sh + 12);     // digits j-1 (high word) and j-2 (low word)
    long long d0 = (long long)(m >> (52 - sh));
    long long d1 = (long long)(low >> 32);
    long long d2 = (long long)(low & 0xffffffffull);
    if ((int)hi < 0) { d0 = -d0; d1 = -d1; d2 = -d2; }
    add(j, d0);
    if (j >= 1 && d1 != 0) add(j - 1, d1);
    if (j >= 2 && d2 != 0) add(j - 2, d2);
    return true;
}

// The case that occurs: x positive, 2^-52 <= x < 2^76 (leading bit in digit 2 or above), where the three
// digits exist and none needs a sign -- no branch inside, `add3(j, d0, d1, d2)` receives the digits of
// slabs j, j-1, j-2 at once.  Anything else (negative, tiny, non-finite, too large) takes the general
// form above; the wavefront decides once (`__any`), so the rare path costs nothing when nobody needs it.
template <class F3, class F>
__device__ __forceinline__ bool deposit_units(double x, F3 &&add3, F &&add) {
    const unsigned hi = (unsigned)__double2hiint(x);
    const unsigned t = (hi >> 20) - (1023u - FX_LSB);          // sign bit set: huge -> not `fast`
    const bool fast = (t - 64u) < (unsigned)(NL * 32 - 64);
    bool ok = true;
    if (__any(!fast)) {
        if (!fast) ok = deposit_units_general(x, add);
    }
    if (fast) {
        const unsigned sh = t & 31u;
        const unsigned long long m =
            ((unsigned long long)((hi & 0xfffffu) | 0x100000u) << 32) | (unsigned)__double2loint(x);
        const unsigned long long low = m << (sh + 12u);
        add3((int)(t >> 5), m >> (52u - sh), low >> 32, low & 0xffffffffull);
    }
    return ok;
}

// The deposit target of the accumulate kernels: the two quantities (w, w2) of one event into bin `bin`.  Digits of slabs
// j, j-1, j-2 of one weight (deposit_units) go to the LDS accumulators `acc` = [slab][quantity][n_bins bins from bin_lo]
// of this workgroup, or -- bins outside the LDS window, binnings without LDS accumulators -- to the global limbs g_out.
// ALL_LDS: every bin is in LDS (no window: bin_lo = 0, g_out unused).  opts: HistArgs::opts.  bad: set where a weight
// did not fit.  References to the kernel's own variables (the general kernel moves acc and bin_lo as it goes).
template <bool LDS_ACC, bool ALL_LDS>
struct DepositTarget {
    unsigned long long *const &acc;
    const int &n_bins, &bin_lo;
    unsigned long long *const &g_out;
    const int &opts;
    bool &bad;
    __device__ __forceinline__ void operator()(int bin, double w, double w2) const {
        const int rel = bin - bin_lo;
        const bool in_lds = ALL_LDS || (LDS_ACC && (unsigned)rel < (unsigned)n_bins);
        auto put = [&](int qn, int j, unsigned long long d) {
            if (in_lds) lds_add(&acc[__mul24(j * 2 + qn, n_bins) + rel], d);
            else glb_add(&g_out[((int64_t)bin * 2 + qn) * NL + j], d);
        };
        auto add0 = [&](int j, long long d) { put(0, j, (unsigned long long)d); };
        auto add1 = [&](int j, long long d) { put(1, j, (unsigned long long)d); };
        auto put3 = [&](int qn, int j, unsigned long long d0, unsigned long long d1, unsigned long long d2) {
            if (in_lds) {
                const int i0 = __mul24(j * 2 + qn, n_bins) + rel;
                lds_add(&acc[i0], d0); lds_add(&acc[i0 - 2 * n_bins], d1); lds_add(&acc[i0 - 4 * n_bins], d2);
            } else {
                const int64_t i0 = ((int64_t)bin * 2 + qn) * NL + j;
                glb_add(&g_out[i0], d0); glb_add(&g_out[i0 - 1], d1); glb_add(&g_out[i0 - 2], d2);
            }
        };
        auto add30 = [&](int j, unsigned long long d0, unsigned long long d1, unsigned long long d2) { put3(0, j, d0, d1, d2); };
        auto add31 = [&](int j, unsigned long long d0, unsigned long long d1, unsigned long long d2) { put3(1, j, d0, d1, d2); };
#ifdef PISA_DEV_PROBES
        if (opts & 2) {  // probe: keep the loads and the weight chain alive, no atomics
            if (w == 1.2345e-300 || w2 == 1.2345e-300) bad = true;
            return;
        }
#endif
        bool ok = deposit_units(w, add30, add0);
        if (!(opts & 1)) ok = deposit_units(w2, add31, add1) && ok;
        if (!ok) bad = true;
    }
};

// ---------------------------------------------------------------------------
struct ContDev {
    int64_t n;
    const double *gx, *gy, *flux, *aeff, *w0;
    const double *s[3];
    const int32_t *node, *bin;  // optional pre-digitised indices
    const int2 *node_bin;       // optional packed (node, bin) per event
    const double2 *aeff_w0;     // optional packed (weighted_aeff, initial_weights) per event
    const double2 *pepmu_own;   // optional per-container (P_e, P_mu) table (event-mode prob3)
    const double2 *wflux;       // optional static-weighted flux (w0*aeff*f_e, w0*aeff*f_mu) per event
    const uint32_t *idx16;      // optional 16-bit packed (node | bin << 16) per event, 0xffff = outside
    const double2 *wflux_q;     // wflux in quad-blocked order [q / 64][4][q % 64], padded to 256 events
    double scale;
    int32_t flav, side;
    // optional, 16-bit index form with a binning beyond the LDS accumulators: the resident order is cut into
    // n_part partitions, partition p = events [256 part_start[p], 256 part_start[p+1]) holding only deposits into
    // bins [p W, (p+1) W), W = the LDS window (HistArgs::window)
    const int32_t *part_start;
    int32_t n_part, part_width;
    // pisa_hip_hist_plan (hist_planned_kernel): the n_dep blocks of 256 events that hold an event which can deposit, ascending
    // -- the sweep visits these and no other block; bit 31 of an entry: the block also holds an event that deposits nothing
    const int32_t *dep_blocks;
    int32_t n_dep, reserved;
};

struct HistArgs {
    int32_t n_cont;
    int32_t cont_base;    // index of cont[0] in the output limb array
    int64_t n_bins;
    int64_t n_nodes;      // calc-grid nodes (stride of the (P_e,P_mu) tables)
    int64_t chunk;        // events per workgroup (multiple of 2*HIST_THREADS)
    DevBinning grid;      // calc grid (lookup)
    DevBinning outb;      // output binning
    const double *prob[2];   // P[node][3][3] for nu / nubar
    const double2 *pepmu;    // optional compact tables [side][flav][node] = (P_e->f, P_mu->f)
    ContDev cont[MAX_CONT];
    int32_t blk_start[MAX_CONT + 1];
    int32_t cont_chunk[MAX_CONT];   // > 0: events per workgroup of this container / 256 (instead of `chunk`)
    int32_t copies;       // LDS replicas of the accumulators (power of two), lane-interleaved
    int32_t opts;         // 1: the caller has no use for the second quantity (plain histogram without counts).
                          // Development library only (PISA_HIP_HIST_DBG): 2 no deposits, 4 no flush
    int32_t window;       // > 0: LDS holds this many bins starting at the chunk's lowest bin
};
static_assert(sizeof(HistArgs) + 2 * sizeof(void *) <= 4096, "kernel arguments of the accumulate kernels beyond 4 KiB");

// One window of LDS slab accumulators (`ncopies` replicas of n_acc = NL * 2 * n_bins words, first bin `lo`) -> integer
// units, handed to add(g, bin, v): v units for word g = (bin * 2 + quantity) * NL + slab of the window's limbs.  The
// loop runs in GLOBAL order (limb fastest): a wave's 64 atomics fall into 512 contiguous bytes, which the L2 atomic
// units take at full rate (scattered 96 B apart they do not).  Workgroups of a container finish together; each starts
// at a different offset `rot` (flush_rotation of its ordinal lb) so that they do not all queue on the same limbs.
__device__ __forceinline__ int flush_rotation(int64_t lb, int n_acc) { return (int)((lb * 7 * 64) % n_acc); }
template <class F>
__device__ __forceinline__ void flush_window(const unsigned long long *win, int ncopies, int n_bins, int n_acc,
                                             int rot, int nthreads, F &&add) {
    for (int g0 = threadIdx.x; g0 < n_acc; g0 += nthreads) {
        int g = g0 + rot;
        if (g >= n_acc) g -= n_acc;
        const int bin = g / (2 * NL);
        const int rem = g - bin * 2 * NL;
        const int q = rem / NL;
        const int j = rem - q * NL;
        const int k = (j * 2 + q) * n_bins + bin;
        unsigned long long v = win[k];
        for (int r = 1; r < ncopies; r++) v += win[r * n_acc + k];  // integer: exact
        if (v != 0ull) add(g, bin, v);
    }
}

// The two weight chains (-ffp-contract=off for the files that use them: the association is the rounding).  Compact: the flux pair
// (g_e, g_mu) pre-multiplied by the static per-event factor initial_weights * weighted_aeff.  Reference: its own order.
__device__ __forceinline__ double weight_compact(double ge, double gmu, double pe, double pmu, double scale) {
    return ((ge * pe) + (gmu * pmu)) * scale;
}
__device__ __forceinline__ double weight_reference(double w0, double fe, double fmu, double pe, double pmu, double ae, double scale) {
    const double w = w0 * ((fe * pe) + (fmu * pmu));  // prob3.py:622
    return w * (ae * scale);                          // aeff.py:87
}

// Development build (make EXTRA=-DPISA_HIST_STAMPS, scripts/dev/hist_stamps.py): wall-clock stamps of
// thread 0 of every workgroup at six points of the kernel, in the g_hist_stamps of the file that holds the kernel.
#ifdef PISA_HIST_STAMPS
#define STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 1024) g_hist_stamps[8 * blockIdx.x + (k)] = wall_clock64(); } while (0)
#else
#define STAMP(k) do {} while (0)
#endif

// limbs (possibly summed over workgroups and ranks, un-normalised) -> fp64,
// rounded once (RNE).  Sets *ovf if the value does not fit the format.
__device__ __forceinline__ double limbs_to_double(const long long *in, bool &ovf) {
    long long L[NL + 1];
    long long carry = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
        long long v = in[k] + carry;
        carry = v >> 32;  // arithmetic shift = floor division
        L[k] = v & 0xffffffffLL;
    }
    L[NL] = carry;  // signed remainder
    bool neg = L[NL] < 0;
    if (neg) {
        long long c2 = 1;  // two's complement negate of the (NL+1)-limb number
#pragma unroll
        for (int k = 0; k < NL; k++) {
            long long v = (0xffffffffLL - L[k]) + c2;
            c2 = v >> 32;
            L[k] = v & 0xffffffffLL;
        }
        L[NL] = ~L[NL] + c2;
    }
    if (L[NL] != 0) ovf = true;
    // the NL digits as three 64-bit words; the highest non-zero word and the two below it, shifted so
    // that the value's leading bit is bit 63 of `top`: 64 significant bits and a sticky bit for the rest
    // (no indexing of the digit array with a run-time index: that costs a select chain per access)
    static_assert(NL == 6, "three 64-bit words");
    const unsigned long long w0 = (unsigned long long)L[0] | ((unsigned long long)L[1] << 32);
    const unsigned long long w1 = (unsigned long long)L[2] | ((unsigned long long)L[3] << 32);
    const unsigned long long w2 = (unsigned long long)L[4] | ((unsigned long long)L[5] << 32);
    if ((w0 | w1 | w2) == 0ULL) return 0.0;
    unsigned long long a_, b_, c_;
    int base;
    if (w2) { a_ = w2; b_ = w1; c_ = w0; base = 128; }
    else if (w1) { a_ = w1; b_ = w0; c_ = 0ULL; base = 64; }
    else { a_ = w0; b_ = 0ULL; c_ = 0ULL; base = 0; }
    const int s_ = __clzll(a_);   // 0 .. 63
    unsigned long long top = a_, lost = b_ | c_;
    if (s_) {
        top = (a_ << s_) | (b_ >> (64 - s_));
        lost = (b_ << s_) | c_;   // (only whether anything is left matters)
    }
    if (lost != 0ULL) top |= 1ULL;   // sticky bit: sits below the rounding position (bit 11 of `top`)
    double d = (double)top;           // u64 -> f64 is round-to-nearest-even
    d = ldexp(d, base - s_ - FX_LSB);
    return neg ? -d : d;
}

}  // namespace pisa
