// hist_planned.hip -- THE ACCUMULATE PLAN (pisa_hip_hist_plan_*), its kernel and its launch for gfx950: which events lie
// outside the output binning is fixed by the binning and the events' static coordinates; the resident order (order.hip,
// `deposit_block_order`) gathers the others into whole blocks of 256.  The plan lists those blocks once -- and marks the
// listed blocks that also hold an event which deposits nothing --, and hist_planned_kernel then streams them alone:
// the sweep that every headline evaluation runs.
#include <type_traits>
#include <vector>

#include "hist_host.hpp"

// The accumulate plan of a set of containers (include/pisa_hip.h, pisa_hip_hist_plan_create): which 256-event
// blocks of every container hold an event that can deposit, and the work split of the launches that sweep them.
struct pisa_hip_hist_plan {
    int32_t n_cont = 0, threads = 0;
    int64_t n_nodes = 0, n_bins = 0;
    std::vector<int64_t> n_events;           // per container: the snapshot a planned call is checked against
    std::vector<int32_t> n_blocks, n_dep;    // per container: blocks of 256 events / those that deposit
    std::vector<const int32_t *> list;       // per container: DEVICE block numbers, ascending, bit 31 = needs guards
    std::vector<int64_t> offset;             // per container: its list starts at d_lists + offset
    std::vector<int32_t> blk_start;          // per launch (MAX_CONT containers): MAX_CONT + 1 entries
    std::vector<int64_t> chunk;              // per launch
    int32_t *d_lists = nullptr;              // one allocation: the lists, the counts, the marks
};

namespace pisa {

#ifdef PISA_HIST_STAMPS
static __device__ unsigned long long g_hist_stamps[8 * 1024];
#endif

// THE PLANNED SWEEP: the 16-bit index form (20 B per event, four events per thread and sweep; MODE 7 of
// hist_accumulate_kernel, hist.hip) with every bin in LDS, over the blocks of the plan's list.  The workgroups of a
// container sweep its columns TOGETHER, and the loads of the first sweep are issued before the LDS accumulators are
// cleared, so that the clearing overlaps the first HBM round trip.
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
hist_planned_kernel(const HistArgs a, unsigned long long *__restrict__ g_limbs, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_acc[];  // [slab][quantity][bin], integer units
    STAMP(0);
    const int nthreads = blockDim.x;
    int c = 0;
    const int bid = blockIdx.x;
    while (c + 1 < a.n_cont && bid >= a.blk_start[c + 1]) c++;  // workgroup-uniform
    const ContDev &C = a.cont[c];
    const int64_t lb = bid - a.blk_start[c];
    const int n_bins = (int)a.n_bins;
    const int n_acc = NL * 2 * n_bins;
    // replica used by this lane: neighbouring lanes (neighbouring, i.e. correlated,
    // events) add into different copies, which cuts same-address serialisation
    unsigned long long *my_acc = s_acc + (int)(threadIdx.x & (a.copies - 1)) * n_acc;
    unsigned long long *g_out = g_limbs + (int64_t)(a.cont_base + c) * a.n_bins * 2 * NL;
    const int64_t n_wg = a.blk_start[c + 1] - a.blk_start[c];
    const int64_t q_end = (C.n + 3) >> 2;   // quads of events (columns padded to whole blocks of 64 quads)
    // The wavefronts of the container's workgroups take the listed blocks (ContDev::dep_blocks)
    // round robin -- wavefront wv of workgroup lb the ordinals wv n_wg + lb + i W n_wg (W wavefronts per workgroup),
    // ordinal o standing for block dep[o] & 0x7fffffff.  The list's last, partial round (n_dep mod W n_wg blocks) is
    // thereby dealt ACROSS the workgroups, wavefront 0 of every workgroup first: a workgroup has one or two wavefronts
    // with a sweep more than the others, which they run on an otherwise idle CU.  (Dealt lb W + wv, the first few
    // workgroups of a container took that round with all sixteen wavefronts and finished 3-6 us after every other
    // workgroup of the launch: in-kernel stamps, EXPERIMENTS R14-1.)  The
    // list entry (block number, and in bit 31 the plan's mark "holds an event that deposits nothing") is one scalar
    // load per sweep (the list is written once, by the plan: constant address space), fetched a sweep ahead of the
    // column loads that need it.  Ordinal and entries are wave-uniform values in scalar registers: a wavefront sweeps
    // whole blocks (both columns are padded to whole blocks), so the sweep loop has no per-lane exit.
    typedef const uint32_t __attribute__((address_space(4))) *dep_list;
    const dep_list dep = (dep_list)C.dep_blocks;
    const int o_step = (int)n_wg * (nthreads >> 6);
    const int n_dep = C.n_dep;
    int o = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6) * (int)n_wg + (int)lb);
    uint32_t ent = 0, ent_next = 0;
    uint4 qx = make_uint4(~0u, ~0u, ~0u, ~0u);
    const double2 none2 = make_double2(0.0, 0.0);
    double2 g0 = none2, g1 = none2;
    bool qhave = o < n_dep;
    if (qhave) {
        const int last = n_dep - 1;
        ent = dep[o];
        ent_next = dep[o + o_step < last ? o + o_step : last];
        const int64_t blk = ent & 0x7fffffffu;
        qx = reinterpret_cast<const uint4 *>(C.idx16)[blk * 64 + (threadIdx.x & 63)];
        const double2 *gq = C.wflux_q + (blk * 256 + (threadIdx.x & 63));
        g0 = gq[0]; g1 = gq[64];
    }

    STAMP(1);
    for (int k = threadIdx.x; k < n_acc * a.copies; k += nthreads) s_acc[k] = 0ull;
    __syncthreads();
    bool bad = false;
    STAMP(2);

    const int bin_lo = 0;
    const DepositTarget<true, true> accumulate{my_acc, n_bins, bin_lo, g_out, a.opts, bad};

    // The 16-bit index sweep with what a planned launch knows taken out of the instruction stream.
    //  * A block the plan did not mark holds 256 events that all deposit (node and bin valid, none beyond the
    //    container's end): no 0xffff selects.  A marked block (the topped-up last one, a block with an event outside
    //    the calc grid or the binning) runs the guarded body with the shared `accumulate`.  The mark is bit 31 of the
    //    list entry: a scalar, wave-uniform choice.
    //  * The wavefront classifies the two weights of a half-sweep ONCE: 2^-26 <= w < 2^38 makes w and w*w both `fast`
    //    in the sense of deposit_units (w*w is then in [2^-52, 2^76): its rounding cannot reach 2^76), and if that
    //    holds in every lane the four deposits run without a branch.  Otherwise this half-sweep takes `accumulate`,
    //    which deposits the same digits.  (Per half-sweep, not per quad: the flux pairs of events 2, 3 are still in
    //    flight while events 0, 1 deposit -- the load pipeline of the QUAD sweep is kept.)
    //  * One LDS byte address per deposit, slab j: slabs j-1, j-2 lie one and two scalar strides below it.
    const double2 *tab = C.pepmu_own ? C.pepmu_own
                                     : a.pepmu + ((int64_t)C.side * 3 + C.flav) * a.n_nodes;
    const double scale = C.scale;
    const uint4 *idxq = reinterpret_cast<const uint4 *>(C.idx16);
    const double2 *aw = C.wflux_q;
    const double2 zero2 = make_double2(0.0, 0.0);
    const unsigned lane = threadIdx.x & 63;
    const unsigned q_bytes = 8u * (unsigned)n_bins, slab_bytes = 2u * q_bytes;   // [slab][quantity][bin] of 8-byte words
    // byte address of (slab -29, quantity 0, bin 0) of this lane's replica: put_fast counts slabs from there
    const unsigned acc0 = (unsigned)(uintptr_t)(lds_u64)my_acc - 29u * slab_bytes;
    auto both_fast = [](double w) { return ((unsigned)__double2hiint(w) >> 20) - (1023u - 26u) < 64u; };
    // deposit_units' fast case at byte address `at` = (slab -29, quantity, bin): biased exponent + 21 = 32 (j + 29) + sh
    auto put_fast = [&](unsigned at, double x) {
        const unsigned hi = (unsigned)__double2hiint(x) + (21u << 20);
        const unsigned sh = (hi >> 20) & 31u;
        const unsigned long long m =
            ((unsigned long long)((hi & 0xfffffu) | 0x100000u) << 32) | (unsigned)__double2loint(x);
        const unsigned long long low = m << (sh + 12u);
        const unsigned at0 = __umul24(hi >> 25, slab_bytes) + at;
        lds_add_at(at0, m >> (52u - sh));
        lds_add_at(at0 - slab_bytes, low >> 32);
        lds_add_at(at0 - 2u * slab_bytes, low & 0xffffffffull);
    };
    int64_t blk = ent & 0x7fffffffu;
    // one block of 256 events: blk_n = the block whose first loads are issued half-way (the last sweep re-reads its own)
    auto sweep = [&](auto guard, int64_t blk_n) {
        constexpr bool GUARD = decltype(guard)::value;
        uint4 x = qx;
        if (GUARD && blk * 64 + lane >= q_end) x = make_uint4(~0u, ~0u, ~0u, ~0u);   // (beyond the container's last quad)
        auto half = [&](unsigned xa, unsigned xb, double2 ga, double2 gb, double2 pa, double2 pb) {
            unsigned ba = xa >> 16, bb = xb >> 16;
            if (GUARD) {
                if ((xa & 0xffffu) == 0xffffu) pa = zero2;
                if ((xb & 0xffffu) == 0xffffu) pb = zero2;
            }
            double wa = weight_compact(ga.x, ga.y, pa.x, pa.y, scale);
            double wb = weight_compact(gb.x, gb.y, pb.x, pb.y, scale);
            if (GUARD) {
                if (ba == 0xffffu) { wa = 0.0; ba = 0; }
                if (bb == 0xffffu) { wb = 0.0; bb = 0; }
                accumulate((int)ba, wa, wa * wa);
                accumulate((int)bb, wb, wb * wb);
                return;
            }
            bool fast = both_fast(wa) && both_fast(wb);
#ifdef PISA_DEV_PROBES
            fast = fast && !(a.opts & 2);
#endif
            if (__all(fast)) {
                const unsigned ata = acc0 + 8u * ba, atb = acc0 + 8u * bb;
                put_fast(ata, wa); put_fast(ata + q_bytes, wa * wa);
                put_fast(atb, wb); put_fast(atb + q_bytes, wb * wb);
            } else {
                accumulate((int)ba, wa, wa * wa);
                accumulate((int)bb, wb, wb * wb);
            }
        };
        auto gather = [&](unsigned w) {
            const unsigned n = w & 0xffffu;
            return tab[GUARD && n == 0xffffu ? 0u : n];
        };
        const double2 *gq = aw + (blk * 256 + lane);   // lane-contiguous 16-B loads
        const double2 p0 = gather(x.x), p1 = gather(x.y);
        const double2 g2 = gq[128], g3 = gq[192];
        half(x.x, x.y, g0, g1, p0, p1);
        const double2 p2 = gather(x.z), p3 = gather(x.w);
        const uint4 qxn = idxq[blk_n * 64 + lane];
        const double2 *gn = aw + (blk_n * 256 + lane);
        const double2 g0n = gn[0], g1n = gn[64];
        half(x.z, x.w, g2, g3, p2, p3);
        qx = qxn; g0 = g0n; g1 = g1n;
    };
    while (qhave) {   // (wave-uniform)
        const int o_next = o + o_step, last = n_dep - 1;
        const bool have_n = o_next < n_dep;
        const int64_t blk_n = have_n ? (int64_t)(ent_next & 0x7fffffffu) : blk;
        const uint32_t ent_nn = dep[o_next + o_step < last ? o_next + o_step : last];
        if (ent >> 31) sweep(std::true_type{}, blk_n);
        else sweep(std::false_type{}, blk_n);
        blk = blk_n; ent = ent_next; ent_next = ent_nn;
        o = o_next;
        qhave = have_n;
    }
    if (bad && status) atomicOr(status, 1);
    STAMP(3);

#ifdef PISA_DEV_PROBES
    if (a.opts & 4) return;
#endif
    __syncthreads();
    STAMP(4);
    // (the general kernel's flush, spelled as there: the compiler's output for the whole kernel follows this expression)
    flush_window(my_acc == s_acc || a.copies > 1 ? s_acc : s_acc + n_acc, a.copies, n_bins, n_acc, flush_rotation(lb, n_acc), nthreads,
                 [&](int g, int bin, unsigned long long v) { if (bin < (int)a.n_bins) atomicAdd(&g_out[g], v); });
    STAMP(5);
}

// marks[b] bit 0 = block b of 256 events holds an event whose bin half is not 0xffff (the multi-point kernel's `any_in`:
// the bin alone -- an event inside the binning but outside the calc grid still forms its product); bit 1 = it holds an
// event that needs a guard in the sweep: a half that is 0xffff, or a position beyond the container's n events
__global__ void __launch_bounds__(256)
hist_plan_mark_kernel(const uint32_t *__restrict__ idx16, int64_t n, uint8_t *__restrict__ marks) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = idx16[e];   // (the column is padded to whole blocks)
    const int any = __syncthreads_or((v >> 16) != 0xffffu);
    const int idle = __syncthreads_or((v >> 16) == 0xffffu || (v & 0xffffu) == 0xffffu || e >= n);
    if (threadIdx.x == 0) marks[blockIdx.x] = (uint8_t)((any != 0) | ((idle != 0) << 1));
}

// the numbers of the blocks with bit 0 set, ascending (bit 1 of the mark in bit 31 of the entry), and their count: one
// workgroup, every thread a contiguous run of blocks
__global__ void __launch_bounds__(1024)
hist_plan_compact_kernel(const uint8_t *__restrict__ marks, int32_t n_blocks, int32_t *__restrict__ list,
                         int32_t *__restrict__ count) {
    __shared__ int s_cnt[1024];
    const int t = threadIdx.x;
    const int per = (n_blocks + 1023) / 1024;
    const int lo = t * per < n_blocks ? t * per : n_blocks;
    const int hi = lo + per < n_blocks ? lo + per : n_blocks;
    int cnt = 0;
    for (int b = lo; b < hi; b++) cnt += marks[b] & 1;
    s_cnt[t] = cnt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {   // inclusive scan
        const int v = t >= d ? s_cnt[t - d] : 0;
        __syncthreads();
        s_cnt[t] += v;
        __syncthreads();
    }
    int pos = s_cnt[t] - cnt;
    for (int b = lo; b < hi; b++)
        if (marks[b] & 1) list[pos++] = (int32_t)((uint32_t)b | ((uint32_t)(marks[b] & 2) << 30));
    if (t == 1023) *count = s_cnt[1023];
}

}  // namespace pisa

using namespace pisa;

#ifdef PISA_HIST_STAMPS
PISA_API int pisa_hip_debug_hist_stamps(unsigned long long *h_out) {
    return check_hip(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_hist_stamps), sizeof(g_hist_stamps)), "stamps");
}
#endif

PISA_API int pisa_hip_hist_plan_destroy(pisa_hip_hist_plan *plan) {
    if (!plan) return PISA_HIP_OK;
    if (plan->d_lists) (void)hipFree(plan->d_lists);   // (waits for the launches that still read it)
    delete plan;
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_hist_plan_create(const pisa_hip_container *h_containers, int32_t n_containers,
                                       const pisa_hip_binning *h_calc_grid, const pisa_hip_binning *h_out_binning,
                                       pisa_hip_hist_plan **out, void *stream) {
    if (!out) return PISA_HIP_ERR_INVALID;
    *out = nullptr;
    if (!h_containers || n_containers < 1 || n_containers > 1024) return PISA_HIP_ERR_INVALID;
    DevBinning grid, outb;
    int64_t n_nodes, n_bins;
    int rc = make_dev_binning(h_calc_grid, grid, n_nodes);
    if (rc) return rc;
    if (grid.ndim > 2) return PISA_HIP_ERR_INVALID;
    if ((rc = make_dev_binning(h_out_binning, outb, n_bins))) return rc;
    // where reweight_hist_impl chooses MODE 7 and run_hist no window: 16-bit indices for every container with
    // events, all accumulators in LDS
    if (!(n_nodes < 0xffff && n_bins < 0xffff) || lds_acc_bytes(n_bins) > LDS_ACC_BYTES_MAX) return PISA_HIP_OK;
    int64_t total = 0;
    for (int c = 0; c < n_containers; c++) {
        const pisa_hip_container &h = h_containers[c];
        if (h.n_events < 0 || h.n_events > (1LL << 38)) return PISA_HIP_ERR_INVALID;
        if (h.n_events > 0 && !(h.d_node_bin16 && h.d_weighted_flux_q)) return PISA_HIP_OK;
        total += (h.n_events + 255) / 256;
    }
    if (total >= (1LL << 31)) return PISA_HIP_ERR_INVALID;
    pisa_hip_hist_plan *p = new pisa_hip_hist_plan();
    p->n_cont = n_containers;
    p->threads = hist_threads();
    p->n_nodes = n_nodes;
    p->n_bins = n_bins;
    p->n_events.resize(n_containers);
    p->n_blocks.resize(n_containers);
    p->n_dep.assign(n_containers, 0);
    p->list.assign(n_containers, nullptr);
    p->offset.resize(n_containers);
    // one allocation: int32 lists[total] | int32 counts[n_containers] | uint8 marks[total]
    const size_t bytes = (size_t)(total + n_containers) * 4 + (size_t)total;
    hipStream_t s = as_stream(stream);
    auto fail = [&](int code) { pisa_hip_hist_plan_destroy(p); return code; };
    if ((rc = check_hip(hipMalloc((void **)&p->d_lists, bytes), "hipMalloc"))) return fail(rc);
    int32_t *d_counts = p->d_lists + total;
    uint8_t *d_marks = reinterpret_cast<uint8_t *>(d_counts + n_containers);
    if ((rc = check_hip(hipMemsetAsync(d_counts, 0, (size_t)n_containers * 4, s), "hipMemsetAsync"))) return fail(rc);
    int64_t at = 0;
    for (int c = 0; c < n_containers; c++) {
        const pisa_hip_container &h = h_containers[c];
        const int32_t nb = (int32_t)((h.n_events + 255) / 256);
        p->n_events[c] = h.n_events;
        p->n_blocks[c] = nb;
        p->offset[c] = at;
        if (nb > 0) {
            hipLaunchKernelGGL(hist_plan_mark_kernel, dim3((unsigned)nb), dim3(256), 0, s, h.d_node_bin16, h.n_events, d_marks + at);
            hipLaunchKernelGGL(hist_plan_compact_kernel, dim3(1), dim3(1024), 0, s, d_marks + at, nb, p->d_lists + at,
                               d_counts + c);
        }
        at += nb;
    }
    if ((rc = check_hip(hipGetLastError(), "hist_plan kernels"))) return fail(rc);
    if ((rc = check_hip(hipMemcpyAsync(p->n_dep.data(), d_counts, (size_t)n_containers * 4, hipMemcpyDeviceToHost, s),
                        "hipMemcpyAsync"))) return fail(rc);
    if ((rc = check_hip(hipStreamSynchronize(s), "hipStreamSynchronize"))) return fail(rc);
    // the work split, once: plan_blocks on the DEPOSITING events of every container (a container without any gets no
    // workgroup, the others at least one sweep per workgroup and together one workgroup per CU)
    for (int base = 0; base < n_containers; base += MAX_CONT) {
        const int nc = n_containers - base < MAX_CONT ? n_containers - base : MAX_CONT;
        int64_t nev[MAX_CONT], chunk = 0;
        int32_t blk_start[MAX_CONT + 1] = {0};
        for (int c = 0; c < nc; c++) {
            if (p->n_dep[base + c] < 0 || p->n_dep[base + c] > p->n_blocks[base + c]) return fail(PISA_HIP_ERR_HIP);
            nev[c] = 256 * (int64_t)p->n_dep[base + c];
            p->list[base + c] = p->n_dep[base + c] > 0 ? p->d_lists + p->offset[base + c] : nullptr;   // (none: no workgroup)
        }
        plan_blocks(nev, nc, p->threads, chunk, blk_start);
        for (int c = nc; c < MAX_CONT; c++) blk_start[c + 1] = blk_start[nc];
        p->blk_start.insert(p->blk_start.end(), blk_start, blk_start + MAX_CONT + 1);
        p->chunk.push_back(chunk);
    }
    *out = p;
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_hist_plan_info(const pisa_hip_hist_plan *plan, int32_t container, int32_t *n_blocks,
                                     int32_t *n_dep_blocks, int32_t *workgroups, int32_t *h_dep_blocks) {
    if (!plan || container < 0 || container >= plan->n_cont) return PISA_HIP_ERR_INVALID;
    const int32_t *bs = plan->blk_start.data() + (size_t)(container / MAX_CONT) * (MAX_CONT + 1) + container % MAX_CONT;
    if (n_blocks) *n_blocks = plan->n_blocks[container];
    if (n_dep_blocks) *n_dep_blocks = plan->n_dep[container];
    if (workgroups) *workgroups = bs[1] - bs[0];
    if (h_dep_blocks && plan->n_dep[container] > 0) {
        PISA_TRY_HIP(hipMemcpy(h_dep_blocks, plan->list[container], (size_t)plan->n_dep[container] * 4, hipMemcpyDeviceToHost));
        for (int32_t b = 0; b < plan->n_dep[container]; b++) h_dep_blocks[b] &= 0x7fffffff;   // (bit 31: the sweep's mark)
    }
    return PISA_HIP_OK;
}

PISA_API int pisa_hip_reweight_hist_planned(const pisa_hip_hist_plan *plan, const pisa_hip_container *h_containers,
                                            int32_t n_containers, const pisa_hip_binning *h_calc_grid,
                                            const double *d_prob_nu, const double *d_prob_nubar, const double *d_pepmu,
                                            const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                                            int32_t *d_status, int32_t clear_first, void *stream) {
    if (!plan || !h_containers || n_containers != plan->n_cont || !d_limbs) return PISA_HIP_ERR_INVALID;
    // a plan stands for the 16-bit index form of exactly these containers on this grid and binning
    DevBinning grid, outb;
    int64_t n_nodes, n_bins;
    int rc = make_dev_binning(h_calc_grid, grid, n_nodes);
    if (rc) return rc;
    if (grid.ndim > 2) return PISA_HIP_ERR_INVALID;
    if ((rc = make_dev_binning(h_out_binning, outb, n_bins))) return rc;
    if (n_nodes != plan->n_nodes || n_bins != plan->n_bins) return PISA_HIP_ERR_INVALID;
    bool any_table = d_pepmu != nullptr;   // (none at all is refused even where no container has events, as by pisa_hip_reweight_hist)
    for (int c = 0; c < n_containers; c++) {
        const pisa_hip_container &h = h_containers[c];
        if (h.n_events != plan->n_events[c] || h.n_events < 0 || h.flav < 0 || h.flav > 2 || (h.nubar != 1 && h.nubar != -1))
            return PISA_HIP_ERR_INVALID;
        if (h.n_events > 0 && !(h.d_node_bin16 && h.d_weighted_flux_q && (d_pepmu || h.d_pepmu))) return PISA_HIP_ERR_INVALID;
        any_table = any_table || h.d_pepmu;
    }
    if (!any_table) return PISA_HIP_ERR_INVALID;
    // two replicas of the LDS accumulators where they fit (run_hist, hist.hip)
    const int64_t lds_bytes = lds_acc_bytes(n_bins);
    const int copies = hist_copies(PISA_DEV_INT("HIST_COPIES", 2), lds_bytes);
    hipStream_t s = as_stream(stream);
    if (clear_first) PISA_TRY_HIP(hipMemsetAsync(d_limbs, 0, (size_t)n_containers * n_bins * 2 * NL * 8, s));
    for (int base = 0; base < n_containers; base += MAX_CONT) {
        const int nc = n_containers - base < MAX_CONT ? n_containers - base : MAX_CONT;
        HistArgs a = {};   // (the fields of the general forms stay zero: no window, no partitions)
        a.n_cont = nc;
        a.cont_base = base;
        a.n_bins = n_bins;
        a.n_nodes = n_nodes;
        a.pepmu = reinterpret_cast<const double2 *>(d_pepmu);
        a.copies = copies;
        a.opts = PISA_DEV_INT("HIST_DBG", 0) & ~1;
        for (int c = 0; c < nc; c++) {
            const pisa_hip_container &h = h_containers[base + c];
            ContDev &d = a.cont[c];
            d.n = h.n_events;
            d.pepmu_own = reinterpret_cast<const double2 *>(h.d_pepmu);
            d.idx16 = h.d_node_bin16;
            d.wflux_q = reinterpret_cast<const double2 *>(h.d_weighted_flux_q);
            d.scale = h.scale;
            d.flav = h.flav;
            d.side = h.nubar > 0 ? 0 : 1;
            d.dep_blocks = plan->list[base + c];
            d.n_dep = plan->n_dep[base + c];
        }
        // the split made with the plan, from the depositing blocks of every container
        const int32_t *bs = plan->blk_start.data() + (size_t)(base / MAX_CONT) * (MAX_CONT + 1);
        for (int c = 0; c <= MAX_CONT; c++) a.blk_start[c] = bs[c];
        a.chunk = plan->chunk[base / MAX_CONT];
        if (a.blk_start[nc] <= 0) continue;
        if (g_prof_start) PISA_TRY_HIP(hipEventRecord(g_prof_start, s));
        hipLaunchKernelGGL(hist_planned_kernel, dim3((unsigned)a.blk_start[nc]), dim3(plan->threads),
                           (size_t)lds_bytes * copies, s, a, reinterpret_cast<unsigned long long *>(d_limbs), d_status);
        PISA_CHECK_LAUNCH("hist_planned_kernel");
        if (g_prof_stop) PISA_TRY_HIP(hipEventRecord(g_prof_stop, s));
    }
    return PISA_HIP_OK;
}
