// hist_host.hpp -- host helpers of the accumulate launches (hist.hip, hist_planned.hip): LDS sizes, the work split, the
// profile-event pair.
#pragma once
#include <algorithm>

#include "hist_device.hpp"

namespace pisa {

inline int64_t lds_acc_bytes(int64_t n_bins) { return n_bins * 2 * NL * 8; }

// LDS replicas of accumulators of lds_bytes: the largest power of two up to `want` that LDS_ACC_BYTES_MAX holds
inline int hist_copies(int want, int64_t lds_bytes) {
    while (want > 1 && (want & (want - 1))) want--;
    while (want > 1 && lds_bytes * want > LDS_ACC_BYTES_MAX) want >>= 1;
    return want < 1 ? 1 : want;
}

// Workgroups of an accumulate launch.  ONE 1024-thread workgroup per CU (`target` = the device's CU count unless
// PISA_HIP_HIST_BLOCKS says otherwise), never one more: with two per CU the SIMDs serve the older one first, the
// younger ones finish 6-8 us later on their own at half the chip's request rate (10^7 events: 40.1 -> 37.0 us by
// HIP events; 3 / 4 * 10^7 events beyond the Infinity Cache: 137 -> 111 / 157 -> 144 us), and a handful of workgroups
// beyond what is resident run as a second round after everything else (264 workgroups: 50 us).  The workgroups are
// dealt to the containers so that the largest share of a workgroup is as small as possible (greedy: the next
// workgroup goes to the container with the most events per workgroup), a workgroup gets at least one sweep
// (4 * threads events) and at most 2^28 events (the 64-bit accumulators take 2^31 32-bit digits).
// chunk = the largest share, a whole number of sweeps: the forms that do not sweep together cut the columns by it.
inline int device_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

// LDS a workgroup of the current device may ask for (opt-in limit; 160 KiB on gfx950, 64 KiB on older parts)
inline int64_t device_lds_bytes() {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 64 * 1024;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || v <= 0)
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
            v = 64 * 1024;
    return v;
}

inline int plan_blocks_balanced(const int64_t *n_events, int n_cont, int threads, int64_t target, int64_t &chunk,
                                int32_t *blk_start) {
    const int64_t sweep = 4 * (int64_t)threads, wg_max = 1LL << 28;
    int64_t nwg[MAX_CONT], cap[MAX_CONT], used = 0;
    for (int c = 0; c < n_cont; c++) {
        const int64_t n = n_events[c];
        cap[c] = n > 0 ? (n + sweep - 1) / sweep : 0;
        nwg[c] = n > 0 ? (n + wg_max - 1) / wg_max : 0;
        used += nwg[c];
    }
    while (used < target) {
        int best = -1;
        double most = 0.0;
        for (int c = 0; c < n_cont; c++) {
            if (nwg[c] >= cap[c]) continue;
            const double per = (double)n_events[c] / (double)nwg[c];
            if (per > most) { most = per; best = c; }
        }
        if (best < 0) break;
        nwg[best]++;
        used++;
    }
    chunk = sweep;
    blk_start[0] = 0;
    for (int c = 0; c < n_cont; c++) {
        if (nwg[c] > 0) {
            const int64_t per = (n_events[c] + nwg[c] - 1) / nwg[c];
            chunk = std::max(chunk, ((per + sweep - 1) / sweep) * sweep);
        }
        blk_start[c + 1] = blk_start[c] + (int32_t)nwg[c];
    }
    return blk_start[n_cont];
}

inline int plan_blocks(const int64_t *n_events, int n_cont, int threads, int64_t &chunk,
                       int32_t *blk_start) {
    const int env = PISA_DEV_INT("HIST_BLOCKS", 0);
    const int64_t target = env > 0 ? env : (int64_t)device_cus() * std::max(1, 1024 / threads);
    return plan_blocks_balanced(n_events, n_cont, threads, target, chunk, blk_start);
}

inline int hist_threads() {
    const int threads = PISA_DEV_INT("HIST_THREADS", 1024);
    return threads < 64 || threads > 1024 || (threads & 63) ? HIST_THREADS : threads;
}

// optional hipEvent pair recorded around the accumulate kernel of the next
// hist launch (bench.py measures the dominant kernel with them); set per host thread by pisa_hip_profile_events
inline thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;

}  // namespace pisa
