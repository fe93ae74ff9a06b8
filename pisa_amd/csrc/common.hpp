// common.hpp -- shared host-side helpers of libpisa_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pisa_hip.h"

#define PISA_API extern "C" __attribute__((visibility("default")))

namespace pisa {

void set_last_hip_error(hipError_t e, const char *what);

inline int check_hip(hipError_t e, const char *what) {
    if (e != hipSuccess) {
        set_last_hip_error(e, what);
        return PISA_HIP_ERR_HIP;
    }
    return PISA_HIP_OK;
}

#define PISA_TRY_HIP(expr)                                       \
    do {                                                         \
        int _rc = ::pisa::check_hip((expr), #expr);              \
        if (_rc != PISA_HIP_OK) return _rc;                      \
    } while (0)

#define PISA_CHECK_LAUNCH(name)                                  \
    do {                                                         \
        int _rc = ::pisa::check_hip(hipGetLastError(), name);    \
        if (_rc != PISA_HIP_OK) return _rc;                      \
    } while (0)

// Development probes.  The product library reads NO environment variable and has no switch that makes a kernel do
// less work: every run-time selection of a kernel form or launch shape (tests/dev_cases.py, scripts/dev/*) exists
// only in the development library (`make dev`: -DPISA_DEV_PROBES).  In the default build PISA_DEV_INT(name, dflt) is
// the constant `dflt` (the name never reaches the binary: tests/test_abi.py checks `strings libpisa_hip.so`).
// A switch is kept only while a test or a kept script sets it: a form that nothing selects is deleted, not switched off.
#ifdef PISA_DEV_PROBES
#include <stdlib.h>
inline long long dev_env_ll(const char *name, long long dflt) {
    const char *v = getenv(name);
    return v ? atoll(v) : dflt;
}
inline const char *dev_env_str(const char *name) { return getenv(name); }
#define PISA_DEV_INT(name, dflt) ((int)::pisa::dev_env_ll("PISA_HIP_" name, (dflt)))
#define PISA_DEV_LL(name, dflt) (::pisa::dev_env_ll("PISA_HIP_" name, (dflt)))
#define PISA_DEV_STR(name) (::pisa::dev_env_str("PISA_HIP_" name))
#else
#define PISA_DEV_INT(name, dflt) ((int)(dflt))
#define PISA_DEV_LL(name, dflt) ((long long)(dflt))
#define PISA_DEV_STR(name) ((const char *)nullptr)
#endif

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// A device buffer of doubles that grows on demand and never shrinks: the scratch of an entry point between its
// launches.  An instance is a file's static, one per process: calls that use it on different streams must not
// overlap.  Instances stay apart, so calls into different entry points share no memory.
struct DeviceScratch {
    double *ptr = nullptr;
    int64_t doubles = 0;
    int reserve(int64_t n, double **w) {
        if (n > doubles) {
            if (ptr) (void)hipFree(ptr);   // (waits for the launches that still read it)
            ptr = nullptr;
            doubles = 0;
            PISA_TRY_HIP(hipMalloc(&ptr, (size_t)n * sizeof(double)));
            doubles = n;
        }
        *w = ptr;
        return PISA_HIP_OK;
    }
};

// a run-time value as a template argument: f(std::integral_constant<int, V>) for the V that equals `value`, the
// last V where none does (callers check the range first)
template <int V0, int... Vs, class F>
inline int dispatch_int(int value, F &&f) {
    if constexpr (sizeof...(Vs) == 0)
        return f(std::integral_constant<int, V0>{});
    else
        return value == V0 ? f(std::integral_constant<int, V0>{}) : dispatch_int<Vs...>(value, f);
}

// Regular (linear, equal-width) binning as the kernels see it
// (fast_histogram rule / translation.py:417-456): bin = (int)((x - min) * norm)
struct DevBinning {
    int32_t ndim;
    int32_t nb[3];
    double mins[3];
    double maxs[3];
    double norm[3];
};

inline int make_dev_binning(const pisa_hip_binning *b, DevBinning &d, int64_t &total) {
    if (!b || b->ndim < 1 || b->ndim > PISA_HIP_MAX_DIMS) return PISA_HIP_ERR_INVALID;
    d.ndim = b->ndim;
    total = 1;
    for (int k = 0; k < 3; k++) {
        d.nb[k] = 1; d.mins[k] = 0; d.maxs[k] = 1; d.norm[k] = 1;
    }
    for (int k = 0; k < b->ndim; k++) {
        if (b->nbins[k] < 1 || b->nbins[k] > (1 << 24) || !(b->maxs[k] > b->mins[k]))
            return PISA_HIP_ERR_INVALID;
        d.nb[k] = (int32_t)b->nbins[k];
        d.mins[k] = b->mins[k];
        d.maxs[k] = b->maxs[k];
        // normx = nx / (xmax - xmin)   (translation.py:419; fast_histogram)
        d.norm[k] = (double)b->nbins[k] / (b->maxs[k] - b->mins[k]);
        total *= b->nbins[k];
    }
    return PISA_HIP_OK;
}

}  // namespace pisa
