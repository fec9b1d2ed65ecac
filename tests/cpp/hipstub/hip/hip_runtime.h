// A stand-in for <hip/hip_runtime.h>, for tests/cpp/own_host_main.cpp only: just what
// zig-flac_amd/csrc/fg_own.hpp calls, on host memory.  Every call is counted or logged, and
// fail_at = k makes the k-th hipMalloc from then on fail.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <string>

typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum { hipStreamNonBlocking = 1 };

namespace hipstub {
inline int mallocs = 0, frees = 0, fail_at = 0, made = 0, destroyed = 0;
inline std::string log;  // 's' hipStreamSynchronize, 'f' hipFree of a buffer, 'm' hipMalloc
}

template <class T>
hipError_t hipMalloc(T **p, size_t bytes) {
    hipstub::log += 'm';
    if (hipstub::fail_at && --hipstub::fail_at == 0) return hipErrorOutOfMemory;
    hipstub::mallocs++;
    *p = (T *)std::aligned_alloc(256, (bytes + 255) / 256 * 256);  // aligned like a device allocation
    return hipSuccess;
}
inline hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    hipstub::log += 'f';
    hipstub::frees++;
    std::free(p);
    return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipstub::log += 's', hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return *s = (hipStream_t)(size_t)++hipstub::made, hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return *e = (hipEvent_t)(size_t)++hipstub::made, hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t) { return hipstub::destroyed++, hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t) { return hipstub::destroyed++, hipSuccess; }
