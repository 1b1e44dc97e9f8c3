// A stand-in for <hip/hip_runtime.h> for tests/cpp/own_test.cpp: the eight create / free functions lm_own.h calls (and hipMemcpy), backed by
// malloc and a table of live handles.  stub.fail_at = k makes the k-th create call from now fail; stub.log records 'a' per create and 'f' per
// free, in order; stub.bad counts frees of handles that are not live (a double free, a handle never created).
#pragma once
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
typedef struct StubStream* hipStream_t;
typedef struct StubEvent* hipEvent_t;
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventDisableTiming = 2 };

struct HipStub {
    std::map<void*, char> live;      // handle -> kind: 'd' device, 'p' pinned, 's' stream, 'e' event
    std::string log;
    long calls = 0, fail_at = 0, bad = 0;
    hipError_t create(void** out, char kind, size_t bytes) {
        *out = nullptr;
        if (++calls == fail_at) return hipErrorOutOfMemory;
        *out = std::malloc(bytes ? bytes : 1);
        live[*out] = kind; log += 'a';
        return hipSuccess;
    }
    hipError_t destroy(void* h, char kind) {
        auto it = live.find(h);
        if (it == live.end() || it->second != kind) { ++bad; return hipErrorOutOfMemory; }
        live.erase(it); log += 'f';
        std::free(h);
        return hipSuccess;
    }
    long count(char kind) const { long n = 0; for (const auto& e : live) n += e.second == kind; return n; }
    void arm(long k) { calls = 0; fail_at = k; }
};
inline HipStub stub;

inline hipError_t hipMalloc(void** p, size_t bytes) { return stub.create(p, 'd', bytes); }
inline hipError_t hipFree(void* p) { return stub.destroy(p, 'd'); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub.create(p, 'p', bytes); }
inline hipError_t hipHostFree(void* p) { return stub.destroy(p, 'p'); }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return stub.create(reinterpret_cast<void**>(s), 's', 1); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return stub.create(reinterpret_cast<void**>(s), 's', 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return stub.destroy(s, 's'); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return stub.create(reinterpret_cast<void**>(e), 'e', 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return stub.destroy(e, 'e'); }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
