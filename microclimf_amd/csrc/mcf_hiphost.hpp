// mcf_hiphost.hpp — host only: what every unit with HIP host code shares (mcf_api.hip, mcf_snow.hip, mcf_terrain.hip,
// mcf_hydro.hip): the error macro, the owner of device allocations, and the device -> host copy of results.
// Included after mcf_rowblocks.hpp, which declares mcf::api_fail.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "mcf_hostpipe.hpp"
#include "mcf_rowblocks.hpp"

// a failed HIP call leaves the function with the library's error code and "<expr> failed: <hip string> (<file>:<line>)"
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            char b_[512];                                                                      \
            snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),     \
                     __FILE__, __LINE__);                                                      \
            return mcf::api_fail(e_ == hipErrorOutOfMemory ? MCF_ERR_NOMEM : MCF_ERR_HIP, b_); \
        }                                                                                      \
    } while (0)

namespace mcf {

// hipMalloc with the library's error (n <= 0: 8 bytes, so that every buffer has an address)
inline int dev_malloc(void** out, int64_t n) {
    hipError_t e = hipMalloc(out, (size_t)(n <= 0 ? 8 : n));
    if (e == hipSuccess) return MCF_OK;
    char b[256];
    snprintf(b, sizeof b, "hipMalloc(%lld bytes) failed: %s", (long long)(n <= 0 ? 8 : n), hipGetErrorString(e));
    return api_fail(MCF_ERR_NOMEM, b);
}

// Device allocations that are released together, when their owner goes: a call's scratch buffers, a plan's buffers.
struct DevOwner {
    std::vector<std::pair<void*, int64_t>> p;      // (buffer, bytes)
    int64_t bytes = 0;                             // what the owner holds now
    DevOwner() = default;
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { release_all(); }
    int alloc(void** out, int64_t n) {
        if (n <= 0) n = 8;
        if (const int rc = dev_malloc(out, n)) return rc;
        p.emplace_back(*out, n);
        bytes += n;
        return MCF_OK;
    }
    // one buffer ahead of the others (a buffer that grows)
    void release(void* q) {
        for (size_t i = 0; i < p.size(); ++i)
            if (p[i].first == q) {
                (void)hipFree(q);
                bytes -= p[i].second;
                p.erase(p.begin() + (long)i);
                return;
            }
    }
    void release_all() {
        for (auto& q : p) (void)hipFree(q.first);
        p.clear();
        bytes = 0;
    }
    // `n` elements of T (T may be const: a buffer its holder only reads)
    template <class T>
    int make(T** out, int64_t n) { return alloc((void**)out, n * (int64_t)sizeof(T)); }
    // a buffer of `n` elements that grows (*cap: its bytes): the old one is released first.  A buffer that has to grow gets a quarter
    // more than is asked for — successive calls ask for about the same, and a release + allocation of a gigabyte costs 50 ms
    template <class T>
    int regrow(T** buf, int64_t* cap, int64_t n) {
        int64_t nbytes = n * (int64_t)sizeof(T);
        if (*buf && *cap >= nbytes) return MCF_OK;
        if (*buf) { nbytes += nbytes / 4; release((void*)*buf); *buf = nullptr; *cap = 0; }
        const int rc = alloc((void**)buf, nbytes);
        if (!rc) *cap = nbytes > 8 ? nbytes : 8;
        return rc;
    }
    // device copy of a host array of `n` elements: one the device goes on to write ...
    template <class T>
    int up_mut(T** dev, const T* host, int64_t n, const char* what) {
        if (!host) return api_fail(MCF_ERR_ARG, std::string("null input: ") + what);
        T* d;
        if (const int rc = make(&d, n)) return rc;
        hipError_t e = hipMemcpy(d, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return api_fail(MCF_ERR_HIP, std::string("upload failed: ") + what);
        *dev = d;
        return MCF_OK;
    }
    // ... and one it only reads
    template <class T>
    int up(const T** dev, const T* host, int64_t n, const char* what) { return up_mut(const_cast<T**>(dev), host, n, what); }
};

// Device -> caller-owned pageable memory.  Results of 64 MiB and more go through the pinned ring + copy threads of
// mcf_hostpipe.hpp (set up at the first such copy; MCF_NO_HOSTPIPE switches them off), smaller ones and every copy after a failed
// set-up through hipMemcpy.  How the copy knows that the producer has finished is the caller's: with `stream`, an event
// recorded on it is handed to the pipe, and the plain copy is hipMemcpyAsync + a synchronise of that stream; without one the
// producers ran on the null stream: the device is synchronised before the pipe, and the plain copy is the blocking one.
struct ToHost {
    HostPipe pipe;
    hipEvent_t ev = nullptr;
    bool tried = false, ok = false;
    ~ToHost() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t dense(void* dst, const void* dev, size_t bytes, hipStream_t stream = nullptr) {
        if (piped(bytes, 0, stream)) {
            hipError_t e = producer_done(stream);
            return e != hipSuccess ? e : pipe.copy(dst, dev, bytes, stream ? ev : nullptr);
        }
        if (!stream) return hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost);
        hipError_t e = hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    }
    // rows of `width` bytes, contiguous on the device, `dpitch` bytes apart on the host (a row block of a taller raster)
    hipError_t pitched(void* dst, size_t dpitch, const void* dev, size_t width, size_t height, hipStream_t stream = nullptr) {
        if (piped(width * height, width, stream)) {
            // contiguous DMA into the pinned ring, the scatter by the host copy threads
            hipError_t e = producer_done(stream);
            return e != hipSuccess ? e : pipe.copy_pitched(dst, dpitch, dev, width, height, stream ? ev : nullptr);
        }
        if (!stream) return hipMemcpy2D(dst, dpitch, dev, width, width, height, hipMemcpyDeviceToHost);
        hipError_t e = hipMemcpy2DAsync(dst, dpitch, dev, width, width, height, hipMemcpyDeviceToHost, stream);
        return e != hipSuccess ? e : hipStreamSynchronize(stream);
    }

private:
    bool piped(size_t bytes, size_t width, hipStream_t stream) {
        static const bool no_pipe = getenv("MCF_NO_HOSTPIPE") != nullptr;
        if (bytes < ((size_t)64 << 20) || width > HostPipe::kPiece || no_pipe) return false;
        if (!tried) {
            tried = true;
            ok = pipe.init() && (!stream || hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess);
        }
        return ok;
    }
    hipError_t producer_done(hipStream_t stream) { return stream ? hipEventRecord(ev, stream) : hipDeviceSynchronize(); }
};

}  // namespace mcf
