// The one launch path of the kernel files (tmpc_kernels.hip, tmpc_block.hip, tmpc_lp.hip): host side, not seen by tmpc_api.cpp.
// launch_grid is the only place where a launcher differs between the GPU build and the host execution model of tests/wavesim.
#pragma once
#include "tmpc_device.hpp"

#ifndef TMPC_HOST_SIM
#include <map>
#include <mutex>
#include <utility>
#endif

namespace tmpc {

#ifdef TMPC_HOST_SIM
inline unsigned long sim_rendezvous_total = 0;
inline unsigned long sim_rendezvous_count() { return sim_rendezvous_total; }
#else
// More than 64 KiB of dynamic LDS needs the opt-in per kernel function and device.  The size may depend on the problem (the
// wave kernel: rows of dense functionals staged; the LP kernel: the staged H'), so the limit is raised whenever a launch asks
// for more than any before it on this device -- and not otherwise.  Handles may be driven from different host threads: the
// check and the call are one critical section.
inline hipError_t raise_lds_limit(const void *kernel, size_t lds) {
    static std::mutex mutex;
    static std::map<std::pair<const void *, int>, size_t> high_water;
    int device = 0;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> guard(mutex);
    size_t &high = high_water[{kernel, device}];
    if (high >= lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e == hipSuccess) high = lds;
    return e;
}
#endif

// Launches `kernel` on `blocks` workgroups of `threads` threads with `lds` bytes of dynamic LDS.  The arguments are converted
// to the kernel's own parameter types.  tests/wavesim: the grid is workgroup 0 alone, run on the host execution model.
template <class... P, class... A>
hipError_t launch_grid(void (*kernel)(P...), unsigned blocks, unsigned threads, size_t lds, hipStream_t stream, A &&...args) {
#ifdef TMPC_HOST_SIM
    (void)blocks; (void)stream;
    sim::Dim3 bi, gd;
    bi.x = bi.y = bi.z = 0;
    sim_rendezvous_total += sim::run_block(static_cast<int>(threads), lds, bi, gd, [&]() { kernel(static_cast<P>(args)...); });
    return hipSuccess;
#else
    if (const hipError_t e = raise_lds_limit(reinterpret_cast<const void *>(kernel), lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, stream, static_cast<P>(args)...);
    return hipGetLastError();
#endif
}

// The fresh (zero) word of a launch's work counter (WorkCounter, tmpc_device.hpp); the ring is cleared in one piece when it
// has gone round.
inline hipError_t next_word(WorkCounter *wc, hipStream_t stream, unsigned long long **word) {
    if (wc == nullptr || wc->ring == nullptr) return hipErrorInvalidValue;
    if (wc->pos >= wc->size) {
        if (const hipError_t e = hipMemsetAsync(wc->ring, 0, sizeof(unsigned long long) * wc->size, stream); e != hipSuccess) return e;
        wc->pos = 0;
    }
    *word = wc->ring + wc->pos++;
    return hipSuccess;
}

}  // namespace tmpc
