// Process-wide host state that every unit of the library reads: the testing knobs (written by bmx_dev_set, abi.hip), the
// BMX_DEBUG switches and the wait with a deadline.  A unit of its own rather than a corner of abi.hip: the watchdog wait
// belongs to no entry point, and abi.hip is the largest host unit already.  No kernel here.
#include "bmx_common.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace bmx {

DevKnobs& dev_knobs() {
    static DevKnobs k;
    return k;
}

bool debug_prints() {  // BMX_DEBUG=1: the shape decisions of every search (slow: lists are copied back for their counts)
    static const bool on = std::getenv("BMX_DEBUG") != nullptr && std::getenv("BMX_DEBUG")[0] != 't';
    return on;
}

bool debug_timings() {  // BMX_DEBUG=t (or 1): host-side timings of the one-shot call
    static const bool on = std::getenv("BMX_DEBUG") != nullptr;
    return on;
}

void guarded_stream_sync(hipStream_t stream, double budget_s) {
    if (!(budget_s > 0.0)) {
        BMX_HIP(hipStreamSynchronize(stream));
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(stream);
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) {
            (void)hipGetLastError();
            throw Error(BMX_ERR_HIP, std::string("hipStreamQuery failed: ") + hipGetErrorString(e));
        }
        (void)hipGetLastError();  // hipErrorNotReady is sticky for hipGetLastError otherwise
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el > budget_s) {
            char msg[200];
            std::snprintf(msg, sizeof(msg),
                          "watchdog: the GPU work queued on the engine's stream did not finish within %.1f s; the engine is "
                          "dead (restart the process)", budget_s);
            throw WatchdogTimeout(msg);
        }
        if (el > 2e-3) std::this_thread::sleep_for(std::chrono::microseconds(100));  // short waits spin, long ones sleep
    }
}

}  // namespace bmx
