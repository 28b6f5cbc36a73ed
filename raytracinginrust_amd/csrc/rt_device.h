// csrc/rt_device.h — owners of the host library's device resources (rt_host.cpp, rt_multi.cpp): plain C++ over the HIP runtime API, no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_scene.h"
#include "rt_launch.h"

namespace rt {
// Events and counter blocks belong to one device: waits, elapsed times and copies run with that device current.  DeviceGuard(d) makes d
// current for a scope and restores the caller's device only if it switched; DeviceGuard() is for a scope that goes from device to device
// itself: it restores the caller's device whatever the scope left current.
struct DeviceGuard {
    int prev = -1; bool switched = false;
    DeviceGuard() { switched = hipGetDevice(&prev) == hipSuccess; }
    explicit DeviceGuard(int device) { if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess; }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
// A device allocation that lives for one call (move-only): allocated on the current device, freed when it leaves scope — with the device
// that is current then, so it is declared after the DeviceGuard it depends on.
class DeviceBuffer {
    void* p = nullptr;
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.release()) {}
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { const hipError_t e = hipMalloc(&p, bytes); if (e != hipSuccess) p = nullptr; return e; }     // once per buffer
    void* get() const { return p; }
    void* release() { void* q = p; p = nullptr; return q; }
};
// What a launch needs from its slot: the queue word, the counter block and the two events, created on the current device on first use.
inline hipError_t ensure_slot_resources(Scene::LaunchSlot& l) {
    hipError_t e = hipSuccess;
    if (!l.d_queue) e = hipMalloc(&l.d_queue, 64);
    if (e == hipSuccess && !l.d_stats) e = hipMalloc(&l.d_stats, RT_STATS_BYTES);
    if (e == hipSuccess && !l.ev_start) { hipEvent_t ev; if ((e = hipEventCreate(&ev)) == hipSuccess) l.ev_start = ev; }
    if (e == hipSuccess && !l.ev_stop) { hipEvent_t ev; if ((e = hipEventCreate(&ev)) == hipSuccess) l.ev_stop = ev; }
    return e;
}
} // namespace rt
