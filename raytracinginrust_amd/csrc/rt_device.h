// csrc/rt_device.h — owners of the host library's device resources (rt_host.cpp, rt_frames.cpp, rt_multi.cpp): plain C++ over the HIP
// runtime API, no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <cassert>
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
// A device allocation that lives for one call, or as a member for as long as its owner (move-only): allocated on the current device, freed
// when it leaves scope — with the device that is current then, so it is declared after the DeviceGuard it depends on, and an owner is
// deleted inside such a guard's scope (rt_frames.cpp progressive_free).
class DeviceBuffer {
    void* p = nullptr; size_t size = 0;
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : size(o.size) { p = o.release(); }
    ~DeviceBuffer() { reset(); }
    hipError_t alloc(size_t bytes) { const hipError_t e = hipMalloc(&p, bytes); if (e != hipSuccess) p = nullptr; size = p ? bytes : 0; return e; }     // once per buffer
    // a member's form: allocated at the first call, a no-op at every later one (a frame's sizes never change)
    __attribute__((visibility("hidden"))) hipError_t ensure(size_t bytes) { assert(!p || size == bytes); return p ? hipSuccess : alloc(bytes); }
    void* get() const { return p; }
    template <typename T> T* as() const { return (T*)p; }
    void* release() { void* q = p; p = nullptr; size = 0; return q; }
    void reset() { if (p) (void)hipFree(release()); }
};
// An event that lives as long as its owner: created on the current device at first use, destroyed as a DeviceBuffer is freed.
class DeviceEvent {
    hipEvent_t ev = nullptr;
public:
    DeviceEvent() = default;
    DeviceEvent(const DeviceEvent&) = delete;
    ~DeviceEvent() { reset(); }
    hipError_t ensure(unsigned flags) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    hipEvent_t get() const { return ev; }
    void reset() { if (ev) { (void)hipEventDestroy(ev); ev = nullptr; } }
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
