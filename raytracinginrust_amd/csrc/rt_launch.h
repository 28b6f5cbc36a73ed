// csrc/rt_launch.h — interface between the host library (rt_host.cpp) and the kernels (rt_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "rt_ir.h"

namespace rt {
// Shape of the instantiation that serves a scene: workgroup size, entries of each wave's camera-path queue and their size (80 B; 104 B
// in the lean f64 kernel, whose entries carry beta: lean_f64_queue below), and whether it runs as ONE workgroup per CU (BVH kernels: the
// CU's LDS then holds one copy of the top of the BVH, KParams::n_cached nodes).
struct LaunchShape { uint32_t threads, queue_entries, entry_bytes; bool one_per_cu; };
// The lean f64 kernels' queue (rt_kernel.hip PrimaryPass, trace_shade_fill): a ring of first-hit records per wave, in one of two forms.
// The primary pass runs when fewer than FILL_AT records are queued and generates min(64, QN - queued) camera paths.
// WIDE: 104 B a record — p, n, d as f64; rng, pixel, sample, material, rect | front << 31 —, HIT_RING_QN = 76 records refilled below
// HIT_RING_FILL_AT = 26.  COMPACT: 80 B — the same without n, whose three sign bits ride in bits 28..30 of the rect word —,
// HIT_RING_QN_COMPACT records refilled below HIT_RING_FILL_AT_COMPACT.  The compact form serves the scenes in which every rect has a valid
// entry in the per-face ONB table (HostFlat::onb_all): there the sign-masked words of a hit's normal are the entry's mag[0..2] for every
// ray (rt_kernel.hip: Lemma N above trace_shade_fill), so the normal is rebuilt from the table and three bits.  Every other scene, and
// RT_NO_PRIMARY_PASS, runs the wide kernel.
// The one definition of the constants, for the kernels, for the LDS the host asks for and for lean_f64_queue; -DRT_HIT_RING_QN /
// -DRT_HIT_RING_FILL_AT / -DRT_HIT_RING_QN_COMPACT / -DRT_HIT_RING_FILL_AT_COMPACT: measurement builds of the lean unit
// (tools/ring_sweep.py).
// The constraint on the size: five workgroups per CU.  76 x 104 B x 4 waves = 31 616 B per workgroup keeps them; the frame time says
// that 77 entries (32 032 B) do not, although the occupancy query still answers 5 — which is what an LDS allocation granule of 1280 B
// would give; the granule itself was not read from anywhere.  98 x 80 B x 4 waves = 31 360 B.  The threshold trades popping lanes left
// dry (low) against short passes (high) and was timed on the final build.  Both with their measurements: docs/history.md,
// profiles/r12_ring_step0.log, profiles/r13_ring_step0.log.
#ifndef RT_HIT_RING_QN
#define RT_HIT_RING_QN 76
#endif
#ifndef RT_HIT_RING_FILL_AT
#define RT_HIT_RING_FILL_AT 26
#endif
#ifndef RT_HIT_RING_QN_COMPACT
#define RT_HIT_RING_QN_COMPACT 98
#endif
#ifndef RT_HIT_RING_FILL_AT_COMPACT
#define RT_HIT_RING_FILL_AT_COMPACT 36
#endif
static constexpr uint32_t HIT_RING_QN = RT_HIT_RING_QN, HIT_RING_FILL_AT = RT_HIT_RING_FILL_AT;
static constexpr uint32_t HIT_RING_QN_COMPACT = RT_HIT_RING_QN_COMPACT, HIT_RING_FILL_AT_COMPACT = RT_HIT_RING_FILL_AT_COMPACT;
static constexpr uint32_t HIT_RING_ENTRY_BYTES = 9u * 8u + 8u * 4u;      // p n d as f64; rng, pixel, sample, material, rect | front << 31
static constexpr uint32_t HIT_RING_ENTRY_BYTES_COMPACT = 6u * 8u + 8u * 4u;      // p d as f64; rng, pixel, sample, material, rect | signs of n << 28 | front << 31
static constexpr uint32_t HIT_RING_SIGN_SHIFT = 28u, HIT_RING_RECT_MASK = 0x0FFFFFFFu;      // (a primitive index has 28 bits: rt_kernel.hip HitId)
static constexpr uint32_t hit_ring_qn(bool compact) { return compact ? HIT_RING_QN_COMPACT : HIT_RING_QN; }
static constexpr uint32_t hit_ring_fill_at(bool compact) { return compact ? HIT_RING_FILL_AT_COMPACT : HIT_RING_FILL_AT; }
static constexpr uint32_t hit_ring_entry_bytes(bool compact) { return compact ? HIT_RING_ENTRY_BYTES_COMPACT : HIT_RING_ENTRY_BYTES; }
static_assert(HIT_RING_QN >= 64u && HIT_RING_FILL_AT >= 1u && HIT_RING_FILL_AT <= HIT_RING_QN, "a pass must find room for at least one path");
static_assert(HIT_RING_QN_COMPACT >= 64u && HIT_RING_FILL_AT_COMPACT >= 1u && HIT_RING_FILL_AT_COMPACT <= HIT_RING_QN_COMPACT, "a pass must find room for at least one path");
#ifndef RT_HIT_RING_ANY_SIZE      // (measurement builds that give up the fifth workgroup on purpose: tools/ring_sweep.py's counter runs)
static_assert(HIT_RING_QN * HIT_RING_ENTRY_BYTES * 4u <= 31616u && HIT_RING_QN_COMPACT * HIT_RING_ENTRY_BYTES_COMPACT * 4u <= 31616u,
              "a workgroup's four rings stay within what five workgroups per CU leave");
#endif
// Slot k behind `head` (head < QN, k <= QN): add, compare, subtract — the capacity need be no power of two
template <uint32_t QN = HIT_RING_QN> constexpr uint32_t hit_ring_slot(uint32_t head, uint32_t k) { return head + k >= QN ? head + k - QN : head + k; }
template <uint32_t QN> constexpr bool hit_ring_slot_ok() {
    for (uint32_t h = 0u; h < QN; h++) for (uint32_t k = 0u; k <= QN; k++) if (hit_ring_slot<QN>(h, k) != (h + k) % QN) return false;
    return true;
}
static_assert(hit_ring_slot_ok<HIT_RING_QN>() && hit_ring_slot_ok<HIT_RING_QN_COMPACT>(), "hit_ring_slot is (head + k) mod QN for every head and k, at both capacities");
// Camera paths per refill with RT_NO_PRIMARY_PASS (trace_lockstep's [7][64] f64, [6][64] u32 view of the same LDS): KParams::queue_entries
static constexpr uint32_t LEAN_F64_CAMERA_QN = 64u;
static const uint32_t RT_PARK_BYTES_PER_WAVE = 64u * (9u * 8u + 7u * 4u);
// Defined in the lean translation unit, so that a measurement build of that unit alone brings its own ring sizes to the host's LDS request
void lean_f64_queue(LaunchShape& g, bool compact);
// The two lean f64 kernels (the lean translation unit): pathtrace_kernel<double, 0u> runs the compact ring, pathtrace_wide_ring_kernel<double>
// the wide one — the same loop over another record; two kernels and not two loops in one, which costs spilled registers.  The host
// chooses (rt_host.cpp lean_f64_compact), launches and queries the one it chose.
hipError_t launch_lean_f64(const KParams<double>& P, bool compact, uint32_t n_blocks, size_t shmem, hipStream_t stream);
int occupancy_lean_f64(bool compact, size_t shmem);
LaunchShape pathtrace_shape(uint32_t scene_feats, uint32_t flags);
uint32_t pathtrace_feats(uint32_t scene_feats, uint32_t flags);      // the instantiation's FEATS template argument (its name: rt::pathtrace_kernel<T, FEATSu>)
// Dynamic LDS of one workgroup: [n_cached nodes][waves x queue][waves x stack_depth x 64 dwords]
inline size_t pathtrace_lds_bytes(const LaunchShape& g, uint32_t stack_depth, uint32_t n_cached, size_t node_bytes) {
    const size_t waves = g.threads / 64u;
    return (size_t)n_cached * node_bytes + waves * ((size_t)g.queue_entries * g.entry_bytes + (size_t)stack_depth * 64u * sizeof(uint32_t));
}
// The kernels walk a BVH in the reference's order through the f32 filter nodes (rt_ir.h DFNode, rt_kernel.hip bvh_hit_filt): those are
// then what the LDS node cache holds.  The near-first order (opt-in) keeps the plain nodes.
inline bool filtered_walk(uint32_t effective_flags) { return !(effective_flags & 8u /* RT_NEAR_FIRST_BVH */); }
// Counter block the kernel reports into: RT_STATS_ROWS copies (row = block index mod rows) of RT_STATS_SLOTS 64-bit counters
static const uint32_t RT_STATS_SLOTS = 16u, RT_STATS_ROWS = 32u;
static const size_t RT_STATS_BYTES = (size_t)RT_STATS_SLOTS * RT_STATS_ROWS * sizeof(unsigned long long);
// Launch the persistent path-tracing kernel: n_blocks workgroups of pathtrace_shape().threads threads, `shmem` bytes of dynamic LDS (above).
template <typename T> hipError_t launch_pathtrace(const KParams<T>& P, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream);
// Known-answer access to the list-scene kernels' closest-hit search (rt_debug_list_hit; the kernel lives in the lean translation unit)
hipError_t launch_list_hit_kat(const KParams<double>& P, uint32_t n, const double* d_rays, const double* d_tlim, double* d_out, hipStream_t stream);
// ... and to the search as the primary pass runs it (rt_debug_list_hit_masked): P.flags holds the object mask
hipError_t launch_list_hit_masked_kat(const KParams<double>& P, uint32_t n, const double* d_rays, const double* d_tlim, double* d_out, hipStream_t stream);
// Known-answer access to the per-face ONB memo as the lean f64 kernel's Lambertian arm reads it (rt_debug_onb; the lean translation unit)
hipError_t launch_onb_kat(const KParams<double>& P, uint32_t n, const double* d_rects, const double* d_normals, double* d_out, hipStream_t stream);
// Known-answer access to the compact first-hit record's normal, packed and rebuilt as the lean f64 kernel does it (rt_debug_ring_normal; the lean translation unit)
hipError_t launch_ring_normal_kat(const KParams<double>& P, uint32_t n, const double* d_rays, const double* d_tlim, double* d_out, hipStream_t stream);
// ... and to w = normalized(normal) as that kernel takes it from the table's DOnbW records (rt_debug_ring_w; the lean translation unit)
hipError_t launch_ring_w_kat(const KParams<double>& P, uint32_t n, const double* d_rays, const double* d_tlim, double* d_out, hipStream_t stream);
// The primary pass's object masks (csrc/rt_primary.h; the kernel lives in the lean translation unit): d_pixels == nullptr — one word per
// local pixel of the launch P describes (camera, frame size, tiling), what KParams::pmask points at; otherwise the n pixels (i, j) listed
// (rt_debug_primary_mask)
hipError_t launch_primary_masks(const KParams<double>& P, uint32_t n, const uint32_t* d_pixels, uint32_t* d_out, hipStream_t stream);
// Known-answer access to the lights' pdf_value as the F_ALL | F_NESTED kernels compute it (rt_debug_light_pdf; the "rest" translation unit)
hipError_t launch_light_pdf_kat(const KParams<double>& P, uint32_t n, const double* d_o, const double* d_v, double* d_out, hipStream_t stream);
// Resident blocks per CU for the instantiation that serves `scene_feats`.
template <typename T> int pathtrace_blocks_per_cu(uint32_t scene_feats, uint32_t flags, size_t shmem);
}
