// csrc/rt_adaptive.hip — adaptive progressive frames on the device: the pixel-list path-tracing kernel (rt_render_pixels_device) and the
// element-wise kernels of rt_adaptive.h — error with counts, selection and its compaction, list merge, resolve with counts.
//
// A translation unit of its own over rt_kernel.hip's device functions, as rt_radiance.hip is (RT_TU == 3 leaves that file's kernels and launch
// code out): the bounce loop is radiance_kernel's — world_hit / world_hit_list, finalize_hit, shade_hit, add_radiance, flush_acc, the code the
// frames run — and nothing is added to the units the frames and the moments are built from.  camera_ray, the cursor's path_step, the
// staging loop and the scene-class dispatch are the query units' own: rt_query_dev.h.
//
// PIXELS: path q = k * n_b + s is sample n[list[k]] + s of output-order pixel list[k], one path per lane, pixel-major: the list is ascending,
// so the lanes of a wave start on the same pixel or on neighbouring ones.  A lane whose path has ended takes the wave's next path (__ballot +
// mbcnt prefix).  The wave's cursor runs through chunks of X.chunk consecutive paths, dealt statically: wave w of W takes chunks w, w + W, ...
// No global counter: nothing to zero, launches on different streams may overlap.  Every loop ends by max_depth or by the end of the wave's
// chunks; lanes past the last path never become alive and take part in every vote.  Sums: the accumulator's key is the PIXEL, so flush_acc
// adds a lane's partial sum straight into the pass frame (masked butterfly, one f64 atomic per channel) when the lane moves to another pixel
// and at the end.  A list entry outside the frame, or one whose samples would pass 2^32 - 1, is consumed and dropped where it is fetched:
// no path, no write — the kernel cannot be made to write out of bounds by its list.
//
// ELEMENT-WISE: pure streams, no LDS beyond a few words for the block reductions, no scratch.  Doubles of pixel p sit at byte 24 p: 16-byte
// aligned for even p and 8 bytes past that for odd p when the buffer is 16-byte aligned — one 16-byte and one 8-byte access either way
// (ld3 / st3; rt_query_dev.h's load_ray is the pattern); buffers that are only 8-byte aligned go through 8-byte accesses.
#define RT_TU 3
#include "rt_kernel.hip"
#include "rt_pixels.h"
#include "rt_adaptive.h"
#include "rt_query_dev.h"

namespace rt {

typedef uint32_t au4 __attribute__((ext_vector_type(4)));

// Resident waves per SIMD the register allocation is held to, from -Rpass-analysis=kernel-resource-usage and the loop depth of every scratch
// access in the ISA (make asm, tools/scratch_map.py); RadianceWaves' classes — the loop is that kernel's with the camera code in the place of
// a 56-byte load; the table is DESIGN §18's.
#ifndef RT_PIXELS_LEAN_WAVES
#define RT_PIXELS_LEAN_WAVES 5u                     // (A/B builds: make KFLAGS=-DRT_PIXELS_LEAN_WAVES=4u)
#endif
template <uint32_t FEATS> struct PixelsWaves {
    static constexpr uint32_t v = FEATS == 0u ? RT_PIXELS_LEAN_WAVES :((FEATS & F_NESTED) ? 1u : ((FEATS & ~(uint32_t)(F_BVH | F_TRIS)) == 0u ? 4u : 3u));
};

template <uint32_t FEATS>
__global__ void __launch_bounds__(PIXELS_THREADS, PixelsWaves<FEATS>::v) pixels_kernel(const KParams<double> P, const PixelsArgs X) {
    typedef double T;
    if ((FEATS & F_BVH) && P.n_cached != 0u) stage_filter_tree<PIXELS_THREADS>(P);      // once per workgroup
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave_in_block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // the wave's cursor (wave-uniform: scalar registers): next chunk, and paths [.., + left) of the current one starting at (cur_k, cur_s)
    const uint64_t n_waves = (uint64_t)gridDim.x * (PIXELS_THREADS / 64u);
    uint64_t next_chunk = (uint64_t)blockIdx.x * (PIXELS_THREADS / 64u) + wave_in_block;
    uint32_t left = 0u, cur_k = 0u, cur_s = 0u;
    // per-lane path state (trace_lockstep's)
    bool alive = false;
    RayT<T> ray; ray.o = mk<T>(T(0), T(0), T(0)); ray.d = ray.o; ray.tm = T(0);
    V3<T> beta = mk<T>(T(0), T(0), T(0));
    uint32_t depth_left = 0, path_s = 0;
    Rng rng; rng.s0 = rng.s1 = rng.s2 = rng.s3 = 0;
    uint32_t acc_px = NONE_PX;                                    // the pixel the accumulator belongs to (W*H <= 2^31 - 1: never a pixel's index)
    AccReg acc; acc.set(0, 0.0); acc.set(1, 0.0); acc.set(2, 0.0);
    uint32_t n_nonfinite = 0, n_flush = 0;

    for (;;) {
        // ---- lanes whose path has ended take the wave's next paths, in lane order
        bool got_new = false;
        uint32_t new_px = 0;
        for (;;) {
            const unsigned long long want = __ballot(!alive && !got_new);
            if (want == 0ull) break;
            if (left == 0u) {
                if (next_chunk >= X.n_chunks) break;              // the wave's chunks are used up
                const uint64_t p0 = next_chunk * X.chunk, rest = X.n_paths - p0;
                left = rest < (uint64_t)X.chunk ? (uint32_t)rest : X.chunk;
                const uint64_t k0 = p0 / P.spp;                   // (once per chunk, wave-uniform)
                cur_k = (uint32_t)k0; cur_s = (uint32_t)(p0 - k0 * P.spp);
                next_chunk += n_waves;
            }
            const uint32_t n_want = (uint32_t)__popcll(want);
            const uint32_t take = n_want < left ? n_want : left;
            const uint32_t rank = lane_rank(want);
            if (!alive && !got_new && rank < take) {
                uint32_t k, s;
                path_step(cur_k, cur_s, rank, P.spp, k, s);
                const uint32_t gp = X.list[k];                    // k < n_list: the path is one of n_list * n_b
                if (gp < X.n_px) {
                    const uint32_t first = X.counts ? X.counts[gp] : 0u;
                    if ((uint64_t)first + P.spp <= 0xFFFFFFFFull) { got_new = true; new_px = gp; path_s = first + s; }
                }
            }
            path_step(cur_k, cur_s, take, P.spp, cur_k, cur_s);
            left -= take;
        }
        if (__ballot(alive || got_new) == 0ull) break;            // no chunk left and every path finished

        // ---- lanes moving on to another pixel hand in their partial sum
        flush_acc<T, AccReg, false>(P, got_new && acc_px != NONE_PX && acc_px != new_px, acc_px, acc, lane, n_flush);

        if (got_new) {
            if (acc_px != new_px) { acc_px = new_px; acc.set(0, 0.0); acc.set(1, 0.0); acc.set(2, 0.0); }
            camera_ray(P, P.seed, new_px, path_s, ray, rng);       // the pixel's own sample: no seed folding
            beta = mk<T>(T(1.0), T(1.0), T(1.0));
            depth_left = P.max_depth;
            alive = true;
        }

        // ---- one level of ray_color (main.rs:41-120) for every live lane
        if (alive) {
            bool done = false;
            V3<T> e = mk<T>(T(0), T(0), T(0));                    // terminal radiance of this path (times beta)
            if (depth_left == 0) {
                done = true;                                      // main.rs:42-45
            } else {
                T t_hit; HitId id; id.obj = 0; id.prim = 0;
                bool any_hit;                                                                            // main.rs:48
                if constexpr (FEATS == 0u) any_hit = world_hit_list<T>(P, ray, TMin<T>::v(), rng, t_hit, id);
                else any_hit = world_hit<T, FEATS>(P, ray, TMin<T>::v(), rng, t_hit, id, nullptr);
                if (!any_hit) {
                    e = ld3(P.background); done = true;                                                  // main.rs:118
                } else {
                    Rec<T> rec;
                    finalize_hit<T, FEATS>(P, ray, t_hit, id, true, rec);
                    shade_hit<T, FEATS>(P, rec, ray, beta, rng, depth_left, done, e);
                }
            }
            if (done) {
                add_radiance(P, beta * e, acc, n_nonfinite, acc_px, path_s);
                alive = false;
            }
        }
    }
    // ---- the wave's chunks are used up: hand in what is left
    flush_acc<T, AccReg, false>(P, acc_px != NONE_PX, acc_px, acc, lane, n_flush);
    if (X.nonfinite && n_nonfinite) atomicAdd(X.nonfinite, (unsigned long long)n_nonfinite);
}

// the instantiation: radiance_kernel's five scene classes
template <typename G> static auto pixels_kernel_for(uint32_t scene_feats, G&& g) {
    return scene_class_dispatch_pbr(scene_feats, [&](auto feats) { return g(pixels_kernel<decltype(feats)::value>); });
}
int pixels_blocks_per_cu(uint32_t scene_feats, size_t shmem) {
    return pixels_kernel_for(scene_feats, [&](auto kernel) { return kernel_blocks_per_cu(kernel, PIXELS_THREADS, shmem); });
}
hipError_t launch_pixels(const KParams<double>& P, const PixelsArgs& X, uint32_t scene_feats, uint32_t n_blocks, size_t shmem, hipStream_t stream) {
    return pixels_kernel_for(scene_feats, [&](auto kernel) { return kernel_launch(kernel, PIXELS_THREADS, n_blocks, shmem, stream, P, X); });
}

// ------------------------------------------------------------------ the element-wise kernels (rt_adaptive.h (A) - (D))
// the three doubles of pixel p; A16: `base` is 16-byte aligned
template <bool A16> DEV void ld3d(const double* base, uint64_t p, double v[3]) {
    const double* q = base + 3u * p;
    if constexpr (A16) {
        const uint32_t odd = (uint32_t)p & 1u;
        const d2 t = *(const d2*)(q + odd);
        const double s = odd ? q[0] : q[2];
        v[0] = odd ? s : t.x; v[1] = odd ? t.x : t.y; v[2] = odd ? t.y : s;
    } else { v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; }
}
template <bool A16> DEV void st3d(double* base, uint64_t p, const double v[3]) {
    double* q = base + 3u * p;
    if constexpr (A16) {
        const uint32_t odd = (uint32_t)p & 1u;
        d2 t; t.x = odd ? v[1] : v[0]; t.y = odd ? v[2] : v[1];
        *(d2*)(q + odd) = t;
        if (odd) q[0] = v[0]; else q[2] = v[2];
    } else { q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; }
}
static bool is_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15u) == 0u; }
static uint32_t blocks_for(uint64_t n, uint32_t most = ADAPTIVE_MAX_BLOCKS) {
    const uint64_t b = (n + ADAPTIVE_THREADS - 1u) / ADAPTIVE_THREADS;
    return (uint32_t)(b > most ? most : b);
}

// (A): rt_moments.hip's error kernel with the pixel's own counts
template <bool A16>
__global__ __launch_bounds__(256) void adaptive_error_kernel(const double* __restrict__ sum, const double* __restrict__ sq, const uint32_t* __restrict__ cnt,
                                                             const uint32_t* __restrict__ pas, uint32_t n_px, double* __restrict__ e2_out, double tau2,
                                                             unsigned long long* stats) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    uint32_t conv = 0u, unconv = 0u, nonfinite = 0u;          // (a lane sees at most n_px / stride + 1 pixels, a wave 64 times that: n_px < 2^31)
    double mx = 0.0;
    for (uint64_t p = (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; p < n_px; p += stride) {
        double S[3], Q[3];
        ld3d<A16>(sum, p, S); ld3d<A16>(sq, p, Q);
        const double e = adaptive_pixel_e2(S, Q, cnt[p], pas[p]);
        if (e2_out) e2_out[p] = e;
        if (!moments_finite(e)) nonfinite++;
        else {
            if (e <= tau2) conv++; else unconv++;
            if (e > mx) mx = e;
        }
    }
    if (!stats) return;                                        // (uniform: a kernel argument)
    unsigned long long mbits = (unsigned long long)__double_as_longlong(mx);      // mx >= +0.0: its bit pattern orders as it does
    for (int off = 32; off > 0; off >>= 1) {
        conv += __shfl_xor(conv, off, 64);
        unconv += __shfl_xor(unconv, off, 64);
        nonfinite += __shfl_xor(nonfinite, off, 64);
        const unsigned long long other = __shfl_xor(mbits, off, 64);
        mbits = other > mbits ? other : mbits;
    }
    __shared__ unsigned long long part[ADAPTIVE_THREADS / 64u][MOMENTS_STATS_WORDS];
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* w = part[threadIdx.x >> 6];
        w[MOMENTS_CONVERGED] = conv; w[MOMENTS_UNCONVERGED] = unconv; w[MOMENTS_NONFINITE] = nonfinite; w[MOMENTS_MAX_E2] = mbits;
    }
    __syncthreads();                                           // (every lane of the workgroup is here: `stats` is uniform)
    if (threadIdx.x == 0u) {
        unsigned long long c = 0ull, u = 0ull, nf = 0ull, mb = 0ull;
        for (uint32_t k = 0; k < ADAPTIVE_THREADS / 64u; k++) {
            c += part[k][MOMENTS_CONVERGED]; u += part[k][MOMENTS_UNCONVERGED]; nf += part[k][MOMENTS_NONFINITE];
            mb = part[k][MOMENTS_MAX_E2] > mb ? part[k][MOMENTS_MAX_E2] : mb;
        }
        if (c) atomicAdd(&stats[MOMENTS_CONVERGED], c);
        if (u) atomicAdd(&stats[MOMENTS_UNCONVERGED], u);
        if (nf) atomicAdd(&stats[MOMENTS_NONFINITE], nf);
        if (mb) atomicMax(&stats[MOMENTS_MAX_E2], mb);
    }
}

// (B) step 1: need[p], one byte per pixel
template <bool A16>
__global__ __launch_bounds__(256) void adaptive_need_kernel(const double* __restrict__ sum, const double* __restrict__ sq, const uint32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ pas, uint32_t n_px, double tau2, uint8_t* __restrict__ need) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    for (uint64_t p = (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; p < n_px; p += stride) {
        double S[3], Q[3];
        ld3d<A16>(sum, p, S); ld3d<A16>(sq, p, Q);
        const uint32_t b = pas[p];
        need[p] = adaptive_need(adaptive_pixel_e2(S, Q, cnt[p], b), b, tau2) ? (uint8_t)1u : (uint8_t)0u;
    }
}

// the sum of `v` over the workgroup's 256 lanes in every lane's `total`, and the sum over the lanes below this one returned (exclusive scan):
// shuffles inside a wave, four words of LDS across the waves
DEV uint32_t block_exclusive_scan256(uint32_t v, uint32_t* wave_part, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += o;
    }
    if (lane == 63u) wave_part[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
    for (uint32_t k = 0; k < ADAPTIVE_THREADS / 64u; k++) { const uint32_t w = wave_part[k]; if (k < wave) before += w; all += w; }
    __syncthreads();                                           // wave_part may be written again by the caller's next use
    total = all;
    return before + inc - v;
}

// (B) step 2: active[p] for the ADAPTIVE_BLOCK_PX pixels of this workgroup, four consecutive pixels per lane, and the workgroup's count.
// need and active are the workspace's: 16-byte aligned, so a lane's four flags are one aligned dword.
__global__ __launch_bounds__(256) void adaptive_active_kernel(const uint8_t* __restrict__ need, const uint32_t* __restrict__ cnt, uint32_t W, uint32_t H, uint32_t n_b,
                                                              unsigned long long max_samples, uint32_t spread, uint8_t* __restrict__ active,
                                                              uint32_t* __restrict__ block_count) {
    const uint32_t n_px = W * H;
    const uint64_t p0 = (uint64_t)blockIdx.x * ADAPTIVE_BLOCK_PX + 4u * threadIdx.x;
    uint32_t flags = 0u, mine = 0u;
    if (p0 < n_px) {
        uint32_t y = (uint32_t)(p0 / W), x = (uint32_t)(p0 - (uint64_t)y * W);
        for (uint32_t i = 0; i < 4u && p0 + i < n_px; i++) {
            const uint64_t p = p0 + i;
            bool needed = need[p] != 0u;
            if (!needed && spread) {
                const uint32_t y0 = y ? y - 1u : 0u, y1 = y + 1u < H ? y + 1u : y, x0 = x ? x - 1u : 0u, x1 = x + 1u < W ? x + 1u : x;
                for (uint32_t yy = y0; yy <= y1; yy++)
                    for (uint32_t xx = x0; xx <= x1; xx++) needed = needed || need[(uint64_t)yy * W + xx] != 0u;
            }
            if (needed && adaptive_room(cnt[p], n_b, max_samples)) { flags |= 1u << (8u * i); mine++; }
            if (++x == W) { x = 0u; y++; }
        }
        if (p0 + 3u < n_px) *(uint32_t*)(active + p0) = flags;
        else for (uint32_t i = 0; p0 + i < n_px; i++) active[p0 + i] = (uint8_t)((flags >> (8u * i)) & 1u);
    }
    __shared__ uint32_t wave_part[ADAPTIVE_THREADS / 64u];
    uint32_t total;
    (void)block_exclusive_scan256(mine, wave_part, total);
    if (threadIdx.x == 0u) block_count[blockIdx.x] = total;
}

// (B) step 3: the workgroups' counts become their offsets (exclusive scan, in place) and the total the list's length; ONE workgroup, which
// walks the counts 1024 at a time and carries the running sum
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(uint32_t* __restrict__ block_count, uint32_t n_blocks, uint32_t* __restrict__ n_list_out) {
    __shared__ uint32_t wave_part[ADAPTIVE_SCAN_THREADS / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < n_blocks; base += ADAPTIVE_SCAN_THREADS) {      // (uniform trip count: every lane reaches the barriers)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_count[i] : 0u;
        uint32_t inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off, 64);
            if (lane >= (uint32_t)off) inc += o;
        }
        if (lane == 63u) wave_part[wave] = inc;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t k = 0; k < ADAPTIVE_SCAN_THREADS / 64u; k++) { const uint32_t w = wave_part[k]; if (k < wave) before += w; all += w; }
        __syncthreads();
        if (i < n_blocks) block_count[i] = carry + before + inc - v;
        carry += all;
    }
    if (threadIdx.x == 0u) *n_list_out = carry;
}

// (B) step 4: the active pixels' indices, ascending: a workgroup's pixels follow those of the workgroups before it, a lane's those of the
// lanes below it, and a lane writes its own in order
__global__ __launch_bounds__(256) void adaptive_scatter_kernel(const uint8_t* __restrict__ active, uint32_t n_px, const uint32_t* __restrict__ block_offset,
                                                               uint32_t* __restrict__ list) {
    const uint64_t p0 = (uint64_t)blockIdx.x * ADAPTIVE_BLOCK_PX + 4u * threadIdx.x;
    uint32_t flags = 0u;
    if (p0 + 3u < n_px) flags = *(const uint32_t*)(active + p0);
    else for (uint32_t i = 0; p0 + i < n_px; i++) flags |= (uint32_t)active[p0 + i] << (8u * i);
    const uint32_t mine = (flags & 1u) + ((flags >> 8) & 1u) + ((flags >> 16) & 1u) + ((flags >> 24) & 1u);
    __shared__ uint32_t wave_part[ADAPTIVE_THREADS / 64u];
    uint32_t total;
    uint32_t at = block_offset[blockIdx.x] + block_exclusive_scan256(mine, wave_part, total);
    for (uint32_t i = 0; i < 4u; i++)
        if ((flags >> (8u * i)) & 1u) list[at++] = (uint32_t)p0 + i;
}

// (C) over a list: one listed pixel per lane
template <bool A16>
__global__ __launch_bounds__(256) void adaptive_merge_kernel(double* __restrict__ pass, double nb, uint32_t n_b, double* __restrict__ sum, double* __restrict__ sq,
                                                             uint32_t* __restrict__ cnt, uint32_t* __restrict__ pas, const uint32_t* __restrict__ list, uint32_t n_list,
                                                             uint32_t* max_out) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    const double zero[3] = {0.0, 0.0, 0.0};
    uint32_t largest = 0u;
    for (uint64_t k = (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; k < n_list; k += stride) {
        const uint64_t p = list[k];
        double x[3], S[3], Q[3];
        ld3d<A16>(pass, p, x); ld3d<A16>(sum, p, S); ld3d<A16>(sq, p, Q);
        moments_merge(x[0], nb, S[0], Q[0]); moments_merge(x[1], nb, S[1], Q[1]); moments_merge(x[2], nb, S[2], Q[2]);
        st3d<A16>(sum, p, S); st3d<A16>(sq, p, Q); st3d<A16>(pass, p, zero);
        const uint32_t n = cnt[p] + n_b;
        cnt[p] = n; pas[p] += 1u;
        largest = n > largest ? n : largest;
    }
    if (!max_out) return;                                      // (uniform: a kernel argument)
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(largest, off, 64); largest = o > largest ? o : largest; }
    if ((threadIdx.x & 63u) == 0u && largest != 0u) atomicMax(max_out, largest);      // an integer maximum: no word depends on the order of arrival
}
// (C)'s counts over ALL pixels (a uniform pass: rt_moments.hip's merge has done the doubles): four pixels per lane where both arrays are 16-byte aligned
__global__ __launch_bounds__(256) void adaptive_bump4_kernel(au4* __restrict__ cnt, au4* __restrict__ pas, uint32_t n_b, uint32_t n_quads) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; i < n_quads; i += stride) {
        au4 c = cnt[i], b = pas[i];
        c.x += n_b; c.y += n_b; c.z += n_b; c.w += n_b;
        b.x += 1u; b.y += 1u; b.z += 1u; b.w += 1u;
        cnt[i] = c; pas[i] = b;
    }
}
__global__ __launch_bounds__(256) void adaptive_bump1_kernel(uint32_t* __restrict__ cnt, uint32_t* __restrict__ pas, uint32_t n_b, uint32_t first, uint32_t n_px) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    for (uint64_t i = (uint64_t)first + (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; i < n_px; i += stride) { cnt[i] += n_b; pas[i] += 1u; }
}

// the workgroup's changed-pixel count added with ONE atomic: every atomic of a launch lands on the same word, and atomics on one line are
// served one after another (rt_moments.hip: about 150 per microsecond) — one per wave was *measured* first: 0.036 ms at 800 x 800 and
// 0.40 ms at 3840 x 2160, the time of the atomics alone.  Hence also the smaller grid: at most ADAPTIVE_ERROR_MAX_BLOCKS workgroups.
DEV void add_changed(uint32_t changed, unsigned long long* changed_px) {
    for (int off = 32; off > 0; off >>= 1) changed += __shfl_xor(changed, off, 64);
    __shared__ uint32_t part[ADAPTIVE_THREADS / 64u];
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = changed;
    __syncthreads();                                           // (every lane of the workgroup is here: the grid-stride loops have ended)
    if (threadIdx.x == 0u && changed_px) {
        uint32_t all = 0u;
        for (uint32_t k = 0; k < ADAPTIVE_THREADS / 64u; k++) all += part[k];
        if (all) atomicAdd(changed_px, (unsigned long long)all);
    }
}

// (D): rt_resolve.hip's shape — FOUR consecutive pixels per lane: 96 B of sums as six 16-byte loads, the four counts as one, three dwords of
// the previous image, three dword stores — for 16-byte aligned sums and counts and 4-byte aligned images; the frame's last n_px % 4 pixels
// byte-wise by one lane
__global__ __launch_bounds__(256) void adaptive_resolve4_kernel(const double* __restrict__ sum, const uint32_t* __restrict__ cnt, const uint8_t* rgb8_prev,
                                                                uint8_t* __restrict__ rgb8_out, unsigned long long* changed_px, uint32_t n_px) {
    const uint32_t n_groups = n_px / 4u;
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    uint32_t changed = 0u;
    for (uint32_t g = blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; g < n_groups; g += stride) {
        const d2* in = reinterpret_cast<const d2*>(sum) + (size_t)g * 6u;
        d2 v[6];
#pragma unroll
        for (int k = 0; k < 6; k++) v[k] = in[k];
        const au4 n4 = reinterpret_cast<const au4*>(cnt)[g];
        const uint32_t n[4] = {n4.x, n4.y, n4.z, n4.w};
        uint32_t b[12];
#pragma unroll
        for (int k = 0; k < 6; k++) { b[2 * k] = adaptive_format_channel(v[k].x, n[(2 * k) / 3]); b[2 * k + 1] = adaptive_format_channel(v[k].y, n[(2 * k + 1) / 3]); }
        uint32_t w[3];
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        if (rgb8_prev) {
            const uint32_t* pv = reinterpret_cast<const uint32_t*>(rgb8_prev) + (size_t)g * 3u;
            const uint32_t x0 = pv[0] ^ w[0], x1 = pv[1] ^ w[1], x2 = pv[2] ^ w[2];
            // bytes 0..2 | 3..5 | 6..8 | 9..11 of the twelve are the four pixels
            changed += ((x0 & 0x00FFFFFFu) != 0u) + (((x0 >> 24) | (x1 & 0x0000FFFFu)) != 0u) + (((x1 >> 16) | (x2 & 0x000000FFu)) != 0u) + ((x2 >> 8) != 0u);
        } else changed += 4u;
        uint32_t* o = reinterpret_cast<uint32_t*>(rgb8_out) + (size_t)g * 3u;
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)                               // the frame's last n_px % 4 pixels
        for (uint32_t p = n_groups * 4u; p < n_px; p++) {
            bool differs = rgb8_prev == nullptr;
            for (uint32_t k = 0; k < 3u; k++) {
                const uint8_t c = (uint8_t)adaptive_format_channel(sum[(size_t)p * 3u + k], cnt[p]);
                if (rgb8_prev && rgb8_prev[(size_t)p * 3u + k] != c) differs = true;
                rgb8_out[(size_t)p * 3u + k] = c;
            }
            changed += differs ? 1u : 0u;
        }
    add_changed(changed, changed_px);
}
// ... and for any other alignment: one pixel per lane, byte-wise
__global__ __launch_bounds__(256) void adaptive_resolve1_kernel(const double* __restrict__ sum, const uint32_t* __restrict__ cnt, const uint8_t* rgb8_prev,
                                                                uint8_t* __restrict__ rgb8_out, unsigned long long* changed_px, uint32_t n_px) {
    const uint32_t stride = gridDim.x * ADAPTIVE_THREADS;
    uint32_t changed = 0u;
    for (uint64_t p = (uint64_t)blockIdx.x * ADAPTIVE_THREADS + threadIdx.x; p < n_px; p += stride) {
        const uint32_t n = cnt[p];
        bool differs = rgb8_prev == nullptr;
        for (uint32_t k = 0; k < 3u; k++) {
            const uint8_t c = (uint8_t)adaptive_format_channel(sum[p * 3u + k], n);
            if (rgb8_prev && rgb8_prev[p * 3u + k] != c) differs = true;
            rgb8_out[p * 3u + k] = c;
        }
        changed += differs ? 1u : 0u;
    }
    add_changed(changed, changed_px);
}

int launch_adaptive_error(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t n_px, double* d_e2_out, double tau2,
                          unsigned long long* d_stats, void* stream) {
    if (n_px == 0u) return 0;
    const dim3 grid(blocks_for(n_px, ADAPTIVE_ERROR_MAX_BLOCKS)), block(ADAPTIVE_THREADS);
    if (is_aligned16(d_S, d_Q)) hipLaunchKernelGGL(adaptive_error_kernel<true>, grid, block, 0, (hipStream_t)stream, d_S, d_Q, d_n, d_b, n_px, d_e2_out, tau2, d_stats);
    else hipLaunchKernelGGL(adaptive_error_kernel<false>, grid, block, 0, (hipStream_t)stream, d_S, d_Q, d_n, d_b, n_px, d_e2_out, tau2, d_stats);
    return (int)hipGetLastError();
}

int launch_adaptive_select(const double* d_S, const double* d_Q, const uint32_t* d_n, const uint32_t* d_b, uint32_t W, uint32_t H, uint32_t n_b, double tau2,
                           uint64_t max_samples, uint32_t spread, uint32_t* d_list_out, uint32_t* d_count_out, void* d_workspace, void* stream) {
    const uint32_t n_px = W * H;
    if (n_px == 0u) return 0;
    const uint64_t flag_bytes = ((uint64_t)n_px + 15u) & ~(uint64_t)15u;
    uint8_t* need = (uint8_t*)d_workspace;
    uint8_t* active = need + flag_bytes;
    uint32_t* block_count = (uint32_t*)(active + flag_bytes);
    const uint32_t n_blocks = (uint32_t)(((uint64_t)n_px + ADAPTIVE_BLOCK_PX - 1u) / ADAPTIVE_BLOCK_PX);
    hipStream_t st = (hipStream_t)stream;
    if (is_aligned16(d_S, d_Q)) hipLaunchKernelGGL(adaptive_need_kernel<true>, dim3(blocks_for(n_px)), dim3(ADAPTIVE_THREADS), 0, st, d_S, d_Q, d_n, d_b, n_px, tau2, need);
    else hipLaunchKernelGGL(adaptive_need_kernel<false>, dim3(blocks_for(n_px)), dim3(ADAPTIVE_THREADS), 0, st, d_S, d_Q, d_n, d_b, n_px, tau2, need);
    hipLaunchKernelGGL(adaptive_active_kernel, dim3(n_blocks), dim3(ADAPTIVE_THREADS), 0, st, need, d_n, W, H, n_b, (unsigned long long)max_samples, spread, active, block_count);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(ADAPTIVE_SCAN_THREADS), 0, st, block_count, n_blocks, d_count_out);
    hipLaunchKernelGGL(adaptive_scatter_kernel, dim3(n_blocks), dim3(ADAPTIVE_THREADS), 0, st, active, n_px, block_count, d_list_out);
    return (int)hipGetLastError();
}

int launch_adaptive_merge(double* d_pass, uint32_t n_b, double* d_S, double* d_Q, uint32_t* d_n, uint32_t* d_b, const uint32_t* d_list, uint32_t n_list,
                          uint32_t* d_max_out, void* stream) {
    if (n_list == 0u) return 0;
    const dim3 grid(blocks_for(n_list)), block(ADAPTIVE_THREADS);
    if (is_aligned16(d_pass, d_S, d_Q)) hipLaunchKernelGGL(adaptive_merge_kernel<true>, grid, block, 0, (hipStream_t)stream, d_pass, (double)n_b, n_b, d_S, d_Q, d_n, d_b, d_list, n_list, d_max_out);
    else hipLaunchKernelGGL(adaptive_merge_kernel<false>, grid, block, 0, (hipStream_t)stream, d_pass, (double)n_b, n_b, d_S, d_Q, d_n, d_b, d_list, n_list, d_max_out);
    return (int)hipGetLastError();
}

int launch_adaptive_bump(uint32_t* d_n, uint32_t* d_b, uint32_t n_b, uint32_t n_px, void* stream) {
    if (n_px == 0u) return 0;
    const uint32_t n_quads = is_aligned16(d_n, d_b) ? n_px / 4u : 0u;
    if (n_quads) hipLaunchKernelGGL(adaptive_bump4_kernel, dim3(blocks_for(n_quads)), dim3(ADAPTIVE_THREADS), 0, (hipStream_t)stream, (au4*)d_n, (au4*)d_b, n_b, n_quads);
    if (4u * n_quads < n_px) hipLaunchKernelGGL(adaptive_bump1_kernel, dim3(blocks_for(n_px - 4u * n_quads)), dim3(ADAPTIVE_THREADS), 0, (hipStream_t)stream, d_n, d_b, n_b, 4u * n_quads, n_px);
    return (int)hipGetLastError();
}

int launch_adaptive_resolve(const double* d_S, const uint32_t* d_n, const uint8_t* d_rgb8_prev, uint8_t* d_rgb8_out, unsigned long long* d_changed, uint32_t n_px, void* stream) {
    if (n_px == 0u) return 0;
    const bool wide = is_aligned16(d_S, d_n) && ((((uintptr_t)d_rgb8_prev) | ((uintptr_t)d_rgb8_out)) & 3u) == 0u;
    if (wide) {
        uint32_t blocks = blocks_for(n_px / 4u, ADAPTIVE_ERROR_MAX_BLOCKS);
        if (blocks == 0u) blocks = 1u;
        hipLaunchKernelGGL(adaptive_resolve4_kernel, dim3(blocks), dim3(ADAPTIVE_THREADS), 0, (hipStream_t)stream, d_S, d_n, d_rgb8_prev, d_rgb8_out, d_changed, n_px);
    } else hipLaunchKernelGGL(adaptive_resolve1_kernel, dim3(blocks_for(n_px, ADAPTIVE_ERROR_MAX_BLOCKS)), dim3(ADAPTIVE_THREADS), 0, (hipStream_t)stream, d_S, d_n, d_rgb8_prev, d_rgb8_out, d_changed, n_px);
    return (int)hipGetLastError();
}

} // namespace rt
