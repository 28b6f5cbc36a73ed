// csrc/rt_frames.cpp — the progressive frame of librt_amd.so's C-ABI (include/rt_amd.h: rt_progressive_*) and the image operations over a
// frame of sums: moments, adaptive passes, the denoisers, reprojection, the temporal blend.  No launch shape of a path-tracing kernel lives
// here: passes go through rt_host.cpp's render_any and launch_pixel_list (rt_host_shared.h), guides and albedo sums through the public queries.
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>
#include "rt_host_shared.h"
#include "rt_device.h"
#include "rt_resolve.h"
#include "rt_denoise.h"
#include "rt_albedo.h"
#include "rt_moments.h"
#include "rt_denoise_var.h"
#include "rt_adaptive.h"
#include "rt_denoise_frame.h"
#include "rt_reproject.h"
#include "rt_reproject_var.h"
#include "rt_chain.h"

using namespace rt;

// A progressive frame (rt_progressive_*, include/rt_amd.h): one fixed view of one scene, the device-resident f64 sum frame its passes
// accumulate into, and two RGB8 images — the most recent resolve and the one before it, which the next resolve is compared with and
// then overwrites.  Everything lives on `device`: the buffers are members that free themselves, so the frame is deleted with that device
// current (progressive_free).  The handle the C-ABI passes around (a void*) is a pointer to this.
namespace {
struct Progressive {
    rt_scene* sc = nullptr;                // nullptr once the scene has been destroyed: the frame can still be read, resolved and destroyed
    unsigned long long scene_version = 0;  // Scene::version at create / reset: a pass after a change to the scene is refused
    rt_camera cam; double bg[3] = {0, 0, 0};
    uint32_t W = 0, H = 0, max_depth = 0, flags = 0; uint64_t seed = 0;
    int device = -1;
    uint64_t done = 0;                     // samples per pixel accumulated so far
    DeviceBuffer d_sum;                    // W*H*3 doubles, output order
    DeviceBuffer d_rgb8[2]; int cur = 0; bool have_prev = false, resolved = false;     // d_rgb8[cur]: the most recent resolve
    DeviceBuffer d_changed;                // one 64-bit word: the most recent resolve's changed-pixel count
    // rt_progressive_resolve_denoised_rgb8's own buffers, allocated at its first call: the filter's workspace (two packed colour frames and
    // the packed guide, rt_denoise.h), the filtered sums, their RGB8 image and the count word its resolve launch needs.  The guide — sample
    // 0's camera hits of this view, keyed for guide_flags — is built once and kept until rt_progressive_reset.
    DeviceBuffer d_dn_ws, d_dn_sum, d_dn_rgb8, d_dn_changed;
    bool guide_valid = false; uint32_t guide_flags = 0;
    // rt_progressive_set_guide_samples: 1 is the guide above; n > 1 builds it from samples [0, n) of this view under the frame's seed instead
    // (rt_query_camera_guide_device, rt_guide.h).  guide_builds counts the guides built, of either kind.
    uint32_t guide_samples = 1; uint64_t guide_builds = 0;
    // rt_progressive_set_guide_chain: chain_links > 0 builds the guide AND the albedo sums from the specular-chain records of samples
    // [0, guide_samples) (rt_query_camera_chain_guide_device, rt_chain.h) in one launch; albedo_chain says that d_alb_sum holds such sums
    uint32_t chain_links = 0; double chain_fuzz = 0.0; bool albedo_chain = false;
    // rt_progressive_resolve_denoised_albedo_rgb8's own, beside the above: the albedo sums of samples [0, albedo_samples) of this view under
    // the frame's seed (rt_query_camera_albedo_device), built when first asked for and kept until rt_progressive_reset or another
    // albedo_samples, and the demodulated frame of a run (24 + 24 bytes per pixel).  albedo_builds counts the launches that built d_alb_sum.
    DeviceBuffer d_alb_sum, d_alb_x;
    uint32_t albedo_samples = 0; uint64_t albedo_builds = 0;
    // rt_progressive_enable_moments (rt_moments.h): the second moments Q (d_sq) and the pass frame a pass renders into before the merge
    // kernel adds it to d_sum and d_sq and zeroes it again (24 + 24 bytes per pixel); `passes` merges so far; moments_valid: d_sq describes
    // the samples d_sum holds (rt_progressive_load_sum breaks that).  ev_merged is recorded behind every merge: the next pass's stream waits
    // for it, because passes on different streams share d_pass.  d_e2 (rt_progressive_error_map*, allocated at the first call) and the
    // four statistics words.
    bool moments = false, moments_valid = false, merge_recorded = false; uint64_t passes = 0;
    DeviceBuffer d_sq, d_pass, d_e2, d_mstats;
    DeviceEvent ev_merged;
    // rt_progressive_variance / rt_progressive_resolve_denoised_variance_rgb8: the per-channel variance frame (rt_moments.h (4)) of the sums
    // as they are at that call, allocated at the first one (24 bytes per pixel)
    DeviceBuffer d_var;
    // rt_progressive_enable_adaptive (rt_adaptive.h): per-pixel counts n (d_cnt) and b (d_pas), the pixel list of a pass with its length and
    // the largest count behind a list merge (d_words: two uint32), and the selection's workspace.  `uniform`: every n[p] equals `done` and
    // every b[p] equals `passes` — true until the first pass over a proper subset; from then on `done` is the largest n[p] and `passes` the
    // passes of the frame.  total: the sum of n[p].
    bool adaptive = false, uniform = true; uint64_t total = 0;
    DeviceBuffer d_cnt, d_pas, d_list, d_words, d_sel_ws;
    // rt_progressive_resolve_denoised_frame_rgb8's own, beside the denoised resolves': the per-pixel means c and the demodulated variance Vd
    // of a run (rt_denoise_frame.h (F): two frames of 24 bytes per pixel, each padded to 16), allocated at its first call
    DeviceBuffer d_fr_planes;
    // rt_progressive_set_view (rt_reproject.h): the history H_sum (24 bytes per pixel) and H_cnt (4), allocated at first use; hist_valid: they
    // hold a history (rt_progressive_reset drops it; an all-zero one is made when one is needed); hist_px: the pixels with H_cnt > 0;
    // views: the views taken over the frame's life
    DeviceBuffer d_hist_sum, d_hist_cnt;
    bool hist_valid = false; uint64_t hist_px = 0, views = 0;
    // ... on a frame with moments (rt_reproject_var.h): the history's variance H_var (24 bytes per pixel), allocated at first use;
    // hist_var_valid: it describes the history the two buffers above hold
    DeviceBuffer d_hist_var;
    bool hist_var_valid = false;
    size_t n_px() const { return (size_t)W * H; }
    size_t sum_bytes() const { return n_px() * 3 * sizeof(double); }
    const uint32_t* counts() const { return adaptive ? d_cnt.as<uint32_t>() : nullptr; }
};
} // namespace

void rt::frames_scene_gone(Scene& s) { for (void* f : s.frames) ((Progressive*)f)->sc = nullptr; }

// A call that needs the frame's scene as the frame knows it; `gone`: the sentence for a scene that has been destroyed — a resolve that
// would build something from it says what the frame lacks.
static const char* const SCENE_GONE = "the scene of this progressive frame has been destroyed";
static const char* const SCENE_GONE_NO_GUIDE = "the scene of this progressive frame has been destroyed and the frame holds no denoising guide for these flags: the guide is built from the scene (rt_query_camera_device)";
static const char* const SCENE_GONE_NO_ALBEDO = "the scene of this progressive frame has been destroyed and the frame holds no albedo sums for this albedo_samples: they are built from the scene (rt_query_camera_albedo_device)";
static int frame_scene_current(const Progressive* p, const char* gone = SCENE_GONE) {
    if (!p->sc) return set_error(gone);
    if (p->scene_version != p->sc->s.version) return set_error("the scene changed after this progressive frame was created: the frame is forgotten (rt_progressive_reset starts a new one)");
    return 0;
}
// A host array's copy in `d` for one call; a null host pointer leaves d empty, and get() then yields the null the device entry expects.
// a *_check's verdict: empty, or the message of a refusal
static int refused(const std::string& problem) { return problem.empty() ? 0 : set_error(problem); }
static int upload(DeviceBuffer& d, const void* host, size_t bytes) {
    if (!host) return 0;
    HIP_OK(d.alloc(bytes));
    HIP_OK(hipMemcpy(d.get(), host, bytes, hipMemcpyHostToDevice));
    return 0;
}
// The rt_debug_*_ms calls: n marks, created here and destroyed on every path; `run` makes the warm run and then the timed one, which records
// every mark in order (a refused call records nothing and returns non-zero); the n - 1 times between them go to ms_out.
static int timed_between_marks(uint32_t n, float* ms_out, const std::function<int(hipEvent_t*)>& run) {
    hipEvent_t marks[DENOISE_MAX_ITERATIONS + 3u] = {};
    int rc = 0;
    for (uint32_t k = 0; k < n && rc == 0; k++) if (hipEventCreate(&marks[k]) != hipSuccess) rc = set_error("hipEventCreate failed");
    if (rc == 0) rc = run(marks);
    if (rc == 0 && hipEventSynchronize(marks[n - 1u]) != hipSuccess) rc = set_error("hipEventSynchronize failed");
    for (uint32_t k = 0; k + 1u < n && rc == 0; k++) if (hipEventElapsedTime(&ms_out[k], marks[k], marks[k + 1u]) != hipSuccess) rc = set_error("hipEventElapsedTime failed");
    for (uint32_t k = 0; k < n; k++) if (marks[k]) (void)hipEventDestroy(marks[k]);
    return rc;
}

extern "C" {

// ---------------------------------------------------------------- progressive frames
// (the reference's loop prints `Scanlines remaining` while it works, src/main.rs:772-775, and formats each pixel as it is finished,
// src/main.rs:832: a frame that accumulates passes of samples and can be resolved to the 8-bit image at any time is that, per pass)
// what a call that knows one sample count for the whole frame checks first on an adaptive frame
static int adaptive_needs_uniform(const Progressive* p, const char* what) {
    if (p && p->adaptive && !p->uniform)
        return set_error(std::string(what) + ": the pixels of this adaptive frame hold different sample counts, and this call knows one count for the whole frame (rt_progressive_read_counts has them; rt_progressive_variance_counts and rt_progressive_resolve_denoised_frame_rgb8 take the frame as it is)");
    return 0;
}
static void progressive_free(Progressive* p) {
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();                   // passes and resolves may still be in flight on the caller's streams
    delete p;                                       // (its buffers and its event: freed with the frame's device current)
}
void* rt_progressive_create(rt_scene* sc, const rt_camera* cam, const double bg[3], uint32_t W, uint32_t H, uint32_t max_depth,
                            uint64_t seed, uint32_t flags) {
    if (frame_prologue(sc, cam, bg, W, H, 1u)) return nullptr;
    Progressive* p = new Progressive();
    p->sc = sc; p->scene_version = sc->s.version; std::memcpy(&p->cam, cam, sizeof(rt_camera));
    for (int k = 0; k < 3; k++) p->bg[k] = bg[k];
    p->W = W; p->H = H; p->max_depth = max_depth; p->flags = flags; p->seed = seed;
    const size_t n = p->n_px();
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = p->d_sum.ensure(p->sum_bytes());
    if (e == hipSuccess) e = p->d_rgb8[0].ensure(n * 3);
    if (e == hipSuccess) e = p->d_rgb8[1].ensure(n * 3);
    if (e == hipSuccess) e = p->d_changed.ensure(sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(p->d_sum.get(), 0, p->sum_bytes(), nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        set_error(std::string("rt_progressive_create: ") + hipGetErrorString(e));
        if (p->device >= 0) progressive_free(p); else delete p;
        return nullptr;
    }
    sc->s.frames.push_back(p);
    return p;
}
void rt_progressive_destroy(void* frame) {
    Progressive* p = (Progressive*)frame;
    if (!p) return;
    if (p->sc) { std::vector<void*>& fr = p->sc->s.frames; fr.erase(std::remove(fr.begin(), fr.end(), (void*)p), fr.end()); }
    progressive_free(p);
}
// what both forms of a pass check before anything is launched
static int progressive_pass_args(Progressive* p, uint32_t n) {
    if (n == 0) return set_error("n_samples must be >= 1");
    if (!p) return set_error("null argument");
    if (frame_scene_current(p)) return -1;
    if (p->done + n > 0xFFFFFFFFull) return set_error("samples done + n_samples must be <= 2^32 - 1 (the sample field of a path's RNG key is 32 bits, csrc/rt_rng.h)");
    return 0;
}
static int progressive_pass(Progressive* p, uint32_t n, void* d_samples, hipStream_t stream, bool may_calibrate) {
    const size_t n_px = p->n_px();
    if (p->moments) {
        // the pass frame is shared: this pass starts behind the merge of the one before it, whatever stream that was on (the host does not wait)
        if (p->merge_recorded) HIP_OK(hipStreamWaitEvent(stream, p->ev_merged.get(), 0));
        if (render_any(p->sc, &p->cam, p->bg, p->W, p->H, n, p->max_depth, p->seed, p->flags, (uint32_t)n_px, 0, 1, p->d_pass.get(), p->sum_bytes(),
                       d_samples, stream, may_calibrate, (uint32_t)p->done, true)) return -1;
        HIP_OK((hipError_t)launch_moments_merge(p->d_pass.as<double>(), n, p->d_sum.as<double>(), p->d_sq.as<double>(), (uint64_t)n_px * 3u, stream));
        // (an adaptive frame comes here only while it is uniform: (C) over all pixels is the merge above and the counts)
        if (p->adaptive) { HIP_OK((hipError_t)launch_adaptive_bump(p->d_cnt.as<uint32_t>(), p->d_pas.as<uint32_t>(), n, (uint32_t)n_px, stream)); p->total += (uint64_t)n_px * n; }
        HIP_OK(hipEventRecord(p->ev_merged.get(), stream));
        p->merge_recorded = true;
        p->done += n; p->passes++;
        return 0;
    }
    if (render_any(p->sc, &p->cam, p->bg, p->W, p->H, n, p->max_depth, p->seed, p->flags, (uint32_t)n_px, 0, 1, p->d_sum.get(), p->sum_bytes(),
                   d_samples, stream, may_calibrate, (uint32_t)p->done, true)) return -1;
    p->done += n;
    return 0;
}
static int adaptive_pass_over_all(Progressive* p, uint32_t n, double* samples_out);
int rt_progressive_add(void* frame, uint32_t n, double* samples_out) {
    Progressive* p = (Progressive*)frame;
    if (progressive_pass_args(p, n)) return -1;
    if (p->adaptive && !p->uniform) return adaptive_pass_over_all(p, n, samples_out);
    DeviceGuard guard(p->device);
    DeviceBuffer d_samples;
    const size_t sample_bytes = p->n_px() * n * 3 * sizeof(double);
    if (samples_out) HIP_OK(d_samples.alloc(sample_bytes));
    if (progressive_pass(p, n, d_samples.get(), nullptr, true)) return -1;
    hipError_t e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess && samples_out) e = hipMemcpy(samples_out, d_samples.get(), sample_bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? 0 : set_error(std::string("rt_progressive_add: ") + hipGetErrorString(e));
}
int rt_progressive_add_async(void* frame, uint32_t n, void* hip_stream) {
    Progressive* p = (Progressive*)frame;
    if (progressive_pass_args(p, n)) return -1;
    if (p->adaptive) return set_error("rt_progressive_add_async: not available on an adaptive frame (a pass selects, renders, merges and waits: rt_progressive_add, rt_progressive_add_adaptive)");
    DeviceGuard guard(p->device);
    return progressive_pass(p, n, nullptr, (hipStream_t)hip_stream, false);
}
int rt_progressive_samples(void* frame, uint64_t* done_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !done_out) return set_error("null argument");
    *done_out = p->done;
    return 0;
}
int rt_progressive_resolve_rgb8_device(void* frame, void** d_rgb8_out, void* hip_stream) {
    Progressive* p = (Progressive*)frame;
    if (!p) return set_error("null argument");
    if (p->done == 0) return set_error("nothing to resolve: the frame holds 0 samples (format_color divides by the sample count, src/vec.rs:126)");
    DeviceGuard guard(p->device);
    hipStream_t stream = (hipStream_t)hip_stream;
    const int next = 1 - p->cur;
    const uint8_t* prev = p->have_prev ? p->d_rgb8[p->cur].as<uint8_t>() : nullptr;
    HIP_OK(hipMemsetAsync(p->d_changed.get(), 0, sizeof(unsigned long long), stream));
    if (p->adaptive)
        HIP_OK((hipError_t)launch_adaptive_resolve(p->d_sum.as<double>(), p->d_cnt.as<uint32_t>(), prev, p->d_rgb8[next].as<uint8_t>(),
                                                   p->d_changed.as<unsigned long long>(), (uint32_t)p->n_px(), stream));
    else
        HIP_OK(launch_resolve_rgb8(p->d_sum.as<double>(), p->done, prev, p->d_rgb8[next].as<uint8_t>(), p->d_changed.as<unsigned long long>(), (uint32_t)p->n_px(), stream));
    p->cur = next; p->have_prev = true; p->resolved = true;
    if (d_rgb8_out) *d_rgb8_out = p->d_rgb8[next].get();
    return 0;
}
int rt_progressive_copy_rgb8(void* frame, uint8_t* rgb8_out, uint64_t* changed_px_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !rgb8_out) return set_error("null argument");
    if (!p->resolved) return set_error("the frame has not been resolved (rt_progressive_resolve_rgb8_device)");
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rgb8_out, p->d_rgb8[p->cur].get(), p->n_px() * 3, hipMemcpyDeviceToHost));
    unsigned long long changed = 0;
    HIP_OK(hipMemcpy(&changed, p->d_changed.get(), sizeof(changed), hipMemcpyDeviceToHost));
    if (changed_px_out) *changed_px_out = changed;
    return 0;
}
int rt_progressive_resolve_rgb8(void* frame, uint8_t* rgb8_out, uint64_t* changed_px_out) {
    if (!frame || !rgb8_out) return set_error("null argument");
    {   // passes enqueued on the caller's streams (rt_progressive_add_async) belong to the image
        DeviceGuard guard(((Progressive*)frame)->device);
        HIP_OK(hipDeviceSynchronize());
    }
    if (rt_progressive_resolve_rgb8_device(frame, nullptr, nullptr)) return -1;
    return rt_progressive_copy_rgb8(frame, rgb8_out, changed_px_out);
}
int rt_progressive_read_sum(void* frame, double* rgb_sum_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !rgb_sum_out) return set_error("null argument");
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rgb_sum_out, p->d_sum.get(), p->sum_bytes(), hipMemcpyDeviceToHost));
    return 0;
}
static int progressive_restart(Progressive* p, const double* rgb_sum, uint64_t samples_done) {
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());                 // nothing of the old frame may still be adding to the buffer
    if (rgb_sum) HIP_OK(hipMemcpy(p->d_sum.get(), rgb_sum, p->sum_bytes(), hipMemcpyHostToDevice));
    else { HIP_OK(hipMemsetAsync(p->d_sum.get(), 0, p->sum_bytes(), nullptr)); HIP_OK(hipStreamSynchronize(nullptr)); }
    p->done = samples_done; p->have_prev = false; p->resolved = false;       // the next resolve is a first one: every pixel counts as changed
    if (p->moments) {
        // a frame of sums alone (rt_progressive_load_sum) holds samples the second moments know nothing of: they are invalid until a reset
        // or rt_progressive_load_moments; a reset starts them again.  The pass frame is +0.0 either way (a pass that failed half-way too).
        p->moments_valid = rgb_sum == nullptr;
        p->passes = 0;
        HIP_OK(hipMemsetAsync(p->d_sq.get(), 0, p->sum_bytes(), nullptr));
        HIP_OK(hipMemsetAsync(p->d_pass.get(), 0, p->sum_bytes(), nullptr));
        if (p->adaptive) {                              // every pixel holds samples_done samples of 0 passes (the loads set the passes afterwards)
            HIP_OK(hipMemsetD32Async((hipDeviceptr_t)p->d_cnt.get(), (int)(uint32_t)samples_done, p->n_px(), nullptr));
            HIP_OK(hipMemsetD32Async((hipDeviceptr_t)p->d_pas.get(), 0, p->n_px(), nullptr));
            p->uniform = true; p->total = (uint64_t)p->n_px() * samples_done;
        }
        HIP_OK(hipStreamSynchronize(nullptr));
    }
    return 0;
}
int rt_progressive_load_sum(void* frame, const double* rgb_sum, uint64_t samples_done) {
    Progressive* p = (Progressive*)frame;
    if (!rgb_sum) return set_error("null argument");
    if (samples_done > 0xFFFFFFFFull) return set_error("samples_done must be <= 2^32 - 1 (the sample field of a path's RNG key is 32 bits, csrc/rt_rng.h)");
    if (!p) return set_error("null argument");
    if (adaptive_needs_uniform(p, "rt_progressive_load_sum")) return -1;
    if (samples_done == 0) {                        // 0 samples is the empty frame and nothing else (-0.0 is not empty either: its bits are a checkpoint's)
        const size_t n = p->n_px() * 3;
        for (size_t i = 0; i < n; i++) { uint64_t w; std::memcpy(&w, rgb_sum + i, sizeof(w)); if (w != 0) return set_error("samples_done = 0 with a non-zero frame: a checkpoint is a sum AND its sample count"); }
    }
    return progressive_restart(p, rgb_sum, samples_done);
}
int rt_progressive_reset(void* frame) {
    Progressive* p = (Progressive*)frame;
    if (!p) return set_error("null argument");
    if (p->sc) p->scene_version = p->sc->s.version;     // a new frame, of the scene as it is now
    p->guide_valid = false;                             // ... and so is its denoising guide, rebuilt when it is next needed
    p->albedo_samples = 0;                              // ... and its albedo sums
    p->hist_valid = false; p->hist_px = 0;              // ... and the history of the views before it (rt_progressive_set_view keeps it)
    p->hist_var_valid = false;                          // ... with its variance
    return progressive_restart(p, nullptr, 0);
}

// ---------------------------------------------------------------- moments (csrc/rt_moments.h: the specification; rt_moments.hip: the kernels)
int rt_moments_merge_device(void* d_pass_sum, uint64_t n_samples, void* d_rgb_sum, void* d_sq_sum, uint64_t n_doubles, void* hip_stream) {
    if (!d_pass_sum || !d_rgb_sum || !d_sq_sum) return set_error("null argument");
    if (refused(moments_merge_check(n_samples))) return -1;
    if ((((uintptr_t)d_pass_sum | (uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum) & 7u) != 0u) return set_error("d_pass_sum, d_rgb_sum and d_sq_sum must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_moments_merge((double*)d_pass_sum, n_samples, (double*)d_rgb_sum, (double*)d_sq_sum, n_doubles, hip_stream));
    return 0;
}
int rt_moments_error_device(const void* d_rgb_sum, const void* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H,
                            void* d_e2_out, double tau, void* d_stats_out, void* hip_stream) {
    if (!d_rgb_sum || !d_sq_sum) return set_error("null argument");
    std::string problem = moments_error_check(samples, passes, W, H);
    if (problem.empty() && d_stats_out) problem = moments_tau_check(tau);
    if (!problem.empty()) return set_error(problem);
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum | (uintptr_t)d_e2_out | (uintptr_t)d_stats_out) & 7u) != 0u) return set_error("d_rgb_sum, d_sq_sum, d_e2_out and d_stats_out must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    if (!d_e2_out && !d_stats_out) return 0;                    // nothing asked for
    if (d_stats_out) HIP_OK(hipMemsetAsync(d_stats_out, 0, MOMENTS_STATS_WORDS * sizeof(uint64_t), (hipStream_t)hip_stream));
    HIP_OK((hipError_t)launch_moments_error((const double*)d_rgb_sum, (const double*)d_sq_sum, samples, passes, W * H, (double*)d_e2_out, tau * tau,
                                            (unsigned long long*)d_stats_out, hip_stream));
    return 0;
}
int rt_progressive_enable_moments(void* frame) {
    Progressive* p = (Progressive*)frame;
    if (!p) return set_error("null argument");
    if (p->moments) return 0;
    if (p->done != 0) return set_error("moments can only be enabled while the frame holds 0 samples (the second moments must cover every sample of the sums): rt_progressive_reset first");
    DeviceGuard guard(p->device);
    const size_t bytes = p->sum_bytes();
    hipError_t e = p->d_sq.ensure(bytes);
    if (e == hipSuccess) e = p->d_pass.ensure(bytes);
    if (e == hipSuccess) e = p->d_mstats.ensure(MOMENTS_STATS_WORDS * sizeof(uint64_t));
    if (e == hipSuccess) e = p->ev_merged.ensure(hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_sq.get(), 0, bytes, nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_pass.get(), 0, bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        p->d_sq.reset(); p->d_pass.reset(); p->d_mstats.reset(); p->ev_merged.reset();
        return set_error(std::string("rt_progressive_enable_moments: ") + hipGetErrorString(e));
    }
    p->moments = true; p->moments_valid = true; p->merge_recorded = false; p->passes = 0;
    return 0;
}
static int moments_frame(Progressive* p) {
    if (!p) return set_error("null argument");
    if (!p->moments) return set_error("this progressive frame has no moments (rt_progressive_enable_moments, while it holds 0 samples)");
    return 0;
}
// what the three error calls check: moments that describe the sums, and two passes
static int moments_error_ready(Progressive* p) {
    if (moments_frame(p)) return -1;
    if (!p->moments_valid) return set_error("the moments of this frame are invalid: rt_progressive_load_sum loaded sums whose second moments are unknown (rt_progressive_reset or rt_progressive_load_moments)");
    return refused(moments_error_check(p->done, p->passes, p->W, p->H));
}
int rt_progressive_passes(void* frame, uint64_t* passes_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !passes_out) return set_error("null argument");
    *passes_out = p->moments ? p->passes : 0u;
    return 0;
}
int rt_progressive_read_moments(void* frame, double* sq_sum_out) {
    Progressive* p = (Progressive*)frame;
    if (!sq_sum_out) return set_error("null argument");
    if (moments_frame(p)) return -1;
    if (!p->moments_valid) return set_error("the moments of this frame are invalid: rt_progressive_load_sum loaded sums whose second moments are unknown (rt_progressive_reset or rt_progressive_load_moments)");
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(sq_sum_out, p->d_sq.get(), p->sum_bytes(), hipMemcpyDeviceToHost));
    return 0;
}
int rt_progressive_load_moments(void* frame, const double* rgb_sum, const double* sq_sum, uint64_t samples_done, uint64_t passes) {
    Progressive* p = (Progressive*)frame;
    if (!rgb_sum || !sq_sum) return set_error("null argument");
    if (moments_frame(p)) return -1;
    if (adaptive_needs_uniform(p, "rt_progressive_load_moments")) return -1;
    if (samples_done > 0xFFFFFFFFull) return set_error("samples_done must be <= 2^32 - 1 (the sample field of a path's RNG key is 32 bits, csrc/rt_rng.h)");
    if (passes > samples_done) return set_error("passes must be <= samples_done: a pass holds at least one sample");
    if ((samples_done == 0) != (passes == 0)) return set_error("samples_done = 0 and passes = 0 go together: a checkpoint is the sums, the second moments, the sample count AND the pass count");
    if (samples_done == 0) {
        const size_t n = p->n_px() * 3;
        for (size_t i = 0; i < n; i++) {
            uint64_t w, v; std::memcpy(&w, rgb_sum + i, sizeof(w)); std::memcpy(&v, sq_sum + i, sizeof(v));
            if ((w | v) != 0) return set_error("samples_done = 0 with a non-zero frame: a checkpoint is the sums, the second moments, the sample count AND the pass count");
        }
    }
    if (progressive_restart(p, rgb_sum, samples_done)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipMemcpy(p->d_sq.get(), sq_sum, p->sum_bytes(), hipMemcpyHostToDevice));
    if (p->adaptive) { HIP_OK(hipMemsetD32Async((hipDeviceptr_t)p->d_pas.get(), (int)(uint32_t)passes, p->n_px(), nullptr)); HIP_OK(hipStreamSynchronize(nullptr)); }
    p->passes = passes; p->moments_valid = true;
    return 0;
}
// e2 into d_e2_out and / or the statistics of tau2 into d_stats_out, from the frame's own sums: per-pixel counts on an adaptive frame
static int frame_error_enqueue(Progressive* p, double* d_e2_out, double tau2, unsigned long long* d_stats_out, void* stream) {
    if (p->adaptive)
        HIP_OK((hipError_t)launch_adaptive_error(p->d_sum.as<double>(), p->d_sq.as<double>(), p->d_cnt.as<uint32_t>(), p->d_pas.as<uint32_t>(), (uint32_t)p->n_px(),
                                                 d_e2_out, tau2, d_stats_out, stream));
    else
        HIP_OK((hipError_t)launch_moments_error(p->d_sum.as<double>(), p->d_sq.as<double>(), p->done, p->passes, (uint32_t)p->n_px(), d_e2_out, tau2, d_stats_out, stream));
    return 0;
}
int rt_progressive_error_map_device(void* frame, void** d_e2_out, void* hip_stream) {
    Progressive* p = (Progressive*)frame;
    if (moments_error_ready(p)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(p->d_e2.ensure(p->n_px() * sizeof(double)));
    if (frame_error_enqueue(p, p->d_e2.as<double>(), 0.0, nullptr, hip_stream)) return -1;
    if (d_e2_out) *d_e2_out = p->d_e2.get();
    return 0;
}
int rt_progressive_error_map(void* frame, double* e2_out) {
    Progressive* p = (Progressive*)frame;
    if (!e2_out) return set_error("null argument");
    if (moments_error_ready(p)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());                 // passes enqueued on the caller's streams belong to the estimate
    if (rt_progressive_error_map_device(frame, nullptr, nullptr)) return -1;
    HIP_OK(hipMemcpy(e2_out, p->d_e2.get(), p->n_px() * sizeof(double), hipMemcpyDeviceToHost));      // (waits for the kernel: the null stream)
    return 0;
}
int rt_progressive_error_stats(void* frame, double tau, uint64_t stats_out[4]) {
    Progressive* p = (Progressive*)frame;
    if (!stats_out) return set_error("null argument");
    if (moments_error_ready(p)) return -1;
    if (refused(moments_tau_check(tau))) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemsetAsync(p->d_mstats.get(), 0, MOMENTS_STATS_WORDS * sizeof(uint64_t), nullptr));
    if (frame_error_enqueue(p, nullptr, tau * tau, p->d_mstats.as<unsigned long long>(), nullptr)) return -1;
    HIP_OK(hipMemcpy(stats_out, p->d_mstats.get(), MOMENTS_STATS_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}
// (4) of rt_moments.h
int rt_moments_variance_device(const void* d_rgb_sum, const void* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H, void* d_var_out, void* hip_stream) {
    if (!d_rgb_sum || !d_sq_sum || !d_var_out) return set_error("null argument");
    if (refused(moments_error_check(samples, passes, W, H))) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum | (uintptr_t)d_var_out) & 7u) != 0u) return set_error("d_rgb_sum, d_sq_sum and d_var_out must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_moments_variance((const double*)d_rgb_sum, (const double*)d_sq_sum, samples, passes, (uint64_t)W * H * 3u, (double*)d_var_out, hip_stream));
    return 0;
}
// ... on the frame's own sums, into the frame's own variance frame, on `stream`
static int progressive_variance_enqueue(Progressive* p, hipStream_t stream) {
    HIP_OK(p->d_var.ensure(p->sum_bytes()));
    HIP_OK((hipError_t)launch_moments_variance(p->d_sum.as<double>(), p->d_sq.as<double>(), p->done, p->passes, (uint64_t)p->n_px() * 3u, p->d_var.as<double>(), stream));
    return 0;
}
int rt_progressive_variance(void* frame, double* var_out) {
    Progressive* p = (Progressive*)frame;
    if (!var_out) return set_error("null argument");
    if (adaptive_needs_uniform(p, "rt_progressive_variance")) return -1;
    if (moments_error_ready(p)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());                 // passes enqueued on the caller's streams belong to the estimate
    if (progressive_variance_enqueue(p, nullptr)) return -1;
    HIP_OK(hipMemcpy(var_out, p->d_var.get(), p->sum_bytes(), hipMemcpyDeviceToHost));      // (waits for the kernel: the null stream)
    return 0;
}

// ---------------------------------------------------------------- adaptive frames (csrc/rt_adaptive.h: the specification; rt_adaptive.hip: the kernels)
int rt_render_pixels_device(rt_scene* sc, const rt_camera* cam, const double bg[3], uint32_t W, uint32_t H, uint32_t n_samples, uint32_t max_depth,
                            uint64_t seed, uint32_t flags, const void* d_list, uint32_t n_list, const void* d_counts, void* d_out, size_t d_out_bytes,
                            void* hip_stream) {
    if (!sc || !cam || !bg) return set_error("null argument");
    if (W < 2 || H < 2) return set_error("W and H must be >= 2 (u,v divide by W-1 and H-1, src/main.rs:817-818)");
    if ((uint64_t)W * H > 0x7FFFFFFFull) return set_error("frame too large: W*H must be <= 2^31 - 1 (per-path RNG keys, csrc/rt_rng.h)");
    if (n_samples == 0) return set_error("n_samples must be >= 1");
    if (flags & ~(uint32_t)(RT_STOP_ON_ZERO | RT_ISOTROPIC_SCATTER))
        return set_error("pixel-list passes take RT_STOP_ON_ZERO and RT_ISOTROPIC_SCATTER only: they run in f64 and in the reference's traversal order (RT_F32 and every other flag: not supported)");
    if (!d_out || (!d_list && n_list)) return set_error("null argument");
    if (n_list > W * H) return set_error("n_list must be <= W * H: the list names each pixel at most once");
    if (d_out_bytes < (size_t)W * H * 3u * sizeof(double)) return set_error("output buffer too small for W * H * 3 doubles (24 bytes per pixel)");
    if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_list & 3u) || ((uintptr_t)d_counts & 3u)) return set_error("d_out must be 8-byte aligned, d_list and d_counts 4-byte aligned");
    if (need_device_and_flat(sc->s)) return -1;
    if (n_list == 0) return 0;
    return launch_pixel_list(sc->s, cam, bg, W, H, n_samples, max_depth, seed, flags, d_list, n_list, d_counts, d_out, (hipStream_t)hip_stream);
}
int rt_adaptive_error_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                             void* d_e2_out, double tau, void* d_stats_out, void* hip_stream) {
    if (!d_rgb_sum || !d_sq_sum || !d_counts || !d_passes) return set_error("null argument");
    std::string problem = adaptive_frame_check(W, H);
    if (problem.empty() && d_stats_out) problem = moments_tau_check(tau);
    if (!problem.empty()) return set_error(problem);
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum | (uintptr_t)d_e2_out | (uintptr_t)d_stats_out) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_passes) & 3u) != 0u)
        return set_error("d_rgb_sum, d_sq_sum, d_e2_out and d_stats_out must be 8-byte aligned, d_counts and d_passes 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    if (!d_e2_out && !d_stats_out) return 0;                    // nothing asked for
    if (d_stats_out) HIP_OK(hipMemsetAsync(d_stats_out, 0, MOMENTS_STATS_WORDS * sizeof(uint64_t), (hipStream_t)hip_stream));
    HIP_OK((hipError_t)launch_adaptive_error((const double*)d_rgb_sum, (const double*)d_sq_sum, (const uint32_t*)d_counts, (const uint32_t*)d_passes, W * H,
                                             (double*)d_e2_out, tau * tau, (unsigned long long*)d_stats_out, hip_stream));
    return 0;
}
size_t rt_adaptive_select_workspace_bytes(uint32_t W, uint32_t H) { return adaptive_select_workspace_bytes((uint64_t)W * H); }
int rt_adaptive_select_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                              uint32_t n_samples, double tau, uint64_t max_samples, uint32_t spread, void* d_list_out, void* d_n_list_out,
                              void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_rgb_sum || !d_sq_sum || !d_counts || !d_passes || !d_list_out || !d_n_list_out || !d_workspace) return set_error("null argument");
    if (refused(adaptive_select_check(W, H, n_samples, tau, max_samples, spread))) return -1;
    if (workspace_bytes < rt_adaptive_select_workspace_bytes(W, H)) return set_error("adaptive: workspace too small: rt_adaptive_select_workspace_bytes(W, H) bytes are needed");
    if (query_aligned(d_workspace, "d_workspace")) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_passes | (uintptr_t)d_list_out | (uintptr_t)d_n_list_out) & 3u) != 0u)
        return set_error("d_rgb_sum and d_sq_sum must be 8-byte aligned, d_counts, d_passes, d_list_out and d_n_list_out 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_adaptive_select((const double*)d_rgb_sum, (const double*)d_sq_sum, (const uint32_t*)d_counts, (const uint32_t*)d_passes, W, H, n_samples,
                                              tau * tau, max_samples, spread, (uint32_t*)d_list_out, (uint32_t*)d_n_list_out, d_workspace, hip_stream));
    return 0;
}
int rt_adaptive_merge_device(void* d_pass_sum, uint32_t n_samples, void* d_rgb_sum, void* d_sq_sum, void* d_counts, void* d_passes, const void* d_list,
                             uint32_t n_list, void* hip_stream) {
    if (!d_pass_sum || !d_rgb_sum || !d_sq_sum || !d_counts || !d_passes || (!d_list && n_list)) return set_error("null argument");
    if (n_samples == 0u) return set_error("adaptive: n_samples must be >= 1 (a pass's square is divided by its sample count)");
    if (n_list > 0x7FFFFFFFu) return set_error("adaptive: n_list must be <= 2^31 - 1");
    if ((((uintptr_t)d_pass_sum | (uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_passes | (uintptr_t)d_list) & 3u) != 0u)
        return set_error("d_pass_sum, d_rgb_sum and d_sq_sum must be 8-byte aligned, d_counts, d_passes and d_list 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_adaptive_merge((double*)d_pass_sum, n_samples, (double*)d_rgb_sum, (double*)d_sq_sum, (uint32_t*)d_counts, (uint32_t*)d_passes,
                                             (const uint32_t*)d_list, n_list, nullptr, hip_stream));
    return 0;
}
int rt_adaptive_resolve_rgb8_device(const void* d_rgb_sum, const void* d_counts, uint32_t W, uint32_t H, const void* d_rgb8_prev, void* d_rgb8_out,
                                    void* d_changed_px_out, void* hip_stream) {
    if (!d_rgb_sum || !d_counts || !d_rgb8_out) return set_error("null argument");
    if (refused(adaptive_frame_check(W, H))) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_changed_px_out) & 7u) != 0u || ((uintptr_t)d_counts & 3u) != 0u) return set_error("d_rgb_sum and d_changed_px_out must be 8-byte aligned, d_counts 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_adaptive_resolve((const double*)d_rgb_sum, (const uint32_t*)d_counts, (const uint8_t*)d_rgb8_prev, (uint8_t*)d_rgb8_out,
                                               (unsigned long long*)d_changed_px_out, W * H, hip_stream));
    return 0;
}

static int adaptive_frame(Progressive* p) {
    if (!p) return set_error("null argument");
    if (!p->adaptive) return set_error("this progressive frame is not adaptive (rt_progressive_enable_adaptive, on a frame with moments while it holds 0 samples)");
    return 0;
}
int rt_progressive_enable_adaptive(void* frame) {
    Progressive* p = (Progressive*)frame;
    if (moments_frame(p)) return -1;
    if (p->adaptive) return 0;
    if (p->done != 0) return set_error("adaptive sampling can only be enabled while the frame holds 0 samples (the counts must cover every sample of the sums): rt_progressive_reset first");
    if (p->flags & ~(uint32_t)(RT_STOP_ON_ZERO | RT_ISOTROPIC_SCATTER))
        return set_error("adaptive frames take RT_STOP_ON_ZERO and RT_ISOTROPIC_SCATTER only: the pixel-list kernel runs in f64 and in the reference's traversal order (RT_F32 and every other flag: not supported)");
    DeviceGuard guard(p->device);
    const size_t n = p->n_px();
    hipError_t e = p->d_cnt.ensure(n * sizeof(uint32_t));
    if (e == hipSuccess) e = p->d_pas.ensure(n * sizeof(uint32_t));
    if (e == hipSuccess) e = p->d_list.ensure(n * sizeof(uint32_t));
    if (e == hipSuccess) e = p->d_words.ensure(2 * sizeof(uint32_t));
    if (e == hipSuccess) e = p->d_sel_ws.ensure(rt_adaptive_select_workspace_bytes(p->W, p->H));
    if (e == hipSuccess) e = hipMemsetAsync(p->d_cnt.get(), 0, n * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_pas.get(), 0, n * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_words.get(), 0, 2 * sizeof(uint32_t), nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        p->d_cnt.reset(); p->d_pas.reset(); p->d_list.reset(); p->d_words.reset(); p->d_sel_ws.reset();
        return set_error(std::string("rt_progressive_enable_adaptive: ") + hipGetErrorString(e));
    }
    p->adaptive = true; p->uniform = true; p->total = 0;
    return 0;
}
// one pass of n samples over the n_list pixels of the frame's list (already in d_list) through the list kernel, merged, waited for
static int adaptive_list_pass(Progressive* p, uint32_t n, uint32_t n_list) {
    const size_t n_px = p->n_px();
    uint32_t* words = p->d_words.as<uint32_t>();                // [0] the list's length, [1] the largest count behind the merge
    if (p->merge_recorded) HIP_OK(hipStreamWaitEvent(nullptr, p->ev_merged.get(), 0));
    if (rt_render_pixels_device(p->sc, &p->cam, p->bg, p->W, p->H, n, p->max_depth, p->seed, p->flags, p->d_list.get(), n_list, p->d_cnt.get(), p->d_pass.get(),
                                p->sum_bytes(), nullptr)) return -1;
    HIP_OK(hipMemsetAsync(words + 1, 0, sizeof(uint32_t), nullptr));
    HIP_OK((hipError_t)launch_adaptive_merge(p->d_pass.as<double>(), n, p->d_sum.as<double>(), p->d_sq.as<double>(), p->d_cnt.as<uint32_t>(), p->d_pas.as<uint32_t>(),
                                             p->d_list.as<uint32_t>(), n_list, words + 1, nullptr));
    HIP_OK(hipEventRecord(p->ev_merged.get(), nullptr));
    p->merge_recorded = true;
    uint32_t largest = 0;
    HIP_OK(hipMemcpy(&largest, words + 1, sizeof(largest), hipMemcpyDeviceToHost));       // (waits for the pass: the null stream)
    if (n_list != n_px) p->uniform = false;
    if (largest > p->done) p->done = largest;
    p->passes++; p->total += (uint64_t)n_list * n;
    return 0;
}
// rt_progressive_add on an adaptive frame whose counts differ: a pass over all pixels through the list kernel
static int adaptive_pass_over_all(Progressive* p, uint32_t n, double* samples_out) {
    if (samples_out) return set_error("rt_progressive_add: samples_out is not available on an adaptive frame whose pixels hold different sample counts");
    DeviceGuard guard(p->device);
    const size_t n_px = p->n_px();
    std::vector<uint32_t> all(n_px);
    for (size_t i = 0; i < n_px; i++) all[i] = (uint32_t)i;
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(p->d_list.get(), all.data(), n_px * sizeof(uint32_t), hipMemcpyHostToDevice));
    return adaptive_list_pass(p, n, (uint32_t)n_px);
}
int rt_progressive_add_adaptive(void* frame, uint32_t n, double tau, uint64_t max_samples, uint32_t spread, uint64_t info_out[4]) {
    Progressive* p = (Progressive*)frame;
    if (!info_out) return set_error("null argument");
    if (adaptive_frame(p)) return -1;
    if (max_samples == 0u) max_samples = ADAPTIVE_MAX_SAMPLES;
    if (refused(adaptive_select_check(p->W, p->H, n, tau, max_samples, spread))) return -1;
    if (frame_scene_current(p)) return -1;
    if (!p->moments_valid) return set_error("the moments of this frame are invalid: rt_progressive_load_sum loaded sums whose second moments are unknown (rt_progressive_reset or rt_progressive_load_adaptive)");
    DeviceGuard guard(p->device);
    const size_t n_px = p->n_px();
    uint32_t* words = p->d_words.as<uint32_t>();
    HIP_OK((hipError_t)launch_adaptive_select(p->d_sum.as<double>(), p->d_sq.as<double>(), p->d_cnt.as<uint32_t>(), p->d_pas.as<uint32_t>(), p->W, p->H, n,
                                              tau * tau, max_samples, spread, p->d_list.as<uint32_t>(), words, p->d_sel_ws.get(), nullptr));
    uint32_t n_list = 0;
    HIP_OK(hipMemcpy(&n_list, words, sizeof(n_list), hipMemcpyDeviceToHost));             // (waits for the selection: the null stream)
    info_out[0] = n_list; info_out[1] = (uint64_t)n_list * n; info_out[2] = p->total; info_out[3] = 0;
    if (n_list == 0u) return 0;                                  // nothing listed: the stop condition
    if (n_list == n_px && p->uniform) {                          // still a uniform frame: the frames' own kernels are the fast ones
        if (progressive_pass(p, n, nullptr, nullptr, true)) return -1;
        HIP_OK(hipStreamSynchronize(nullptr));
    } else {
        if (adaptive_list_pass(p, n, n_list)) return -1;
        info_out[3] = 1;
    }
    info_out[2] = p->total;
    return 0;
}
int rt_progressive_read_counts(void* frame, uint32_t* counts_out, uint32_t* passes_out) {
    Progressive* p = (Progressive*)frame;
    if (adaptive_frame(p)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    if (counts_out) HIP_OK(hipMemcpy(counts_out, p->d_cnt.get(), p->n_px() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (passes_out) HIP_OK(hipMemcpy(passes_out, p->d_pas.get(), p->n_px() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
int rt_progressive_load_adaptive(void* frame, const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes) {
    Progressive* p = (Progressive*)frame;
    if (!rgb_sum || !sq_sum || !counts || !passes) return set_error("null argument");
    if (adaptive_frame(p)) return -1;
    const size_t n_px = p->n_px();
    uint32_t most = 0, most_b = 0; uint64_t total = 0; bool uniform = true;
    for (size_t i = 0; i < n_px; i++) {
        if (passes[i] > counts[i]) return set_error("passes must be <= counts for every pixel: a pass holds at least one sample");
        if (counts[i] == 0u)
            for (size_t k = 0; k < 3; k++) {
                uint64_t w, v; std::memcpy(&w, rgb_sum + 3 * i + k, sizeof(w)); std::memcpy(&v, sq_sum + 3 * i + k, sizeof(v));
                if ((w | v) != 0) return set_error("a pixel with count 0 that is not all zero: a checkpoint is the sums, the second moments AND the counts");
            }
        if (counts[i] != counts[0] || passes[i] != passes[0]) uniform = false;
        if (counts[i] > most) most = counts[i];
        if (passes[i] > most_b) most_b = passes[i];
        total += counts[i];
    }
    if (progressive_restart(p, rgb_sum, most)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipMemcpy(p->d_sq.get(), sq_sum, p->sum_bytes(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(p->d_cnt.get(), counts, n_px * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(p->d_pas.get(), passes, n_px * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->passes = most_b; p->moments_valid = true; p->uniform = uniform; p->total = total;
    return 0;
}

// ---------------------------------------------------------------- denoiser (csrc/rt_denoise.h: the specification; rt_denoise.hip: the kernels)
size_t rt_denoise_workspace_bytes(uint32_t W, uint32_t H) { return (size_t)W * H * DENOISE_WORKSPACE_BYTES_PER_PX; }

// The launches of one run, enqueued on `stream`: pack (the colour always; the guide when d_hits is given — a progressive frame brings a guide
// it packed earlier), then the iterations, alternating between the workspace's two colour frames, the last one writing sums to d_out.
// The workspace is {colour A, colour B, guide}: 32 + 32 + 64 bytes per pixel.
// `marks` (rt_debug_denoise_ms only): iterations + 2 events, recorded in front of every launch and behind the last.
static int denoise_enqueue(const double* d_sum, uint64_t samples, const double* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                           const double sigma[3], uint32_t flags, double* d_out, void* d_workspace, hipStream_t stream, hipEvent_t* marks = nullptr) {
    const size_t n = (size_t)W * H;
    double* color[2] = {(double*)d_workspace, (double*)d_workspace + n * DENOISE_COLOR_DOUBLES};
    double* guide = (double*)d_workspace + 2u * n * DENOISE_COLOR_DOUBLES;
    double inv[3];
    denoise_inverse_squares(sigma, inv);
    if (marks) HIP_OK(hipEventRecord(marks[0], stream));
    HIP_OK((hipError_t)launch_denoise_pack(d_sum, samples, d_hits, flags, color[0], guide, (uint32_t)n, stream));
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1u == iterations;
        if (marks) HIP_OK(hipEventRecord(marks[i + 1u], stream));
        HIP_OK((hipError_t)launch_denoise_filter(color[i & 1u], guide, last ? nullptr : color[(i + 1u) & 1u], last ? d_out : nullptr, W, H, 1u << i,
                                                 inv[0] * (double)(1ull << (2u * i)), inv[1], inv[2], samples, stream));
    }
    if (marks) HIP_OK(hipEventRecord(marks[iterations + 1u], stream));
    return 0;
}
int rt_denoise_device(const void* d_rgb_sum, uint64_t samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                      const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_rgb_sum || !d_hits || !sigma || !d_rgb_sum_out || !d_workspace) return set_error("null argument");
    if (refused(denoise_check(samples, W, H, iterations, sigma, flags))) return -1;
    if (workspace_bytes < rt_denoise_workspace_bytes(W, H)) return set_error("denoise: workspace too small: rt_denoise_workspace_bytes(W, H) = 128 bytes per pixel are needed");
    if (query_aligned(d_hits, "d_hits") || query_aligned(d_workspace, "d_workspace")) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_rgb_sum_out) & 7u) != 0u) return set_error("d_rgb_sum and d_rgb_sum_out must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    return denoise_enqueue((const double*)d_rgb_sum, samples, (const double*)d_hits, W, H, iterations, sigma, flags, (double*)d_rgb_sum_out,
                           d_workspace, (hipStream_t)hip_stream);
}
int rt_denoise(const double* rgb_sum, uint64_t samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations,
               const double sigma[3], uint32_t flags, double* rgb_sum_out) {
    if (!rgb_sum || !hits || !sigma || !rgb_sum_out) return set_error("null argument");
    if (refused(denoise_check(samples, W, H, iterations, sigma, flags))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), ws_bytes = rt_denoise_workspace_bytes(W, H);
    DeviceBuffer d_sum, d_hits, d_ws;
    if (upload(d_sum, rgb_sum, sum_bytes) || upload(d_hits, hits, n * DENOISE_HIT_DOUBLES * sizeof(double))) return -1;
    HIP_OK(d_ws.alloc(ws_bytes));
    if (rt_denoise_device(d_sum.get(), samples, d_hits.get(), W, H, iterations, sigma, flags, d_sum.get(), d_ws.get(), ws_bytes, nullptr)) return -1;
    HIP_OK(hipMemcpy(rgb_sum_out, d_sum.get(), sum_bytes, hipMemcpyDeviceToHost));       // (waits for the kernels: the null stream)
    return 0;
}
int rt_debug_denoise_ms(const void* d_rgb_sum, uint64_t samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                        const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, float* ms_out) {
    if (!ms_out) return set_error("null argument");
    // (the arguments are rt_denoise_device's and are checked there; nothing is recorded for a refused call)
    return timed_between_marks((iterations <= DENOISE_MAX_ITERATIONS ? iterations : 0u) + 2u, ms_out, [&](hipEvent_t* marks) {
        if (!d_rgb_sum || !d_hits || !sigma || !d_rgb_sum_out || !d_workspace) return set_error("null argument");
        if (rt_denoise_device(d_rgb_sum, samples, d_hits, W, H, iterations, sigma, flags, d_rgb_sum_out, d_workspace, workspace_bytes, nullptr)) return -1;     // the checks, and a warm run
        return denoise_enqueue((const double*)d_rgb_sum, samples, (const double*)d_hits, W, H, iterations, sigma, flags, (double*)d_rgb_sum_out, d_workspace, nullptr, marks);
    });
}
// the guide records of a view of the frame's scene: sample 0's camera hits or, with guide_samples > 1, the averaged record of samples
// [0, guide_samples) (rt_guide.h)
static int progressive_view_records(Progressive* p, const rt_camera* cam, uint64_t seed, void* d_hits, size_t hit_bytes) {
    if (p->guide_samples == 1u) return rt_query_camera_device(p->sc, cam, p->W, p->H, 0u, seed, 0u, nullptr, d_hits, hit_bytes, nullptr);
    return rt_query_camera_guide_device(p->sc, cam, p->W, p->H, 0u, p->guide_samples, seed, 0u, d_hits, hit_bytes, nullptr, 0u, nullptr);
}
// ... and with the chain on (rt_progressive_set_guide_chain) the guide a denoised resolve filters with: the chain records of samples
// [0, guide_samples) reduced as the averaged guide is, and the frame's albedo sums from the same launch.  rt_progressive_set_view does not
// come here: it reprojects with progressive_view_records' first hits, whose points are seen directly from the camera.
static int progressive_chain_records(Progressive* p, void* d_hits, size_t hit_bytes) {
    HIP_OK(p->d_alb_sum.ensure(p->sum_bytes()));
    p->albedo_samples = 0; p->albedo_chain = false;
    if (rt_query_camera_chain_guide_device(p->sc, &p->cam, p->W, p->H, 0u, p->guide_samples, p->seed, p->chain_links, p->chain_fuzz, 0u, d_hits, hit_bytes,
                                           p->d_alb_sum.get(), p->sum_bytes(), nullptr, 0u, nullptr)) return -1;
    p->albedo_samples = p->guide_samples; p->albedo_chain = true; p->albedo_builds++;
    return 0;
}
// the image the denoised resolves write and the count word their resolve launch needs, allocated at the first of them
static int frame_image_ready(Progressive* p) {
    HIP_OK(p->d_dn_rgb8.ensure(p->n_px() * 3)); HIP_OK(p->d_dn_changed.ensure(sizeof(unsigned long long)));
    return 0;
}
// What every denoised resolve does before it filters: the checks, the frame's own buffers, and the packed guide — the records of this view
// (progressive_view_records), keyed for `flags` — in its place in the workspace.  allow_no_samples: the temporal resolve's, which has a
// history to show while the frame holds 0 samples.
static int progressive_denoise_prepare(Progressive* p, uint32_t iterations, const double sigma[3], uint32_t flags, bool allow_no_samples = false) {
    if (refused(denoise_check(p->done ? p->done : 1u, p->W, p->H, iterations, sigma, flags))) return -1;
    if (p->done == 0 && !allow_no_samples) return set_error("nothing to resolve: the frame holds 0 samples (format_color divides by the sample count, src/vec.rs:126)");
    HIP_OK(hipDeviceSynchronize());                 // passes enqueued on the caller's streams belong to the image
    const size_t n = p->n_px();
    const bool build = !p->guide_valid || p->guide_flags != flags;
    if (build && frame_scene_current(p, SCENE_GONE_NO_GUIDE)) return -1;
    HIP_OK(p->d_dn_ws.ensure(rt_denoise_workspace_bytes(p->W, p->H)));
    HIP_OK(p->d_dn_sum.ensure(p->sum_bytes()));
    if (frame_image_ready(p)) return -1;
    if (build) {                                    // the guide's records of this view, packed; the records themselves are not kept
        const size_t hit_bytes = n * DENOISE_HIT_DOUBLES * sizeof(double);
        DeviceBuffer d_hits;
        HIP_OK(d_hits.alloc(hit_bytes));
        p->guide_valid = false;
        if (p->chain_links ? progressive_chain_records(p, d_hits.get(), hit_bytes) : progressive_view_records(p, &p->cam, p->seed, d_hits.get(), hit_bytes)) return -1;
        HIP_OK((hipError_t)launch_denoise_pack(nullptr, 1u, d_hits.as<double>(), flags, nullptr, p->d_dn_ws.as<double>() + 2u * n * DENOISE_COLOR_DOUBLES, (uint32_t)n, nullptr));
        HIP_OK(hipStreamSynchronize(nullptr));
        p->guide_valid = true; p->guide_flags = flags; p->guide_builds++;
    }
    return 0;
}
int rt_progressive_set_guide_samples(void* frame, uint32_t n_samples) {
    Progressive* p = (Progressive*)frame;
    if (!p) return set_error("null argument");
    if (n_samples == 0u) return set_error("guide_samples must be >= 1 (1: the camera hits of sample 0; n: the averaged record of samples 0 .. n - 1)");
    if (n_samples != p->guide_samples) { p->guide_samples = n_samples; p->guide_valid = false; }
    return 0;
}
int rt_progressive_set_guide_chain(void* frame, uint32_t max_links, double max_fuzz) {
    Progressive* p = (Progressive*)frame;
    if (!p) return set_error("null argument");
    if (refused(chain_check(max_links, max_fuzz, 0u))) return -1;
    if (max_links != p->chain_links || (max_links != 0u && max_fuzz != p->chain_fuzz)) {
        p->guide_valid = false; p->albedo_samples = 0; p->albedo_chain = false;
    }
    p->chain_links = max_links; p->chain_fuzz = max_fuzz;
    return 0;
}
int rt_progressive_guide_chain_info(void* frame, uint32_t* max_links_out, double* max_fuzz_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !max_links_out || !max_fuzz_out) return set_error("null argument");
    *max_links_out = p->chain_links; *max_fuzz_out = p->chain_fuzz;
    return 0;
}
int rt_progressive_guide_info(void* frame, uint32_t* guide_samples_out, uint64_t* builds_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !guide_samples_out || !builds_out) return set_error("null argument");
    *guide_samples_out = p->guide_samples; *builds_out = p->guide_builds;
    return 0;
}
// ... and after: d_sums — every pixel's divided by its own count in d_counts, or all of them by `samples` — resolved into the denoised
// resolves' image and copied out
static int frame_resolve_out(Progressive* p, const double* d_sums, const uint32_t* d_counts, uint64_t samples, uint8_t* rgb8_out) {
    const size_t n = p->n_px();
    uint8_t* d_rgb8 = p->d_dn_rgb8.as<uint8_t>();
    unsigned long long* d_changed = p->d_dn_changed.as<unsigned long long>();
    HIP_OK(hipMemsetAsync(d_changed, 0, sizeof(unsigned long long), nullptr));
    if (d_counts) HIP_OK((hipError_t)launch_adaptive_resolve(d_sums, d_counts, nullptr, d_rgb8, d_changed, (uint32_t)n, nullptr));
    else HIP_OK(launch_resolve_rgb8(d_sums, samples, nullptr, d_rgb8, d_changed, (uint32_t)n, nullptr));
    HIP_OK(hipMemcpy(rgb8_out, d_rgb8, n * 3, hipMemcpyDeviceToHost));                   // (waits for the kernels: the null stream)
    return 0;
}
// The frame's sums filtered and resolved, into buffers of the frame's own: d_sum, the plain resolve's two images and its count stay as they are.
int rt_progressive_resolve_denoised_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !sigma || !rgb8_out) return set_error("null argument");
    if (adaptive_needs_uniform(p, "rt_progressive_resolve_denoised_rgb8")) return -1;
    DeviceGuard guard(p->device);
    if (progressive_denoise_prepare(p, iterations, sigma, flags)) return -1;
    if (denoise_enqueue(p->d_sum.as<double>(), p->done, nullptr, p->W, p->H, iterations, sigma, flags, p->d_dn_sum.as<double>(), p->d_dn_ws.get(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), nullptr, p->done, rgb8_out);
}

// ---------------------------------------------------------------- variance-guided denoising (csrc/rt_denoise_var.h: the specification; rt_denoise_var.hip: the kernels)
size_t rt_denoise_variance_workspace_bytes(uint32_t W, uint32_t H) { return rt_denoise_workspace_bytes(W, H); }

// The launches of one run on `stream`, in denoise_enqueue's workspace {colour A, colour B, guide}: the guide when d_hits is given, the pack
// into B, the prefilter of v from B to A, then the iterations alternating from A, the last one writing sums to d_out and v to d_var_out.
static int denoise_variance_enqueue(const double* d_sum, uint64_t samples, const double* d_var, const double* d_hits, uint32_t W, uint32_t H,
                                    uint32_t iterations, const double sigma[3], uint32_t flags, double* d_out, double* d_var_out, void* d_workspace,
                                    hipStream_t stream, hipEvent_t* marks = nullptr) {
    const size_t n = (size_t)W * H;
    double* color[2] = {(double*)d_workspace, (double*)d_workspace + n * DENOISE_COLOR_DOUBLES};
    double* guide = (double*)d_workspace + 2u * n * DENOISE_COLOR_DOUBLES;
    double inv[3];
    denoise_inverse_squares(sigma, inv);
    const double kv = sigma[0] * sigma[0];
    if (marks) HIP_OK(hipEventRecord(marks[0], stream));
    if (d_hits) HIP_OK((hipError_t)launch_denoise_pack(nullptr, samples, d_hits, flags, nullptr, guide, (uint32_t)n, stream));
    HIP_OK((hipError_t)launch_denoise_var_pack(d_sum, samples, d_var, color[1], (uint32_t)n, stream));
    if (marks) HIP_OK(hipEventRecord(marks[1], stream));
    HIP_OK((hipError_t)launch_denoise_var_prefilter(color[1], guide, color[0], W, H, stream));
    for (uint32_t i = 0; i < iterations; i++) {
        const bool last = i + 1u == iterations;
        if (marks) HIP_OK(hipEventRecord(marks[i + 2u], stream));
        HIP_OK((hipError_t)launch_denoise_var_filter(color[i & 1u], guide, last ? nullptr : color[(i + 1u) & 1u], last ? d_out : nullptr, last ? d_var_out : nullptr,
                                                     W, H, 1u << i, kv, inv[1], inv[2], samples, stream));
    }
    if (marks) HIP_OK(hipEventRecord(marks[iterations + 2u], stream));
    return 0;
}
int rt_denoise_variance_device(const void* d_rgb_sum, uint64_t samples, const void* d_var, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                               const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_var_out, void* d_workspace, size_t workspace_bytes,
                               void* hip_stream) {
    if (!d_rgb_sum || !d_var || !d_hits || !sigma || !d_rgb_sum_out || !d_workspace) return set_error("null argument");
    if (refused(denoise_variance_check(samples, W, H, iterations, sigma, flags))) return -1;
    if (workspace_bytes < rt_denoise_variance_workspace_bytes(W, H)) return set_error("denoise: workspace too small: rt_denoise_variance_workspace_bytes(W, H) = 128 bytes per pixel are needed");
    if (query_aligned(d_hits, "d_hits") || query_aligned(d_workspace, "d_workspace")) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_rgb_sum_out | (uintptr_t)d_var | (uintptr_t)d_var_out) & 7u) != 0u) return set_error("d_rgb_sum, d_var, d_rgb_sum_out and d_var_out must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    return denoise_variance_enqueue((const double*)d_rgb_sum, samples, (const double*)d_var, (const double*)d_hits, W, H, iterations, sigma, flags,
                                    (double*)d_rgb_sum_out, (double*)d_var_out, d_workspace, (hipStream_t)hip_stream);
}
int rt_denoise_variance(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H, uint32_t iterations,
                        const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out) {
    if (!rgb_sum || !var || !hits || !sigma || !rgb_sum_out) return set_error("null argument");
    if (refused(denoise_variance_check(samples, W, H, iterations, sigma, flags))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), ws_bytes = rt_denoise_variance_workspace_bytes(W, H);
    DeviceBuffer d_sum, d_var, d_hits, d_ws, d_vout;
    if (upload(d_sum, rgb_sum, sum_bytes) || upload(d_var, var, sum_bytes) || upload(d_hits, hits, n * DENOISE_HIT_DOUBLES * sizeof(double))) return -1;
    HIP_OK(d_ws.alloc(ws_bytes));
    if (var_out) HIP_OK(d_vout.alloc(n * sizeof(double)));
    if (rt_denoise_variance_device(d_sum.get(), samples, d_var.get(), d_hits.get(), W, H, iterations, sigma, flags, d_sum.get(), d_vout.get(), d_ws.get(), ws_bytes, nullptr)) return -1;
    HIP_OK(hipMemcpy(rgb_sum_out, d_sum.get(), sum_bytes, hipMemcpyDeviceToHost));       // (waits for the kernels: the null stream)
    if (var_out) HIP_OK(hipMemcpy(var_out, d_vout.get(), n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
int rt_debug_denoise_variance_ms(const void* d_rgb_sum, uint64_t samples, const void* d_var, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                                 const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, float* ms_out) {
    if (!ms_out) return set_error("null argument");
    // (the arguments are rt_denoise_variance_device's and are checked there; nothing is recorded for a refused call)
    return timed_between_marks((iterations <= DENOISE_MAX_ITERATIONS ? iterations : 0u) + 3u, ms_out, [&](hipEvent_t* marks) {
        if (rt_denoise_variance_device(d_rgb_sum, samples, d_var, d_hits, W, H, iterations, sigma, flags, d_rgb_sum_out, nullptr, d_workspace, workspace_bytes, nullptr)) return -1;     // the checks, and a warm run
        return denoise_variance_enqueue((const double*)d_rgb_sum, samples, (const double*)d_var, (const double*)d_hits, W, H, iterations, sigma, flags,
                                        (double*)d_rgb_sum_out, nullptr, d_workspace, nullptr, marks);
    });
}
// The frame's sums filtered under the guidance of the frame's own variance, and resolved; everything the other resolves own stays as it is.
int rt_progressive_resolve_denoised_variance_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !sigma || !rgb8_out) return set_error("null argument");
    if (adaptive_needs_uniform(p, "rt_progressive_resolve_denoised_variance_rgb8")) return -1;
    if (moments_error_ready(p)) return -1;
    if (refused(denoise_variance_check(p->done, p->W, p->H, iterations, sigma, flags))) return -1;
    DeviceGuard guard(p->device);
    if (progressive_denoise_prepare(p, iterations, sigma, flags)) return -1;
    if (progressive_variance_enqueue(p, nullptr)) return -1;
    if (denoise_variance_enqueue(p->d_sum.as<double>(), p->done, p->d_var.as<double>(), nullptr, p->W, p->H, iterations, sigma, flags, p->d_dn_sum.as<double>(),
                                 nullptr, p->d_dn_ws.get(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), nullptr, p->done, rgb8_out);
}

// ---------------------------------------------------------------- albedo-demodulated denoising (csrc/rt_albedo.h (2))
size_t rt_denoise_albedo_workspace_bytes(uint32_t W, uint32_t H) { return (size_t)W * H * DENOISE_ALBEDO_WORKSPACE_BYTES_PER_PX; }

// The launches of one run on `stream`: demodulate into d_x, the filter's own launches from d_x to d_out, remodulate d_out in place.
// d_out may be d_sum: the demodulate kernel has read it by the time anything is written there (stream order).
static int denoise_albedo_enqueue(const double* d_sum, uint64_t samples, const double* d_albedo_sum, uint64_t albedo_samples, const double* d_hits,
                                  uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* d_out,
                                  void* d_workspace, double* d_x, hipStream_t stream) {
    const uint64_t n = (uint64_t)W * H * 3u;
    HIP_OK((hipError_t)launch_albedo_demodulate(d_sum, d_albedo_sum, albedo_samples, d_x, n, stream));
    if (denoise_enqueue(d_x, samples, d_hits, W, H, iterations, sigma, flags, d_out, d_workspace, stream)) return -1;
    HIP_OK((hipError_t)launch_albedo_remodulate(d_out, d_albedo_sum, albedo_samples, n, stream));
    return 0;
}
int rt_denoise_albedo_device(const void* d_rgb_sum, uint64_t samples, const void* d_albedo_sum, uint64_t albedo_samples, const void* d_hits,
                             uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, void* d_rgb_sum_out,
                             void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_rgb_sum || !d_albedo_sum || !d_hits || !sigma || !d_rgb_sum_out || !d_workspace) return set_error("null argument");
    if (refused(denoise_albedo_check(samples, albedo_samples, W, H, iterations, sigma, flags))) return -1;
    if (workspace_bytes < rt_denoise_albedo_workspace_bytes(W, H)) return set_error("denoise: workspace too small: rt_denoise_albedo_workspace_bytes(W, H) = 152 bytes per pixel are needed");
    if (query_aligned(d_hits, "d_hits") || query_aligned(d_workspace, "d_workspace")) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_rgb_sum_out | (uintptr_t)d_albedo_sum) & 7u) != 0u) return set_error("d_rgb_sum, d_albedo_sum and d_rgb_sum_out must be 8-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    double* d_x = (double*)((unsigned char*)d_workspace + rt_denoise_workspace_bytes(W, H));
    return denoise_albedo_enqueue((const double*)d_rgb_sum, samples, (const double*)d_albedo_sum, albedo_samples, (const double*)d_hits, W, H, iterations,
                                  sigma, flags, (double*)d_rgb_sum_out, d_workspace, d_x, (hipStream_t)hip_stream);
}
int rt_denoise_albedo(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                      uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out) {
    if (!rgb_sum || !albedo_sum || !hits || !sigma || !rgb_sum_out) return set_error("null argument");
    if (refused(denoise_albedo_check(samples, albedo_samples, W, H, iterations, sigma, flags))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), ws_bytes = rt_denoise_albedo_workspace_bytes(W, H);
    DeviceBuffer d_sum, d_alb, d_hits, d_ws;
    if (upload(d_sum, rgb_sum, sum_bytes) || upload(d_alb, albedo_sum, sum_bytes) || upload(d_hits, hits, n * DENOISE_HIT_DOUBLES * sizeof(double))) return -1;
    HIP_OK(d_ws.alloc(ws_bytes));
    if (rt_denoise_albedo_device(d_sum.get(), samples, d_alb.get(), albedo_samples, d_hits.get(), W, H, iterations, sigma, flags, d_sum.get(), d_ws.get(), ws_bytes, nullptr)) return -1;
    HIP_OK(hipMemcpy(rgb_sum_out, d_sum.get(), sum_bytes, hipMemcpyDeviceToHost));       // (waits for the kernels: the null stream)
    return 0;
}
// The albedo sums of samples [0, albedo_samples) of the frame's view in d_alb_sum: built from the scene when the frame holds none or those
// of another albedo_samples (it holds none while the build is in flight), kept until then or rt_progressive_reset.
// With the chain on (rt_progressive_set_guide_chain) the sums are the chain albedos of samples [0, guide_samples), from the launch that builds
// the guide, and albedo_samples is SET to guide_samples: the caller's value only says that the frame is to be demodulated.
static int frame_albedo_ready(Progressive* p, uint32_t& albedo_samples) {
    if (p->chain_links) {
        albedo_samples = p->guide_samples;
        if (p->albedo_chain && p->albedo_samples == albedo_samples) return 0;
        if (frame_scene_current(p, SCENE_GONE_NO_ALBEDO)) return -1;
        const size_t hit_bytes = p->n_px() * DENOISE_HIT_DOUBLES * sizeof(double);
        DeviceBuffer d_hits;                        // (the records go: the packed guide the frame holds is that of the same launch arguments)
        HIP_OK(d_hits.alloc(hit_bytes));
        if (progressive_chain_records(p, d_hits.get(), hit_bytes)) return -1;
        HIP_OK(hipStreamSynchronize(nullptr));
        return 0;
    }
    const bool build = p->albedo_samples != albedo_samples || p->albedo_chain;
    if (build && frame_scene_current(p, SCENE_GONE_NO_ALBEDO)) return -1;
    HIP_OK(p->d_alb_sum.ensure(p->sum_bytes()));
    if (build) {
        p->albedo_samples = 0; p->albedo_chain = false;
        if (rt_query_camera_albedo_device(p->sc, &p->cam, p->W, p->H, 0u, albedo_samples, p->seed, 0u, p->d_alb_sum.get(), p->sum_bytes(), nullptr)) return -1;
        p->albedo_samples = albedo_samples; p->albedo_builds++;
    }
    return 0;
}
// The frame's sums demodulated by its own albedo frame, filtered, remodulated and resolved; everything the other resolves own stays as it is.
int rt_progressive_resolve_denoised_albedo_rgb8(void* frame, uint32_t albedo_samples, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !sigma || !rgb8_out) return set_error("null argument");
    if (albedo_samples == 0u) return set_error("denoise: albedo_samples must be >= 1 (the frame is demodulated by albedo_sum / albedo_samples)");
    if (adaptive_needs_uniform(p, "rt_progressive_resolve_denoised_albedo_rgb8")) return -1;
    DeviceGuard guard(p->device);
    if (progressive_denoise_prepare(p, iterations, sigma, flags) || frame_albedo_ready(p, albedo_samples)) return -1;
    HIP_OK(p->d_alb_x.ensure(p->sum_bytes()));
    if (denoise_albedo_enqueue(p->d_sum.as<double>(), p->done, p->d_alb_sum.as<double>(), albedo_samples, nullptr, p->W, p->H, iterations, sigma, flags,
                               p->d_dn_sum.as<double>(), p->d_dn_ws.get(), p->d_alb_x.as<double>(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), nullptr, p->done, rgb8_out);
}
int rt_debug_albedo_modulate_ms(const void* d_rgb_sum, const void* d_albedo_sum, uint64_t albedo_samples, void* d_x, uint64_t n_doubles, float ms_out[2]) {
    if (!d_rgb_sum || !d_albedo_sum || !d_x || !ms_out) return set_error("null argument");
    if (albedo_samples == 0u || n_doubles == 0u || n_doubles > 3ull * 0x7FFFFFFFull) return set_error("albedo_samples and n_doubles must be >= 1 (n_doubles <= 3 (2^31 - 1))");
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_albedo_sum | (uintptr_t)d_x) & 7u) != 0u) return set_error("the buffers must be 8-byte aligned");
    return timed_between_marks(3u, ms_out, [&](hipEvent_t* marks) {
        for (int pass = 0; pass < 2; pass++)                      // a warm run, then the one that is timed
            if (hipEventRecord(marks[0], nullptr) != hipSuccess || launch_albedo_demodulate((const double*)d_rgb_sum, (const double*)d_albedo_sum, albedo_samples, (double*)d_x, n_doubles, nullptr) != 0 ||
                hipEventRecord(marks[1], nullptr) != hipSuccess || launch_albedo_remodulate((double*)d_x, (const double*)d_albedo_sum, albedo_samples, n_doubles, nullptr) != 0 ||
                hipEventRecord(marks[2], nullptr) != hipSuccess) return set_error("rt_debug_albedo_modulate_ms: a launch failed");
        return 0;
    });
}
int rt_progressive_albedo_info(void* frame, uint32_t* albedo_samples_out, uint64_t* builds_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !albedo_samples_out || !builds_out) return set_error("null argument");
    *albedo_samples_out = p->albedo_samples; *builds_out = p->albedo_builds;
    return 0;
}

// ---------------------------------------------------------------- denoising a frame as it is (csrc/rt_denoise_frame.h: the specification; rt_denoise_frame.hip: the kernels)
int rt_adaptive_variance_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                                void* d_var_out, void* hip_stream) {
    if (!d_rgb_sum || !d_sq_sum || !d_counts || !d_passes || !d_var_out) return set_error("null argument");
    if (refused(adaptive_frame_check(W, H))) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_sq_sum | (uintptr_t)d_var_out) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_passes) & 3u) != 0u)
        return set_error("d_rgb_sum, d_sq_sum and d_var_out must be 8-byte aligned, d_counts and d_passes 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_frame_variance((const double*)d_rgb_sum, (const double*)d_sq_sum, (const uint32_t*)d_counts, (const uint32_t*)d_passes, W * H,
                                             (double*)d_var_out, hip_stream));
    return 0;
}
size_t rt_denoise_frame_workspace_bytes(uint32_t W, uint32_t H) { return denoise_frame_workspace_bytes((uint64_t)W * H); }

// The launches of one run on `stream`: prepare (c into d_c; Vd into d_vd when there are both a variance frame and albedo sums), the filter's
// own launches from d_c with samples = 1 to d_out, finish on d_out in place.  d_out may be d_sum: prepare has read it by the time anything
// is written there (stream order).  d_planes: d_c and, one padded plane behind it, d_vd.
static int denoise_frame_enqueue(const double* d_sum, const uint32_t* d_counts, uint64_t samples, const double* d_var, const double* d_albedo_sum,
                                 uint64_t albedo_samples, const double* d_hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                                 uint32_t flags, double* d_out, double* d_var_out, void* d_workspace, void* d_planes, hipStream_t stream) {
    const uint32_t n_px = W * H;
    double* d_c = (double*)d_planes;
    double* d_vd = (double*)((unsigned char*)d_planes + denoise_frame_plane_bytes(n_px));
    HIP_OK((hipError_t)launch_frame_prepare(d_sum, d_counts, samples, d_var, d_albedo_sum, albedo_samples, d_c, d_vd, n_px, stream));
    if (d_var) {
        if (denoise_variance_enqueue(d_c, 1u, d_albedo_sum ? d_vd : d_var, d_hits, W, H, iterations, sigma, flags, d_out, d_var_out, d_workspace, stream)) return -1;
    } else if (denoise_enqueue(d_c, 1u, d_hits, W, H, iterations, sigma, flags, d_out, d_workspace, stream)) return -1;
    HIP_OK((hipError_t)launch_frame_finish(d_out, d_counts, samples, d_albedo_sum, albedo_samples, n_px, stream));
    return 0;
}
int rt_denoise_frame_device(const void* d_rgb_sum, const void* d_counts, uint64_t samples, const void* d_var, const void* d_albedo_sum,
                            uint64_t albedo_samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                            uint32_t flags, void* d_rgb_sum_out, void* d_var_out, void* d_workspace, size_t workspace_bytes, void* hip_stream) {
    if (!d_rgb_sum || !d_hits || !sigma || !d_rgb_sum_out || !d_workspace) return set_error("null argument");
    if (refused(denoise_frame_check(d_counts != nullptr, samples, d_var != nullptr, d_albedo_sum != nullptr, albedo_samples, W, H, iterations, sigma,
                                    flags, d_var_out != nullptr))) return -1;
    if (workspace_bytes < rt_denoise_frame_workspace_bytes(W, H))
        return set_error("denoise: workspace too small: rt_denoise_frame_workspace_bytes(W, H) — the filter's 128 bytes per pixel and two frames of 24 — are needed");
    if (query_aligned(d_hits, "d_hits") || query_aligned(d_workspace, "d_workspace")) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_rgb_sum_out | (uintptr_t)d_var | (uintptr_t)d_var_out | (uintptr_t)d_albedo_sum) & 7u) != 0u || ((uintptr_t)d_counts & 3u) != 0u)
        return set_error("d_rgb_sum, d_var, d_albedo_sum, d_rgb_sum_out and d_var_out must be 8-byte aligned, d_counts 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    return denoise_frame_enqueue((const double*)d_rgb_sum, (const uint32_t*)d_counts, samples, (const double*)d_var, (const double*)d_albedo_sum, albedo_samples,
                                 (const double*)d_hits, W, H, iterations, sigma, flags, (double*)d_rgb_sum_out, (double*)d_var_out, d_workspace,
                                 (unsigned char*)d_workspace + rt_denoise_workspace_bytes(W, H), (hipStream_t)hip_stream);
}
int rt_denoise_frame(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum,
                     uint64_t albedo_samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                     uint32_t flags, double* rgb_sum_out, double* var_out) {
    if (!rgb_sum || !hits || !sigma || !rgb_sum_out) return set_error("null argument");
    if (refused(denoise_frame_check(counts != nullptr, samples, var != nullptr, albedo_sum != nullptr, albedo_samples, W, H, iterations, sigma,
                                    flags, var_out != nullptr))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), ws_bytes = rt_denoise_frame_workspace_bytes(W, H);
    DeviceBuffer d_sum, d_cnt, d_var, d_alb, d_hits, d_ws, d_vout;
    if (upload(d_sum, rgb_sum, sum_bytes) || upload(d_hits, hits, n * DENOISE_HIT_DOUBLES * sizeof(double)) || upload(d_cnt, counts, n * sizeof(uint32_t)) ||
        upload(d_var, var, sum_bytes) || upload(d_alb, albedo_sum, sum_bytes)) return -1;
    HIP_OK(d_ws.alloc(ws_bytes));
    if (var_out) HIP_OK(d_vout.alloc(n * sizeof(double)));
    if (rt_denoise_frame_device(d_sum.get(), d_cnt.get(), samples, d_var.get(), d_alb.get(), albedo_samples, d_hits.get(), W, H, iterations, sigma, flags, d_sum.get(),
                                d_vout.get(), d_ws.get(), ws_bytes, nullptr)) return -1;
    HIP_OK(hipMemcpy(rgb_sum_out, d_sum.get(), sum_bytes, hipMemcpyDeviceToHost));       // (waits for the kernels: the null stream)
    if (var_out) HIP_OK(hipMemcpy(var_out, d_vout.get(), n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
// what the variance of a frame with counts needs: moments that describe the sums (two passes are every pixel's own matter, (E))
static int frame_variance_ready(Progressive* p) {
    if (!p->adaptive) return moments_error_ready(p);
    if (!p->moments_valid) return set_error("the moments of this frame are invalid: rt_progressive_load_sum loaded sums whose second moments are unknown (rt_progressive_reset or rt_progressive_load_moments)");
    return 0;
}
// (E) on an adaptive frame, (4) on any other: into the frame's own variance frame, on `stream`
static int frame_variance_enqueue(Progressive* p, hipStream_t stream) {
    if (!p->adaptive) return progressive_variance_enqueue(p, stream);
    HIP_OK(p->d_var.ensure(p->sum_bytes()));
    HIP_OK((hipError_t)launch_frame_variance(p->d_sum.as<double>(), p->d_sq.as<double>(), p->d_cnt.as<uint32_t>(), p->d_pas.as<uint32_t>(), (uint32_t)p->n_px(),
                                             p->d_var.as<double>(), stream));
    return 0;
}
int rt_progressive_variance_counts(void* frame, double* var_out) {
    Progressive* p = (Progressive*)frame;
    if (!var_out) return set_error("null argument");
    if (moments_frame(p) || frame_variance_ready(p)) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());                 // passes enqueued on the caller's streams belong to the estimate
    if (frame_variance_enqueue(p, nullptr)) return -1;
    HIP_OK(hipMemcpy(var_out, p->d_var.get(), p->sum_bytes(), hipMemcpyDeviceToHost));      // (waits for the kernel: the null stream)
    return 0;
}
// The frame as it is — its counts when it has them, its variance under the variance stop, its albedo sums when asked for — filtered and
// resolved; everything the other resolves own stays as it is.
int rt_progressive_resolve_denoised_frame_rgb8(void* frame, uint32_t stop, uint32_t albedo_samples, uint32_t iterations, const double sigma[3],
                                               uint32_t flags, uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !sigma || !rgb8_out) return set_error("null argument");
    if (stop > (uint32_t)RT_DENOISE_STOP_VARIANCE) return set_error("denoise: stop must be RT_DENOISE_STOP_COLOUR = 0 or RT_DENOISE_STOP_VARIANCE = 1");
    const bool variance = stop == (uint32_t)RT_DENOISE_STOP_VARIANCE;
    if (variance && (moments_frame(p) || frame_variance_ready(p) || refused(denoise_variance_check(p->done ? p->done : 1u, p->W, p->H, iterations, sigma, flags)))) return -1;
    DeviceGuard guard(p->device);
    if (progressive_denoise_prepare(p, iterations, sigma, flags)) return -1;
    // (the albedo sums rt_progressive_resolve_denoised_albedo_rgb8 keeps, built as it builds them)
    if (albedo_samples && frame_albedo_ready(p, albedo_samples)) return -1;
    HIP_OK(p->d_fr_planes.ensure(2u * denoise_frame_plane_bytes(p->n_px())));
    if (variance && frame_variance_enqueue(p, nullptr)) return -1;
    if (denoise_frame_enqueue(p->d_sum.as<double>(), p->counts(), p->done, variance ? p->d_var.as<double>() : nullptr,
                              albedo_samples ? p->d_alb_sum.as<double>() : nullptr, albedo_samples, nullptr, p->W, p->H, iterations, sigma, flags,
                              p->d_dn_sum.as<double>(), nullptr, p->d_dn_ws.get(), p->d_fr_planes.get(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), p->counts(), p->done, rgb8_out);
}

// ---------------------------------------------------------------- temporal accumulation (csrc/rt_reproject.h: the specification; rt_reproject.hip: the kernels)
int rt_reproject_device(const void* d_prev_sum, const void* d_prev_counts, uint64_t prev_samples, const void* d_prev_hits, const rt_camera* prev_cam,
                        const void* d_cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                        void* d_hist_sum_out, void* d_hist_counts_out, void* hip_stream) {
    if (!d_prev_sum || !d_prev_hits || !prev_cam || !d_cur_hits || !sigma || !d_hist_sum_out || !d_hist_counts_out) return set_error("null argument");
    if (refused(reproject_check(d_prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags))) return -1;
    if (query_aligned(d_prev_hits, "d_prev_hits") || query_aligned(d_cur_hits, "d_cur_hits")) return -1;
    if ((((uintptr_t)d_prev_sum | (uintptr_t)d_hist_sum_out) & 7u) != 0u || (((uintptr_t)d_prev_counts | (uintptr_t)d_hist_counts_out) & 3u) != 0u)
        return set_error("d_prev_sum and d_hist_sum_out must be 8-byte aligned, d_prev_counts and d_hist_counts_out 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    double fields[21];
    rt_camera_fields(prev_cam, fields);
    HIP_OK((hipError_t)launch_reproject(reproject_consts(fields, prev_samples, W, H, max_history, sigma), (const double*)d_prev_sum, (const uint32_t*)d_prev_counts,
                                        (const double*)d_prev_hits, (const double*)d_cur_hits, (double*)d_hist_sum_out, (uint32_t*)d_hist_counts_out, hip_stream));
    return 0;
}
int rt_reproject(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_hits, const rt_camera* prev_cam,
                 const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                 double* hist_sum_out, uint32_t* hist_counts_out) {
    if (!prev_sum || !prev_hits || !prev_cam || !cur_hits || !sigma || !hist_sum_out || !hist_counts_out) return set_error("null argument");
    if (refused(reproject_check(prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), cnt_bytes = n * sizeof(uint32_t), hit_bytes = n * REPROJECT_HIT_DOUBLES * sizeof(double);
    DeviceBuffer d_sum, d_cnt, d_prev, d_cur, d_hsum, d_hcnt;
    if (upload(d_sum, prev_sum, sum_bytes) || upload(d_cnt, prev_counts, cnt_bytes) || upload(d_prev, prev_hits, hit_bytes) || upload(d_cur, cur_hits, hit_bytes)) return -1;
    HIP_OK(d_hsum.alloc(sum_bytes)); HIP_OK(d_hcnt.alloc(cnt_bytes));
    if (rt_reproject_device(d_sum.get(), d_cnt.get(), prev_samples, d_prev.get(), prev_cam, d_cur.get(), W, H, max_history, sigma, flags, d_hsum.get(), d_hcnt.get(), nullptr)) return -1;
    HIP_OK(hipMemcpy(hist_sum_out, d_hsum.get(), sum_bytes, hipMemcpyDeviceToHost));     // (waits for the kernel: the null stream)
    HIP_OK(hipMemcpy(hist_counts_out, d_hcnt.get(), cnt_bytes, hipMemcpyDeviceToHost));
    return 0;
}
int rt_temporal_blend_device(const void* d_rgb_sum, const void* d_counts, uint64_t samples, const void* d_hist_sum, const void* d_hist_counts,
                             uint32_t W, uint32_t H, void* d_sum_out, void* d_counts_out, void* hip_stream) {
    if (!d_rgb_sum || !d_hist_sum || !d_hist_counts || !d_sum_out || !d_counts_out) return set_error("null argument");
    if (refused(reproject_frame_check(W, H))) return -1;
    if ((((uintptr_t)d_rgb_sum | (uintptr_t)d_hist_sum | (uintptr_t)d_sum_out) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_hist_counts | (uintptr_t)d_counts_out) & 3u) != 0u)
        return set_error("d_rgb_sum, d_hist_sum and d_sum_out must be 8-byte aligned, d_counts, d_hist_counts and d_counts_out 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_temporal_blend((const double*)d_rgb_sum, (const uint32_t*)d_counts, samples, (const double*)d_hist_sum, (const uint32_t*)d_hist_counts,
                                             W * H, (double*)d_sum_out, (uint32_t*)d_counts_out, hip_stream));
    return 0;
}
// ---- temporal variance (csrc/rt_reproject_var.h: the specification; rt_reproject_var.hip: the kernels)
int rt_reproject_variance_device(const void* d_prev_sum, const void* d_prev_counts, uint64_t prev_samples, const void* d_prev_var, const void* d_prev_hits,
                                 const rt_camera* prev_cam, const void* d_cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                                 uint32_t flags, void* d_hist_sum_out, void* d_hist_counts_out, void* d_hist_var_out, void* hip_stream) {
    if (!d_prev_sum || !d_prev_var || !d_prev_hits || !prev_cam || !d_cur_hits || !sigma || !d_hist_sum_out || !d_hist_counts_out || !d_hist_var_out)
        return set_error("null argument");
    if (refused(reproject_check(d_prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags))) return -1;
    if (query_aligned(d_prev_hits, "d_prev_hits") || query_aligned(d_cur_hits, "d_cur_hits")) return -1;
    if ((((uintptr_t)d_prev_sum | (uintptr_t)d_prev_var | (uintptr_t)d_hist_sum_out | (uintptr_t)d_hist_var_out) & 7u) != 0u ||
        (((uintptr_t)d_prev_counts | (uintptr_t)d_hist_counts_out) & 3u) != 0u)
        return set_error("d_prev_sum, d_prev_var, d_hist_sum_out and d_hist_var_out must be 8-byte aligned, d_prev_counts and d_hist_counts_out 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    double fields[21];
    rt_camera_fields(prev_cam, fields);
    HIP_OK((hipError_t)launch_reproject_variance(reproject_consts(fields, prev_samples, W, H, max_history, sigma), (const double*)d_prev_sum, (const uint32_t*)d_prev_counts,
                                                 (const double*)d_prev_var, (const double*)d_prev_hits, (const double*)d_cur_hits, (double*)d_hist_sum_out,
                                                 (uint32_t*)d_hist_counts_out, (double*)d_hist_var_out, hip_stream));
    return 0;
}
int rt_reproject_variance(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_var, const double* prev_hits,
                          const rt_camera* prev_cam, const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                          uint32_t flags, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out) {
    if (!prev_sum || !prev_var || !prev_hits || !prev_cam || !cur_hits || !sigma || !hist_sum_out || !hist_counts_out || !hist_var_out) return set_error("null argument");
    if (refused(reproject_check(prev_counts != nullptr, prev_samples, W, H, max_history, sigma, flags))) return -1;
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    const size_t n = (size_t)W * H, sum_bytes = n * 3 * sizeof(double), cnt_bytes = n * sizeof(uint32_t), hit_bytes = n * REPROJECT_HIT_DOUBLES * sizeof(double);
    DeviceBuffer d_sum, d_cnt, d_var, d_prev, d_cur, d_hsum, d_hcnt, d_hvar;
    if (upload(d_sum, prev_sum, sum_bytes) || upload(d_cnt, prev_counts, cnt_bytes) || upload(d_var, prev_var, sum_bytes) || upload(d_prev, prev_hits, hit_bytes) ||
        upload(d_cur, cur_hits, hit_bytes)) return -1;
    HIP_OK(d_hsum.alloc(sum_bytes)); HIP_OK(d_hcnt.alloc(cnt_bytes)); HIP_OK(d_hvar.alloc(sum_bytes));
    if (rt_reproject_variance_device(d_sum.get(), d_cnt.get(), prev_samples, d_var.get(), d_prev.get(), prev_cam, d_cur.get(), W, H, max_history, sigma, flags, d_hsum.get(),
                                     d_hcnt.get(), d_hvar.get(), nullptr)) return -1;
    HIP_OK(hipMemcpy(hist_sum_out, d_hsum.get(), sum_bytes, hipMemcpyDeviceToHost));     // (waits for the kernel: the null stream)
    HIP_OK(hipMemcpy(hist_counts_out, d_hcnt.get(), cnt_bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hist_var_out, d_hvar.get(), sum_bytes, hipMemcpyDeviceToHost));
    return 0;
}
int rt_temporal_blend_variance_device(const void* d_var, const void* d_counts, uint64_t samples, const void* d_hist_var, const void* d_hist_counts,
                                      uint64_t n_px, void* d_var_out, void* hip_stream) {
    if (!d_hist_var || !d_hist_counts || !d_var_out) return set_error("null argument");
    if (refused(blend_variance_check(n_px))) return -1;
    if ((((uintptr_t)d_var | (uintptr_t)d_hist_var | (uintptr_t)d_var_out) & 7u) != 0u || (((uintptr_t)d_counts | (uintptr_t)d_hist_counts) & 3u) != 0u)
        return set_error("d_var, d_hist_var and d_var_out must be 8-byte aligned, d_counts and d_hist_counts 4-byte aligned");
    if (rt_device_count() <= 0) return set_error("no HIP device: librt_amd has no CPU rendering path");
    HIP_OK((hipError_t)launch_temporal_blend_variance((const double*)d_var, (const uint32_t*)d_counts, samples, (const double*)d_hist_var, (const uint32_t*)d_hist_counts,
                                                      (uint32_t)n_px, (double*)d_var_out, hip_stream));
    return 0;
}
// The history's buffers, allocated at first use; without a history they are made the empty one (all +0.0 and 0), so that every caller blends
// with something.  On the null stream; nothing waits.
static int progressive_history_ready(Progressive* p) {
    const size_t n = p->n_px();
    HIP_OK(p->d_hist_sum.ensure(p->sum_bytes())); HIP_OK(p->d_hist_cnt.ensure(n * sizeof(uint32_t)));
    if (!p->hist_valid) {
        HIP_OK(hipMemsetAsync(p->d_hist_sum.get(), 0, p->sum_bytes(), nullptr));
        HIP_OK(hipMemsetAsync(p->d_hist_cnt.get(), 0, n * sizeof(uint32_t), nullptr));
        p->hist_valid = true; p->hist_px = 0;
    }
    return 0;
}
// ... and, on a frame with moments, the history's variance beside them (rt_reproject_var.h).  A history taken before the moments were
// enabled has none: unknown (+inf) where H_cnt > 0 and +0.0 elsewhere, as (V) writes a pixel none of whose taps knows its variance.
static int progressive_history_variance_ready(Progressive* p) {
    if (progressive_history_ready(p)) return -1;
    HIP_OK(p->d_hist_var.ensure(p->sum_bytes()));
    if (p->hist_var_valid) return 0;
    if (p->hist_px == 0) HIP_OK(hipMemsetAsync(p->d_hist_var.get(), 0, p->sum_bytes(), nullptr));
    else {
        const size_t n = p->n_px();
        std::vector<uint32_t> cnt(n);
        HIP_OK(hipMemcpy(cnt.data(), p->d_hist_cnt.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));      // (waits: the null stream)
        std::vector<double> var(n * 3u, 0.0);
        for (size_t k = 0; k < n; k++) if (cnt[k] != 0u) var[3u * k] = var[3u * k + 1u] = var[3u * k + 2u] = variance_unknown();
        HIP_OK(hipMemcpy(p->d_hist_var.get(), var.data(), p->sum_bytes(), hipMemcpyHostToDevice));
    }
    p->hist_var_valid = true;
    return 0;
}
// the frame's own variance for (BV): rt_moments.h (4) into d_var when the moments describe the sums and hold two passes, else none (null)
static int frame_variance_or_null(Progressive* p, const double*& d_var_out) {
    d_var_out = nullptr;
    if (!p->moments_valid || p->passes < 2u || p->done < 2u) return 0;
    if (progressive_variance_enqueue(p, nullptr)) return -1;
    d_var_out = p->d_var.as<double>();
    return 0;
}
// the variance of the frame blended with its history (rt_reproject_var.h (BV)) into a buffer of one call, on the null stream
static int frame_blend_variance_with_history(Progressive* p, DeviceBuffer& d_bvar) {
    const double* d_var = nullptr;
    if (frame_variance_or_null(p, d_var)) return -1;
    HIP_OK(d_bvar.alloc(p->sum_bytes()));
    HIP_OK((hipError_t)launch_temporal_blend_variance(d_var, nullptr, p->done, p->d_hist_var.as<double>(), p->d_hist_cnt.as<uint32_t>(), (uint32_t)p->n_px(),
                                                      d_bvar.as<double>(), nullptr));
    return 0;
}
// the frame's sums blended with its history (rt_reproject.h (B)) into two buffers of one call, on the null stream
static int frame_blend_with_history(Progressive* p, DeviceBuffer& d_bsum, DeviceBuffer& d_bcnt) {
    const size_t n = p->n_px();
    HIP_OK(d_bsum.alloc(p->sum_bytes())); HIP_OK(d_bcnt.alloc(n * sizeof(uint32_t)));
    HIP_OK((hipError_t)launch_temporal_blend(p->d_sum.as<double>(), nullptr, p->done, p->d_hist_sum.as<double>(), p->d_hist_cnt.as<uint32_t>(), (uint32_t)n,
                                             d_bsum.as<double>(), d_bcnt.as<uint32_t>(), nullptr));
    return 0;
}
int rt_progressive_set_view(void* frame, const rt_camera* cam, uint64_t seed, uint32_t max_history, const double sigma[2]) {
    Progressive* p = (Progressive*)frame;
    if (!p || !cam || !sigma) return set_error("null argument");
    if (p->adaptive) return set_error("rt_progressive_set_view: not available on an adaptive frame (rt_reproject_device and rt_temporal_blend_device take per-pixel counts: a caller can compose them)");
    if (frame_scene_current(p)) return -1;
    if (refused(reproject_check(true, 0u, p->W, p->H, max_history, sigma, 0u))) return -1;
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());                 // passes enqueued on the caller's streams belong to the previous frame
    if (p->moments ? progressive_history_variance_ready(p) : progressive_history_ready(p)) return -1;
    const size_t n = p->n_px(), cnt_bytes = n * sizeof(uint32_t), hit_bytes = n * REPROJECT_HIT_DOUBLES * sizeof(double);
    if (max_history == 0u || (p->done == 0 && p->hist_px == 0)) {     // nothing is carried over: the empty history, as (R5) gives it
        HIP_OK(hipMemsetAsync(p->d_hist_sum.get(), 0, p->sum_bytes(), nullptr));
        HIP_OK(hipMemsetAsync(p->d_hist_cnt.get(), 0, cnt_bytes, nullptr));
        if (p->moments) HIP_OK(hipMemsetAsync(p->d_hist_var.get(), 0, p->sum_bytes(), nullptr));
        p->hist_px = 0;
    } else {
        // (the blends go to buffers of this call: the kernel reads the old history through them while it writes the new one)
        DeviceBuffer d_bsum, d_bcnt, d_bvar, d_prev, d_cur;
        if (frame_blend_with_history(p, d_bsum, d_bcnt)) return -1;
        if (p->moments && frame_blend_variance_with_history(p, d_bvar)) return -1;
        HIP_OK(d_prev.alloc(hit_bytes)); HIP_OK(d_cur.alloc(hit_bytes));
        if (progressive_view_records(p, &p->cam, p->seed, d_prev.get(), hit_bytes)) return -1;
        if (progressive_view_records(p, cam, seed, d_cur.get(), hit_bytes)) return -1;
        // a frame with moments: sums, counts and variances in one launch (rt_reproject_var.h (V)); any other frame: rt_reproject as before
        if (p->moments ? rt_reproject_variance_device(d_bsum.get(), d_bcnt.get(), 0u, d_bvar.get(), d_prev.get(), &p->cam, d_cur.get(), p->W, p->H, max_history, sigma, 0u,
                                                      p->d_hist_sum.get(), p->d_hist_cnt.get(), p->d_hist_var.get(), nullptr)
                       : rt_reproject_device(d_bsum.get(), d_bcnt.get(), 0u, d_prev.get(), &p->cam, d_cur.get(), p->W, p->H, max_history, sigma, 0u, p->d_hist_sum.get(), p->d_hist_cnt.get(), nullptr)) return -1;
        std::vector<uint32_t> cnt(n);
        HIP_OK(hipMemcpy(cnt.data(), p->d_hist_cnt.get(), cnt_bytes, hipMemcpyDeviceToHost));      // (waits for the kernels: the null stream)
        uint64_t px = 0;
        for (size_t k = 0; k < n; k++) px += cnt[k] != 0u;
        p->hist_px = px;
    }
    std::memcpy(&p->cam, cam, sizeof(rt_camera)); p->seed = seed;
    p->guide_valid = false; p->albedo_samples = 0;      // as rt_progressive_reset: a new frame of the new view ...
    p->views++;
    return progressive_restart(p, nullptr, 0);          // ... that keeps its history
}
int rt_progressive_read_history(void* frame, double* hist_sum_out, uint32_t* hist_counts_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !hist_sum_out || !hist_counts_out) return set_error("null argument");
    const size_t n = p->n_px();
    if (!p->hist_valid) {
        std::memset(hist_sum_out, 0, p->sum_bytes()); std::memset(hist_counts_out, 0, n * sizeof(uint32_t));
        return 0;
    }
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(hist_sum_out, p->d_hist_sum.get(), p->sum_bytes(), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hist_counts_out, p->d_hist_cnt.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}
int rt_progressive_read_history_variance(void* frame, double* hist_var_out) {
    Progressive* p = (Progressive*)frame;
    if (!hist_var_out) return set_error("null argument");
    if (moments_frame(p)) return -1;
    if (!p->hist_valid) {
        std::memset(hist_var_out, 0, p->sum_bytes());
        return 0;
    }
    DeviceGuard guard(p->device);
    HIP_OK(hipDeviceSynchronize());
    if (progressive_history_variance_ready(p)) return -1;
    HIP_OK(hipMemcpy(hist_var_out, p->d_hist_var.get(), p->sum_bytes(), hipMemcpyDeviceToHost));      // (waits: the null stream)
    return 0;
}
int rt_progressive_history_info(void* frame, uint64_t out[2]) {
    Progressive* p = (Progressive*)frame;
    if (!p || !out) return set_error("null argument");
    out[0] = p->views; out[1] = p->hist_valid ? p->hist_px : 0u;
    return 0;
}
// The blend of the frame with its history resolved with the blend's counts, with the frame filter in between when iterations >= 1; into
// the denoised resolves' buffers: d_sum, the history, the plain resolve's two images and its count stay as they are.
int rt_progressive_resolve_temporal_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!p || !rgb8_out || (iterations && !sigma)) return set_error("null argument");
    if (p->adaptive) return set_error("rt_progressive_resolve_temporal_rgb8: not available on an adaptive frame (it has no history: rt_progressive_set_view refuses it)");
    if (iterations > DENOISE_MAX_ITERATIONS) return set_error("denoise: iterations must be 0 .. 8 (0: the resolve of the blend without a filter)");
    const bool history = p->hist_valid && p->hist_px > 0;
    if (p->done == 0 && !history) return set_error("nothing to resolve: the frame holds 0 samples and no history (rt_progressive_add, rt_progressive_set_view)");
    DeviceGuard guard(p->device);
    if (iterations) { if (progressive_denoise_prepare(p, iterations, sigma, flags, true)) return -1; }
    else {
        HIP_OK(hipDeviceSynchronize());             // passes enqueued on the caller's streams belong to the image
        if (frame_image_ready(p)) return -1;
    }
    if (progressive_history_ready(p)) return -1;
    DeviceBuffer d_bsum, d_bcnt;                    // (they go when this call returns: frame_resolve_out has waited for the kernels by then)
    if (frame_blend_with_history(p, d_bsum, d_bcnt)) return -1;
    if (!iterations) return frame_resolve_out(p, d_bsum.as<double>(), d_bcnt.as<uint32_t>(), 0u, rgb8_out);
    HIP_OK(p->d_fr_planes.ensure(2u * denoise_frame_plane_bytes(p->n_px())));
    if (denoise_frame_enqueue(d_bsum.as<double>(), d_bcnt.as<uint32_t>(), 0u, nullptr, nullptr, 0u, nullptr, p->W, p->H, iterations, sigma, flags,
                              p->d_dn_sum.as<double>(), nullptr, p->d_dn_ws.get(), p->d_fr_planes.get(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), d_bcnt.as<uint32_t>(), 0u, rgb8_out);
}

// ... with the variance stop: the blend's variance (rt_reproject_var.h (BV)) beside the blend's sums and counts, albedo sums when asked for
int rt_progressive_resolve_temporal_variance_rgb8(void* frame, uint32_t albedo_samples, uint32_t iterations, const double sigma[3], uint32_t flags,
                                                  uint8_t* rgb8_out) {
    Progressive* p = (Progressive*)frame;
    if (!sigma || !rgb8_out) return set_error("null argument");
    if (moments_frame(p)) return -1;
    if (p->adaptive) return set_error("rt_progressive_resolve_temporal_variance_rgb8: not available on an adaptive frame (it has no history: rt_progressive_set_view refuses it)");
    if (refused(denoise_variance_check(p->done ? p->done : 1u, p->W, p->H, iterations, sigma, flags))) return -1;
    const bool history = p->hist_valid && p->hist_px > 0;
    if (p->done == 0 && !history) return set_error("nothing to resolve: the frame holds 0 samples and no history (rt_progressive_add, rt_progressive_set_view)");
    DeviceGuard guard(p->device);
    if (progressive_denoise_prepare(p, iterations, sigma, flags, true)) return -1;
    if (albedo_samples && frame_albedo_ready(p, albedo_samples)) return -1;
    if (progressive_history_variance_ready(p)) return -1;
    DeviceBuffer d_bsum, d_bcnt, d_bvar;            // (they go when this call returns: frame_resolve_out has waited for the kernels by then)
    if (frame_blend_with_history(p, d_bsum, d_bcnt) || frame_blend_variance_with_history(p, d_bvar)) return -1;
    HIP_OK(p->d_fr_planes.ensure(2u * denoise_frame_plane_bytes(p->n_px())));
    if (denoise_frame_enqueue(d_bsum.as<double>(), d_bcnt.as<uint32_t>(), 0u, d_bvar.as<double>(), albedo_samples ? p->d_alb_sum.as<double>() : nullptr, albedo_samples,
                              nullptr, p->W, p->H, iterations, sigma, flags, p->d_dn_sum.as<double>(), nullptr, p->d_dn_ws.get(), p->d_fr_planes.get(), nullptr)) return -1;
    return frame_resolve_out(p, p->d_dn_sum.as<double>(), d_bcnt.as<uint32_t>(), 0u, rgb8_out);
}

} // extern "C"
