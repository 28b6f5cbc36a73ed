/* include/rt_amd.h — C-ABI of the MI355X-native path tracer (librt_amd.so).
 *
 * Drop-in boundary for the per-pixel sample loop of 4meame/RayTracingInRust.  The reference has
 * no FFI/plugin interface of its own (one binary, `fn main`, src/main.rs:577); the seam is the
 * per-pixel closure src/main.rs:811-830 + `format_color` src/main.rs:832.  A Rust `main.rs`
 * keeps its scene functions and camera set-up, mirrors them through the builder entry points
 * below (one entry point per reference constructor, cited next to each), and replaces the
 * `for j / for i / into_par_iter().map().sum()` loop nest with ONE call to rt_render(); see
 * INTEGRATION.md for the `extern "C"` block.
 *
 * Conventions: plain C, no torch / HIP types.  Handles are small non-negative ints scoped to one
 * rt_scene; every function that can fail returns a negative value (builders) or non-zero status
 * (render) and leaves a message for rt_last_error().  The reference's failure mode is panic
 * (src/bvh.rs:28,55,61; src/hit.rs:95; src/main.rs:431) — an error code here.  All reals are f64,
 * as in the reference (src/vec.rs:10-12).
 */
#ifndef RT_AMD_H
#define RT_AMD_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_scene rt_scene;
typedef struct rt_rng rt_rng;

/* enum Plane, src/rect.rs:9-13;  enum Axis, src/rotate.rs:8-12 */
enum { RT_PLANE_XY = 0, RT_PLANE_XZ = 1, RT_PLANE_YZ = 2 };
enum { RT_AXIS_X = 0, RT_AXIS_Y = 1, RT_AXIS_Z = 2 };

/* Camera::new arguments, src/camera.rs:19 */
typedef struct rt_camera {
    double lookfrom[3], lookat[3], vup[3];
    double vfov, aspect, aperture, focus_dist, time0, time1;
} rt_camera;

/* render flags */
enum {
    RT_F64 = 0,            /* reference precision (default): every operation in f64                         */
    RT_F32 = 1,            /* throughput variant: f32 arithmetic (statistical parity only)                   */
    RT_STOP_ON_ZERO = 2,   /* opt-in: end a path whose throughput is exactly (0,0,0); differs from the
                              reference only where a later bounce would have produced NaN (0*NaN)            */
    RT_NEAR_FIRST_BVH = 8, /* opt-in order (fewer node visits; faster only on some scenes): BVH children are visited nearer-first (by the ray's sign on the split axis) instead
                              of the reference's always-left-first (src/bvh.rs:81-84).  Same closest hit; exact-t ties are
                              still resolved by the reference's DFS order.  Can differ only where a last-ulp box cull depends
                              on the order hits are found.                                                                   */
    RT_PERSISTENT_BVH = 16, /* scheduling only, same samples: lanes keep their place inside a BVH while the rest of the wavefront
                              shades / regenerates (mesh kernels).  Chosen automatically for triangle-mesh BVHs that stand
                              beside other top-level objects: by tree size, or by a calibration of the view (rt_scene_calibrate;
                              rt_render / rt_render_multi run one at a scene's first frame of >= 1e8 samples); this flag forces it on ... */
    RT_LOCKSTEP_BVH = 32,  /* ... and this one forces the lock-step loop                                                      */
    RT_MULTI_COLLECTIVE = 64, /* rt_render_multi only: run the RCCL gather even when one device is selected (a one-GPU box then
                              exercises the same collective calls as an 8-GPU node)                                          */
    RT_SPECULATE_BVH = 1024, /* scheduling only, same samples (lock-step BVH kernel): a lane that has reached a leaf walks on while it waits for the
                              leaf step (rt_kernel.hip: bvh_hit_filt, SPEC).  Chosen automatically for scenes whose world is one BVH (every ray
                              enters it); this flag forces it on ...                                                          */
    RT_NO_SPECULATE_BVH = 2048, /* ... and this one off                                                                        */
    RT_ISOTROPIC_SCATTER = 4 /* opt-in, NOT the committed reference behaviour: Isotropic (constant media) scatters with its
                              old `scatter` (src/mat.rs:417-421) instead of absorbing — the look of img/volume.png       */
};

const char* rt_last_error(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int rt_device_count(void);

/* ---- seeded stream replacing rand::thread_rng() for HOST-side scene construction
 *      (src/main.rs:154,457; src/perlin.rs:5,22).  Spec: raytracinginrust_amd/csrc/rt_rng.h          */
rt_rng* rt_rng_create(uint64_t seed, uint32_t stream);
void rt_rng_destroy(rt_rng*);
double rt_rng_f64(rt_rng*);                       /* rng.gen::<f64>()                 */
double rt_rng_range(rt_rng*, double a, double b); /* rng.gen_range(a..b)              */
int rt_rng_bool(rt_rng*);                         /* rng.gen::<bool>()                */
uint32_t rt_rng_index(rt_rng*, uint32_t n);       /* rng.gen_range(0..n)              */
uint32_t rt_rng_u32(rt_rng*);
void rt_rng_path(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t state_out[4]);

/* ---- scene ------------------------------------------------------------------------------- */
rt_scene* rt_scene_create(void);
void rt_scene_destroy(rt_scene*);
const char* rt_scene_error(rt_scene*);

/* textures, src/texture.rs:16,37,63,90 */
int rt_texture_constant(rt_scene*, const double rgb[3]);              /* ConstantTexture::new  */
int rt_texture_check(rt_scene*, int odd, int even);                   /* CheckTexture::new     */
int rt_texture_noise(rt_scene*, double scale, rt_rng* rng);           /* NoiseTexture::new (Perlin::new draws from rng, src/perlin.rs:67-75) */
int rt_texture_image(rt_scene*, const uint8_t* rgb8, uint32_t width, uint32_t height);   /* ImageTexture::new */

/* materials, src/mat.rs:101,205,260,303,383,410 */
int rt_material_lambertian(rt_scene*, int texture);
int rt_material_metal(rt_scene*, const double albedo[3], double fuzz);
int rt_material_dielectric(rt_scene*, double index_of_refraction);
int rt_material_diffuse_light(rt_scene*, int texture);
int rt_material_isotropic(rt_scene*, int texture);
/* PBR::new (the principled "Disney" material), src/mat.rs:101: params = metallic, subsurface, specular, roughness,
 * specular_tint, anisotropic, sheen, sheen_tint, clearcoat, clearcoat_gloss (the constructor's argument order) */
int rt_material_pbr(rt_scene*, int base_color_texture, const double params[10]);

/* hittables */
int rt_sphere(rt_scene*, const double center[3], double radius, int material);                         /* Sphere::new, src/sphere.rs:46        */
int rt_moving_sphere(rt_scene*, const double c0[3], const double c1[3], double t0, double t1,
                     double radius, int material);                                                     /* MovingSphere::new, src/sphere.rs:133 */
int rt_aarect(rt_scene*, int plane, double a0, double a1, double b0, double b1, double k, int material); /* AARect::new, src/rect.rs:35         */
int rt_cube(rt_scene*, const double min[3], const double max[3], int material);                        /* Cube::new, src/cube.rs:14            */
int rt_triangle(rt_scene*, const double v[9], int material);                                           /* Triangle::new, src/tri.rs:15         */
int rt_list_create(rt_scene*);                                                                         /* HittableList::default, src/hit.rs:46 */
int rt_list_push(rt_scene*, int list, int hittable);                                                   /* HittableList::push, src/hit.rs:52    */
int rt_mesh(rt_scene*, const double* positions, uint32_t n_positions, const uint32_t* indices,
            uint32_t n_indices, int material);                       /* Mesh::new, src/mesh.rs:16 — returns the `tris` HittableList */
/* Mesh::load_obj(path, offset, scale, material), src/mesh.rs:33-61: tobj semantics for what the path uses (f32 positions widened,
 * fan triangulation, models[0] only, then `* scale + offset`); returns the `tris` HittableList; a malformed file is an error
 * (the reference unwraps tobj's Err, src/main.rs:431).  rt_parse_obj is its parsing step on a buffer: malloc'ed
 * positions (3 doubles each) and triangle indices, release with rt_free. */
int rt_mesh_load_obj(rt_scene*, const char* path, const double offset[3], double scale, int material);
int rt_parse_obj(const char* data, size_t size, const double offset[3], double scale, double** positions_out,
                 uint32_t* n_positions_out, uint32_t** indices_out, uint32_t* n_indices_out);
int rt_flip_normal(rt_scene*, int hittable);                                                           /* FlipNormal::new, src/hit.rs:105      */
int rt_translate(rt_scene*, int hittable, const double offset[3]);                                     /* Translate::new, src/translate.rs:13  */
int rt_rotate(rt_scene*, int axis, int hittable, double angle_deg);                                    /* Rotate::new, src/rotate.rs:32        */
/* ConstantMedium::new, src/medium.rs:17.  The boundary may be any Hittable but one that holds a ConstantMedium ("nested ConstantMedium is
 * not supported", at flatten time): a list of several objects — primitives, wrapped objects, BVHs, meshes — is searched as
 * HittableList::hit for each of the two boundary queries (medium.rs:29-30).  The medium may stand at the top level, under wrappers, in
 * BVH leaves. */
int rt_constant_medium(rt_scene*, int boundary, double density, int texture);
/* BVH::new, src/bvh.rs:18-73: `hittables` may be handles of ANY kind, as the reference's Vec<Box<dyn Hittable>> — bare primitives, lists,
 * FlipNormal / Translate / Rotate of anything (a Rotate child has the whole-space box of src/rotate.rs:40-57: such a tree is walked with
 * the exact box test everywhere), ConstantMedium, another BVH (one level of BVHs inside BVH leaves; deeper is an error at flatten time).
 * Errors where the reference panics: n = 0 ("no object in the scene", src/bvh.rs:55); a child without a bounding box — an empty list or a
 * wrapper of one ("no bounding box in bvh node", src/bvh.rs:28,61) — at flatten time.  BVHs nested more than RT_MAX_NEST deep inside
 * BVH leaves (a ConstantMedium's boundary counts as the level it stands at) are refused at flatten time. */
int rt_bvh(rt_scene*, const int* hittables, uint32_t n, double time0, double time1);
int rt_bvh_of_list(rt_scene*, int list, double time0, double time1);                                   /* BVH::new(list.list, ..), src/main.rs:442 */

/* the (world, lights) pair every scene fn returns, src/main.rs:153,278,348,453 */
int rt_scene_set_world(rt_scene*, int hittable);
/* lights.push (the reference's `lights` HittableList): AARect and Sphere (under any FlipNormals) are sampled; HittableLists nest (hit.rs:90-96:
 * pdf_value the mean over the items, random one item drawn uniformly), up to RT_MAX_LIGHT_NEST levels; anything else — Translate, Rotate,
 * Cube, BVH, MovingSphere, Triangle — has the trait defaults (pdf 0, direction (1,0,0)).  An empty nested list is an error at flatten time
 * (the reference panics, src/hit.rs:95; an empty top level is deviation D2). */
int rt_lights_push(rt_scene*, int hittable);

/* ---- host-side pieces of the boundary ------------------------------------------------------ */
/* Camera::new, src/camera.rs:19-49: origin, lower_left_corner, horizontal, vertical, cu, cv (3 each),
 * lens_radius, time0, time1 */
void rt_camera_fields(const rt_camera*, double out21[21]);
/* Vec3::format_color, src/vec.rs:125-131 (NaN -> 0, +inf -> 255) */
void rt_format_color(const double rgb_sum[3], uint64_t samples_per_pixel, uint64_t out3[3]);
/* PPM emitter, src/main.rs:767-769,832: "P3\nW H\n255\n" then one "r g b" line per pixel, rows top to
 * bottom.  rgb_sum is W*H*3 in output order (row 0 = top).  path NULL or "-" writes to stdout. */
int rt_write_ppm(const char* path, const double* rgb_sum, uint32_t W, uint32_t H, uint64_t samples_per_pixel);

/* Host asset ingest, `image::open(path).to_rgb8()` (src/main.rs:248,491): decodes a baseline JPEG (8-bit, grey or YCbCr,
 * 1x1 sampling — the class of the reference's earthmap.jpg) held in memory into a malloc'ed interleaved RGB8 buffer
 * (release with rt_free); NULL + rt_last_error() on anything else.  The result feeds rt_texture_image(). */
uint8_t* rt_decode_jpeg_rgb8(const uint8_t* data, size_t size, uint32_t* width, uint32_t* height);
void rt_free(void*);

/* Flatten the Hittable tree into the device scene (no GPU needed); fills counts for inspection:
 * objects, ops, rects, spheres, moving spheres, triangles, bvh nodes, materials, textures, lights, media, perlins */
int rt_scene_flatten(rt_scene*, uint32_t counts_out[12]);

/* ---- the hot path: replaces src/main.rs:772-833 -------------------------------------------- */
/* Renders the whole frame on the current HIP device and returns, per pixel, the SUM over samples of
 * ray_color (what `.sum()` yields at src/main.rs:830) as W*H*3 doubles in output order (row 0 = top,
 * i.e. j = H-1).  Fails (non-zero) if no GPU/HIP device is present: there is no CPU fallback. */
int rt_render(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
              uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
              double* rgb_sum_out);

/* Tile-sharded form for one-process-per-GPU use.  The image's W*H pixels (output order) are cut into
 * tiles of `tile_px` consecutive pixels; this call renders tiles t with t % world_size == rank into
 * d_out (DEVICE pointer, n_local_tiles * tile_px * 3 doubles, tile-major; pixels past W*H are zero),
 * asynchronously on `hip_stream` (a hipStream_t, may be NULL).  n_local_tiles =
 * rt_local_tiles(W,H,tile_px,rank,world_size) is the same on every rank (padded), so a plain gather
 * reassembles the frame. */
uint32_t rt_local_tiles(uint32_t W, uint32_t H, uint32_t tile_px, uint32_t rank, uint32_t world_size);
int rt_render_device(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                     uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
                     uint32_t tile_px, uint32_t rank, uint32_t world_size,
                     void* d_out, size_t d_out_bytes, void* hip_stream);
/* The same launch for samples [first_sample, first_sample + samples_per_pixel) of every pixel — the very samples a frame of more samples
 * per pixel and the same seed holds at those indices: a path's stream is keyed by z = seed + 2*((pixel << 32) | sample)*G (csrc/rt_rng.h),
 * so the offset is folded into the seed the launch receives, z(seed, pixel, sample + first) = z(seed + 2*first*G mod 2^64, pixel, sample)
 * while sample + first < 2^32; first_sample + samples_per_pixel > 2^32 - 1 is an error.  accumulate != 0: d_out is not zeroed first, the
 * pass is ADDED to what it holds (the kernels' only global writes are f64 atomic adds).  The building block of rt_progressive_* below for
 * one-process-per-GPU callers; asynchronous, never calibrates — like rt_render_device, which is this with (0, 0). */
int rt_render_device_pass(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                          uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
                          uint32_t first_sample, int accumulate,
                          uint32_t tile_px, uint32_t rank, uint32_t world_size,
                          void* d_out, size_t d_out_bytes, void* hip_stream);
/* (rt_render_device and rt_render_multi_device never wait: everything that has to — the first use of a scene on a device, see
 * rt_scene_prepare, and the loop-shape calibration of a mesh scene, see rt_scene_calibrate — is done inside them only as far as it can
 * be done without a wait; call those two first where it matters.) */
/* ---- progressive frames: the reference's loop shows its progress (`Scanlines remaining`, src/main.rs:772-775) and formats every pixel as
 *      it is finished (src/main.rs:832); rt_render is silent until the last sample.  A progressive frame owns a device-resident f64 sum
 *      frame for ONE fixed view of one scene, takes passes of samples that accumulate into it, and resolves it to the reference's 8-bit
 *      output ON THE DEVICE at any time: progress, preview, "another 1000 samples", stop half-way, save and resume.
 * The handle is an opaque pointer (`void* frame`; NULL + rt_last_error() when create fails).  The sum frame, the RGB8 image and the
 * previous RGB8 image live on the HIP device that was current at create; every call below works on that device whatever the current
 * device is, and restores it.  rt_render* are untouched, and a frame and one-shot renders of the same scene may be interleaved freely.
 * A change to the scene after create makes the next add an error (the scene forgets everything on a change; so does the frame) until
 * rt_progressive_reset; a frame outlives its scene (it can still be resolved, read and destroyed; add is an error). */
/* One fixed view: the arguments of rt_render without the sample count.  Fails without a HIP device, as rt_render does. */
void* rt_progressive_create(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                            uint32_t max_depth, uint64_t seed, uint32_t flags);
/* One pass of the sample loop src/main.rs:811-830: samples [done, done + n_samples) of every pixel — the very samples rt_render with
 * samples_per_pixel >= done + n_samples and the same seed renders at those indices (rt_render_device_pass) — added to the frame.
 * samples_out (NULL, or n_samples*W*H*3 doubles) receives the pass's samples laid out as rt_render_samples lays out a frame of n_samples.
 * Errors, nothing launched: n_samples = 0; done + n_samples > 2^32 - 1.  Goes through the launch rt_render uses (loop shape, filter tuning,
 * chunking; rt_last_kernel_ms, rt_last_stats, rt_last_loop_info report the pass).  Synchronous; it tunes / calibrates as rt_render does,
 * deciding by the VIEW as accumulated so far: a mesh scene's loop shape is measured at the pass with which W*H*(done + n_samples) reaches
 * the 1e8 samples at which a one-shot frame measures it (either shape gives the same samples, so a frame may change shape between passes). */
int rt_progressive_add(void* frame, uint32_t n_samples, double* samples_out);
/* The same pass enqueued on hip_stream (a hipStream_t of the frame's device, may be NULL); never waits, never calibrates — like
 * rt_render_device.  Passes on different streams may overlap: they only ever add. */
int rt_progressive_add_async(void* frame, uint32_t n_samples, void* hip_stream);
int rt_progressive_samples(void* frame, uint64_t* done_out);               /* samples per pixel accumulated so far (enqueued passes included) */
/* Vec3::format_color(samples done), src/vec.rs:125-131, for every pixel ON THE DEVICE (csrc/rt_resolve.hip) — equal to rt_format_color
 * on every input, bit for bit — copied to rgb8_out (W*H*3 bytes, output order: what src/main.rs:832 prints).  *changed_px_out (may be
 * NULL): the pixels whose triple differs from the previous resolve of this frame — a convergence signal: stop when the 8-bit image has
 * stopped moving; the first resolve of a frame (also after load_sum / reset) reports W*H.  Waits for every pass enqueued so far.
 * An error while the frame holds 0 samples. */
int rt_progressive_resolve_rgb8(void* frame, uint8_t* rgb8_out, uint64_t* changed_px_out);
/* The same resolve enqueued on hip_stream, never waits: *d_rgb8_out (may be NULL) receives the DEVICE address of the W*H*3 bytes, owned by
 * the frame.  Resolves alternate between TWO images, so an address stays valid, and its pixels untouched, until the next-but-one resolve.
 * Ordered after the passes of the same stream only.  rt_progressive_copy_rgb8 waits and copies the most recent resolve and its
 * changed-pixel count to host memory without resolving again: rt_progressive_resolve_rgb8 = wait + the two. */
int rt_progressive_resolve_rgb8_device(void* frame, void** d_rgb8_out, void* hip_stream);
int rt_progressive_copy_rgb8(void* frame, uint8_t* rgb8_out, uint64_t* changed_px_out);
/* The accumulated sums, W*H*3 doubles in output order, as rt_render returns them (waits for the passes enqueued so far): with
 * rt_progressive_samples, a checkpoint.  The f64 atomic adds reach a pixel in no fixed order, so sums of the same samples differ between
 * runs and from rt_render's within the bound that holds for any order of adding N terms, 2*gamma*sum|x_i|, gamma = (N-1)u / (1 - (N-1)u), u = 2^-53. */
int rt_progressive_read_sum(void* frame, double* rgb_sum_out);
/* Resume from a checkpoint: the frame becomes rgb_sum (W*H*3 doubles) holding samples_done samples per pixel; the next pass starts at sample
 * samples_done.  Errors: samples_done > 2^32 - 1; samples_done = 0 with a frame that is not all zero. */
int rt_progressive_load_sum(void* frame, const double* rgb_sum, uint64_t samples_done);
/* Back to 0 samples, same view — of the scene as it is now (this is what makes a frame usable again after the scene changed). */
int rt_progressive_reset(void* frame);
void rt_progressive_destroy(void* frame);                                  /* waits for the frame's work; the scene may be gone already */

/* ---- moments: the per-pixel error estimate of a frame that accumulates passes, and a statistical stop.  The changed-pixel count of a
 *      resolve depends on the pass size and on when the caller resolves, and says nothing per pixel; a standard error does.  The path-tracing
 *      kernels gather no second moment.  It is taken BETWEEN passes, from the pass frames themselves (batch means): a pass of n_b samples is
 *      rendered into a pass frame p of its own and merged,   S += p,   Q += p*p / n_b   (per pixel and channel),   and for B >= 2 passes and
 *      N samples the between-pass sum of squares  ssb = max(Q - S*S/N, 0)  estimates (B - 1) sigma^2 — for unequal n_b too — so that
 *      V = ssb / (B - 1) / N is the variance of the mean m = S / N, and  e2 = V / (4 max(m, 2^-8))  the squared standard error of what
 *      format_color shows, sqrt(m), in display units (1/256 = one code value); a channel whose mean lies three standard errors above the
 *      clamp counts as 0; a pixel's e2 is the largest of its three channels'.  csrc/rt_moments.h is the exact specification — + - * / and
 *      comparisons in a fixed order — and the host forms, the HIP kernels (csrc/rt_moments.hip) and the NumPy restatement of
 *      tests/moments_cases.py give the same 64-bit words.
 * The building blocks, for one-process-per-GPU callers of rt_render_device_pass too.  n_doubles = 3 * pixels; every frame 8-byte aligned.
 * rt_moments_merge_host merges pass_sum into rgb_sum and sq_sum and leaves pass_sum as it is.  rt_moments_merge_device does the same for
 * DEVICE pointers (three distinct buffers; 16-byte accesses when all are 16-byte aligned) on hip_stream (a hipStream_t, may be NULL), never
 * waits, never allocates, and sets d_pass_sum to +0.0: the pass frame is ready for the next rt_render_device_pass(accumulate = 1), so a pass
 * costs no memset of its own.  Errors (non-zero, a message for rt_last_error, nothing written or launched): null pointers, n_samples = 0. */
int rt_moments_merge_host(const double* pass_sum, uint64_t n_samples, double* rgb_sum, double* sq_sum, uint64_t n_doubles);
int rt_moments_merge_device(void* d_pass_sum, uint64_t n_samples, void* d_rgb_sum, void* d_sq_sum, uint64_t n_doubles, void* hip_stream);
/* e2 of every pixel (W*H doubles, output order) from the sums of `passes` passes holding `samples` samples per pixel.  Errors: null
 * pointers, passes < 2, samples = 0, W*H = 0 or > 2^31 - 1. */
int rt_moments_error_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H, double* e2_out);
/* The statistics of an error map for a threshold tau (a standard error in display units): stats_out[0] = converged, the pixels with e2 finite
 * and e2 <= tau*tau; [1] = unconverged, e2 finite and > tau*tau; [2] = nonfinite, the rest; [3] = the bit pattern of the largest finite e2
 * (+0.0 when there is none).  All four are exact, whatever the order of the pixels.  Errors: null pointers, tau negative or NaN. */
int rt_moments_stats_host(const double* e2, uint64_t n_px, double tau, uint64_t stats_out[4]);
/* Both on the device, enqueued on hip_stream; never waits, never allocates.  d_e2_out (W*H doubles) and d_stats_out (four 64-bit words,
 * zeroed in stream order by this call) may each be NULL; tau is looked at only with d_stats_out. */
int rt_moments_error_device(const void* d_rgb_sum, const void* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H,
                            void* d_e2_out, double tau, void* d_stats_out, void* hip_stream);
/* A progressive frame with moments.  Allowed only while the frame holds 0 samples (an error otherwise); allocates the second-moment frame
 * and the pass frame, zeroed (48 more bytes per pixel).  From then on a pass renders into the pass frame and is followed by the merge kernel on
 * the same stream: the frame's sums are the merge-order sum of the pass frames — still within the any-order bound rt_progressive_read_sum
 * states — and resolve, read_sum, both denoised resolves and samples_out work unchanged.  Passes of rt_progressive_add_async on different
 * streams share the pass frame: the frame records an event behind every merge and makes the next pass's stream wait for it
 * (hipStreamWaitEvent), so the host still never waits and the passes SERIALISE on the device instead of overlapping.  A frame that never
 * enables moments takes exactly the path it took before.  rt_progressive_reset zeroes the second moments and the pass count and keeps
 * moments enabled.  rt_progressive_load_sum keeps working and marks the moments INVALID (the sums would hold samples the second moments do
 * not): the error calls then fail with a message until rt_progressive_reset or rt_progressive_load_moments. */
int rt_progressive_enable_moments(void* frame);
int rt_progressive_passes(void* frame, uint64_t* passes_out);             /* passes merged so far (enqueued ones included); 0 without moments */
/* The second moments, W*H*3 doubles (waits for the passes enqueued so far): with rt_progressive_read_sum, rt_progressive_samples and
 * rt_progressive_passes, a checkpoint — which rt_progressive_load_moments resumes from (samples_done <= 2^32 - 1; 0 samples or 0 passes only
 * with frames that are all zero, and with each other). */
int rt_progressive_read_moments(void* frame, double* sq_sum_out);
int rt_progressive_load_moments(void* frame, const double* rgb_sum, const double* sq_sum, uint64_t samples_done, uint64_t passes);
/* rt_moments_error_device on the frame's own sums.  error_map: e2 of every pixel to host memory (W*H doubles); error_map_device: enqueued
 * on hip_stream, never waits, *d_e2_out receives the DEVICE address of the W*H doubles, a buffer owned by the frame and allocated at the
 * first call; error_stats: the four words of rt_moments_stats_host for tau.  error_map and error_stats wait for every pass enqueued so
 * far, as rt_progressive_resolve_rgb8 does.  Errors: a frame without moments, moments invalid, fewer than 2 passes, tau negative or NaN. */
int rt_progressive_error_map(void* frame, double* e2_out);
int rt_progressive_error_map_device(void* frame, void** d_e2_out, void* hip_stream);
int rt_progressive_error_stats(void* frame, double tau, uint64_t stats_out[4]);
/* The variance of the mean of every pixel and channel, V above, as a frame of its own (W*H*3 doubles, output order; csrc/rt_moments.h (4)) —
 * what the variance-guided denoiser below (rt_denoise_variance*) takes as its input.  e2 is computed from this very V.  A channel whose
 * state is not finite has V = 0, except for a +inf in Q, which gives +inf.  The host form needs no device; the device form only enqueues
 * on hip_stream (8-byte aligned buffers, d_var_out neither input; 16-byte accesses when all three are 16-byte aligned), never waits, never
 * allocates; rt_progressive_variance is the device form on the frame's own sums, into a buffer of the frame's own (24 more bytes per pixel,
 * allocated at the first call), copied out; it waits for every pass enqueued so far.  Errors: those of the error calls above. */
int rt_moments_variance_host(const double* rgb_sum, const double* sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H, double* var_out);
int rt_moments_variance_device(const void* d_rgb_sum, const void* d_sq_sum, uint64_t samples, uint64_t passes, uint32_t W, uint32_t H,
                               void* d_var_out, void* hip_stream);
int rt_progressive_variance(void* frame, double* var_out);

/* ---- adaptive frames: a progressive frame with moments knows, pixel by pixel, which pixels are finished; an ADAPTIVE frame stops sampling
 *      them.  THE INVARIANT: pixel p of an adaptive frame with count n[p] holds exactly samples 0 .. n[p] - 1 of the streams
 *      rt_rng_path(seed, p, s) — the very samples rt_render with the same view and seed holds at those indices.  A pass has ONE size n_b:
 *      a listed pixel receives samples [n[p], n[p] + n_b); no seed folding, the kernel reads the pixel's own first sample.  Per pixel,
 *      beside the sums S and the second moments Q: n[p] (uint32) the samples done, b[p] (uint32) the passes the pixel took part in.
 *      csrc/rt_adaptive.h is the exact specification — (A) the error with counts: e2 of rt_moments_error_* with (n[p], b[p]) in the frame's
 *      counts' place, +inf while b[p] < 2; (B) the selection: need = b < 2 or e2 finite and > tau*tau; with spread = 1 also the pixels with
 *      a needing neighbour (8-neighbourhood inside the frame: a pixel whose passes held no bright path yet looks converged, its neighbours
 *      know better); active = needed and n + n_b <= max_samples; the LIST is the active pixels' output-order indices in ASCENDING order;
 *      (C) the list merge: rt_moments_merge_* for the listed pixels, pass frame zeroed, n += n_b, b += 1, nothing else read or written;
 *      (D) the resolve: rt_format_color(S[p], n[p]), 0 where n[p] = 0 — and the host forms, the HIP kernels (csrc/rt_adaptive.hip) and the
 *      NumPy restatement of tests/adaptive_cases.py give the same words.
 * The path-tracing building block: n_samples samples of every pixel of d_list (n_list output-order indices, uint32, DEVICE memory) of the
 * W x H view, ADDED to d_out (W*H*3 doubles, output order, 8-byte aligned: a pass frame): pixel p receives samples [d_counts[p], + n_samples)
 * (d_counts: W*H uint32 in DEVICE memory, or NULL for first sample 0 everywhere).  f64 and the reference's traversal order only: flags may
 * hold RT_STOP_ON_ZERO and RT_ISOTROPIC_SCATTER.  Enqueued on hip_stream, never waits, never allocates; a scene not yet on the device is
 * uploaded first (rt_scene_prepare).  n_list = 0 is a no-op.  A list entry that is not a pixel of the frame, or whose count + n_samples
 * would pass 2^32 - 1 (the sample field of a path's RNG key), is skipped on the device: nothing is traced or written for it — rt_adaptive_select_*
 * never lists such a pixel, and the frame calls below refuse such a pass on the host.  rt_last_query_ms reports the kernel. */
int rt_render_pixels_device(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                            uint32_t n_samples, uint32_t max_depth, uint64_t seed, uint32_t flags,
                            const void* d_list, uint32_t n_list, const void* d_counts, void* d_out, size_t d_out_bytes, void* hip_stream);
/* (A): e2_out (W*H doubles) and stats_out (the four words of rt_moments_stats_host for tau) may each be NULL.  The host form needs no
 * device; the device form only enqueues (d_stats_out is zeroed in stream order by the call).  Errors: null pointers, W*H = 0 or > 2^31 - 1,
 * tau negative or NaN (looked at only with stats). */
int rt_adaptive_error_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H,
                           double* e2_out, double tau, uint64_t stats_out[4]);
int rt_adaptive_error_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                             void* d_e2_out, double tau, void* d_stats_out, void* hip_stream);
/* (B): the list (room for W*H uint32) and its length.  The device form needs rt_adaptive_select_workspace_bytes(W, H) bytes of 16-byte
 * aligned DEVICE memory (about 2 bytes per pixel) and writes the length to d_n_list_out (one uint32, DEVICE memory): count, scan, scatter,
 * four launches, no wait.  Errors: null pointers, the frame as above, n_samples = 0, tau negative or NaN, max_samples > 2^32 - 1, spread > 1. */
int rt_adaptive_select_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H,
                            uint32_t n_samples, double tau, uint64_t max_samples, uint32_t spread, uint32_t* list_out, uint32_t* n_list_out);
size_t rt_adaptive_select_workspace_bytes(uint32_t W, uint32_t H);
int rt_adaptive_select_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                              uint32_t n_samples, double tau, uint64_t max_samples, uint32_t spread, void* d_list_out, void* d_n_list_out,
                              void* d_workspace, size_t workspace_bytes, void* hip_stream);
/* (C).  The host form checks its list (ascending, inside the frame, count + n_samples <= 2^32 - 1) before it writes anything; the device
 * form cannot and relies on a list of rt_adaptive_select_device's making. */
int rt_adaptive_merge_host(double* pass_sum, uint32_t n_samples, double* rgb_sum, double* sq_sum, uint32_t* counts, uint32_t* passes,
                           const uint32_t* list, uint32_t n_list, uint32_t W, uint32_t H);
int rt_adaptive_merge_device(void* d_pass_sum, uint32_t n_samples, void* d_rgb_sum, void* d_sq_sum, void* d_counts, void* d_passes,
                             const void* d_list, uint32_t n_list, void* hip_stream);
/* (D): rgb8_out (W*H*3 bytes) and the number of pixels whose triple differs from rgb8_prev's (NULL: every pixel counts).  The device form
 * ADDS that number to *d_changed_px_out (one 64-bit word, may be NULL; the caller zeroes it in stream order). */
int rt_adaptive_resolve_rgb8_host(const double* rgb_sum, const uint32_t* counts, uint32_t W, uint32_t H, const uint8_t* rgb8_prev, uint8_t* rgb8_out,
                                  uint64_t* changed_px_out);
int rt_adaptive_resolve_rgb8_device(const void* d_rgb_sum, const void* d_counts, uint32_t W, uint32_t H, const void* d_rgb8_prev, void* d_rgb8_out,
                                    void* d_changed_px_out, void* hip_stream);
/* A progressive frame with moments becomes adaptive: allowed only while it holds 0 samples; allocates the counts, the list and the selection's
 * workspace (about 14 more bytes per pixel).  An error without moments, and when the frame's flags hold anything but RT_STOP_ON_ZERO and
 * RT_ISOTROPIC_SCATTER (the list kernel runs f64 and the reference's traversal order only).  From then on:
 *   rt_progressive_add is a pass over ALL pixels; rt_progressive_add_async is an error; rt_progressive_samples returns the largest n[p];
 *   rt_progressive_resolve_rgb8* use (D); error_map, error_map_device and error_stats use (A) (they need two passes of the frame, not of every pixel);
 *   rt_progressive_reset zeroes the counts; rt_progressive_read_sum / read_moments work as before;
 *   rt_progressive_variance, the three denoised resolves, rt_progressive_load_sum and rt_progressive_load_moments are errors while the counts
 *   are not uniform (all n[p] equal and all b[p] equal, which the host tracks), and behave as before while they are;
 *   rt_progressive_variance_counts and rt_progressive_resolve_denoised_frame_rgb8 (below) take the frame as it is.
 * While every pixel is listed and the frame is uniform a pass goes through the launch rt_progressive_add uses — the frames' own kernels are
 * the fast ones — followed by (C) over all pixels; otherwise through rt_render_pixels_device and the list merge. */
int rt_progressive_enable_adaptive(void* frame);
/* Select (B) with (n_samples, tau, max_samples, spread), render the listed pixels, merge (C), wait.  info_out: [0] the listed pixels, [1] the
 * samples rendered by this pass (listed * n_samples), [2] the sum of n[p] over the frame afterwards, [3] the kernel used: 0 = the frames'
 * kernel, 1 = the list kernel.  With nothing listed it renders nothing and returns 0 with info_out[0] = 0: the stop condition.  max_samples =
 * 0 means 2^32 - 1.  Errors, nothing launched: not an adaptive frame, n_samples = 0, tau negative or NaN, max_samples > 2^32 - 1, spread > 1,
 * the scene destroyed or changed. */
int rt_progressive_add_adaptive(void* frame, uint32_t n_samples, double tau, uint64_t max_samples, uint32_t spread, uint64_t info_out[4]);
/* The counts (W*H uint32 each; either may be NULL; waits): with read_sum and read_moments, a checkpoint — which rt_progressive_load_adaptive
 * resumes from.  Errors of the load: not an adaptive frame, b[p] > n[p], n[p] = 0 with a pixel that is not all zero. */
int rt_progressive_read_counts(void* frame, uint32_t* counts_out, uint32_t* passes_out);
int rt_progressive_load_adaptive(void* frame, const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes);

/* ---- ray queries: the reference's `world.hit(r, 0.00001, f64::INFINITY)` (src/main.rs:48, Hittable::hit) as a function of its own — the
 *      closest hit of rays the caller chooses, or of the camera rays of one sample of every pixel: which object is under pixel (i, j), how far
 *      away it is (auto-focus), depth / normal / material-id frames for a denoiser or a compositor, visibility probes.  The search and the
 *      record are the frames' own device code (csrc/rt_query.hip), for every kind of scene; no shading.  f64 and the reference's traversal
 *      order only: `flags` must be 0 (RT_F32 and every other flag are an error); t_max is +inf; one device, the current one.
 * A ray is 7 doubles: origin[3], direction[3], time.  Non-finite and zero direction components are legal.
 * A hit record is 16 doubles (128 bytes): [0] hit (0 / 1), [1] t, [2..4] position, [5..7] normal, [8] front_face, [9], [10] u, v — computed
 * where the hit's material reads them (only an ImageTexture does, as in the frames), 0 elsewhere —, [11] the material handle rt_material_*
 * returned (handles are indices of the scene's material table; a ConstantMedium hit reports -1: its Isotropic is made by the flattener and
 * has no handle), [12] the object's index in the flattened object table as rt_debug_objects numbers it, [13] the primitive kind (0 rect,
 * 1 sphere, 2 moving sphere, 3 triangle, -1 medium), [14] the index in that primitive pool (-1 medium), [15] 0.  A miss is [0] = 0,
 * [11..14] = -1 and the rest 0.
 * The host forms are synchronous.  The _device forms take DEVICE pointers, 16-byte aligned, only enqueue on hip_stream (a hipStream_t, may be
 * NULL) and never wait.  A scene not yet prepared is flattened and uploaded first, as rt_render_device does it.  Errors (non-zero, a message
 * for rt_last_error, nothing launched): null arguments, flags != 0, d_hits_bytes < 128 bytes per record, W < 2 or H < 2, W*H > 2^31 - 1, no
 * HIP device (there is no CPU path).  n = 0 returns 0 and touches nothing.  Queries leave what rt_last_kernel_ms and friends report alone. */
/* Camera::get_ray for sample `sample` of pixel (i, j), j counted from the BOTTOM row as main.rs:811-820 does: the draws of
 * rng_for_path(seed, (H-1-j)*W + i, sample) in the kernels' order (refill_queue): u, v, lens disk (rejection loop), time.
 * Host only, no GPU.  ray_out = origin[3], direction[3], time. */
int rt_camera_ray(const rt_camera*, uint32_t W, uint32_t H, uint32_t i, uint32_t j, uint64_t seed, uint32_t sample, double ray_out[7]);
/* world.hit(ray, t_min, +inf) for n caller rays: rays = n x 7 (origin[3], direction[3], time), hits_out = n x 16 doubles.  ConstantMedium::hit
 * draws a random number (src/medium.rs:28): ray k draws from the stream of rt_rng_create(seed, k). */
int rt_query_hits(rt_scene*, uint32_t n, const double* rays, double t_min, uint64_t seed, uint32_t flags, double* hits_out);
int rt_query_hits_device(rt_scene*, uint32_t n, const void* d_rays, double t_min, uint64_t seed, uint32_t flags,
                         void* d_hits_out, size_t d_hits_bytes, void* hip_stream);
/* The camera ray of sample `sample` of every pixel, generated ON THE DEVICE (the very ray a frame with that seed traces for that
 * sample), and its closest hit with t_min = 0.00001: the path's own stream simply continues after the camera's draws, so the hit is the one
 * a frame finds at depth 0.  W*H records in output order (row 0 = top).  rays_out may be NULL (else W*H*7). */
int rt_query_camera(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t sample, uint64_t seed, uint32_t flags,
                    double* rays_out, double* hits_out);
int rt_query_camera_device(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t sample, uint64_t seed, uint32_t flags,
                           void* d_rays_out, void* d_hits_out, size_t d_hits_bytes, void* hip_stream);
int rt_last_query_ms(rt_scene*, float* ms_out);   /* HIP events around the most recent query kernel of this scene (ray or radiance query); waits */
/* Geometry of that kernel's launch — the most recent ray, albedo or radiance query or pixel-list pass (rt_render_pixels_device) of this scene —
 * as the host computed it: [0] workgroups launched, [1] threads per workgroup, [2] paths per chunk and [3] number of chunks of a radiance query
 * or pixel-list pass (saturating at 2^32 - 1), both 0 for a ray or albedo query, which have no chunks: n rays with n > [0] * [1] take a lane
 * through its loop more than once, [3] > [0] * [1] / 64 gives a wave a second chunk.  Read-only, waits for nothing; -1 before the first query. */
int rt_last_query_launch(rt_scene*, uint32_t out4[4]);

/* ---- albedo queries: the reflectance at the closest hit, for rays the caller chooses or summed over a range of samples of every pixel's
 *      camera ray — the albedo frame a denoiser divides a textured frame by (rt_denoise_albedo* below), or a compositor's base-colour pass.
 *      The closest hit is found exactly as rt_query_hits / rt_query_camera find it (the same search, stream and record) and its albedo is
 *      (csrc/rt_albedo.h, the definition; csrc/rt_albedo.hip, the kernels):
 *        Lambertian: Texture::mapping(u, v, p) of its texture, the frames' own texture walk on the record (constant, checker, Perlin noise,
 *        image); PBR: the same of its base-colour texture; a ConstantMedium hit (handle -1): the same of the medium's texture; Metal: its
 *        albedo; Dielectric, DiffuseLight and a miss: (1, 1, 1) — radiance of emitters and of the background is not reflectance and stays
 *        un-demodulated.  The albedo is the FIRST hit's; rt_query_chain* below follow specular chains to the first rough surface.
 * rt_query_albedo: albedo_out = n x 3 doubles; hits_out: NULL, or n x 16 — the very words rt_query_hits writes for these rays and this seed.
 * rt_query_camera_albedo: albedo_sum_out = W*H*3 doubles in output order, per pixel the SUM over samples first_sample .. first_sample +
 * n_samples - 1 of the albedo under that sample's camera ray (the ray of rt_query_camera(sample)), added in ascending order into
 * accumulators that start at +0.0 — one pixel per lane, no atomics: the same call gives the same words, and the sum of single-sample calls
 * restates it exactly.  Divide by n_samples for the mean.  n_samples >= 1 and first_sample + n_samples <= 2^32 - 1.
 * Everything else — flags = 0, f64, errors, n = 0, the _device forms (DEVICE pointers: rays and hits 16-byte aligned, albedo 8-byte; they only
 * enqueue on hip_stream and never wait or allocate), rt_last_query_ms — is as for the ray queries above. */
int rt_query_albedo(rt_scene*, uint32_t n, const double* rays, double t_min, uint64_t seed, uint32_t flags, double* albedo_out, double* hits_out);
int rt_query_albedo_device(rt_scene*, uint32_t n, const void* d_rays, double t_min, uint64_t seed, uint32_t flags,
                           void* d_albedo_out, size_t d_albedo_bytes, void* d_hits_out, size_t d_hits_bytes, void* hip_stream);
int rt_query_camera_albedo(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples,
                           uint64_t seed, uint32_t flags, double* albedo_sum_out);
int rt_query_camera_albedo_device(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples,
                                  uint64_t seed, uint32_t flags, void* d_albedo_sum, size_t d_albedo_sum_bytes, void* hip_stream);

/* ---- averaged denoising guides: the first-hit records of n_samples camera samples of every pixel reduced to ONE record in the layout of
 *      rt_query_camera, so that every `hits` parameter of the denoise family below takes it unchanged — a guide that sees what the lens,
 *      the shutter and the pixel's area see, where sample 0's record sees one ray.  An exact f64 specification (csrc/rt_guide.h: only + /
 *      comparisons and integer counts, a fixed order) that the HIP kernel (csrc/rt_guide.hip) and the host twin satisfy bit for bit.
 * Per pixel, over the records r_s of rt_query_camera(sample = s), s = first_sample .. first_sample + n_samples - 1 ascending: h = the number
 * with hit != 0, hf = the number of those with front_face != 0; t, position and normal are summed over the hitting records only, in
 * ascending order, into accumulators that start at +0.0.  The record:
 *   [0] hit = 1.0 if h >= 1 and 2 h >= n_samples (the majority, a tie counting as hit), else 0.0;  [1] t, [2..4] position, [5..7] normal =
 *   sum / h (0 when h = 0; the normal is NOT renormalised: an edge pixel's short normal is information);  [8] front_face = hf / h, a
 *   fraction;  [9], [10] u, v = 0.0;  [11] material, [12] object = the common value over the hitting records (a medium's -1 is a value
 *   like any other), -1 when they differ or h = 0;  [13], [14] = -1;  [15] hits = (double) h, the coverage count (rt_query_camera writes
 *   0.0 there and no reader uses it).
 * n_samples = 1 gives words [0]-[8], [11], [12] of rt_query_camera(first_sample) as values (a -0.0 component becomes +0.0 through the
 * accumulator).  A pixel whose samples mix materials has material -1: key 1 under RT_DENOISE_SAME_MATERIAL, as a medium, never a miss's 0.
 * A pixel whose samples mostly miss is a miss to the filters; words [1]-[8] and [15] still carry what the hitting samples saw.
 * rt_query_camera_guide: guide_out = W*H*16 doubles in output order; albedo_sum_out: NULL, or W*H*3 doubles — the very words
 * rt_query_camera_albedo(first_sample, n_samples) writes, from the SAME searches (one search per sample instead of two for a caller who
 * wants both).  n_samples >= 1 and first_sample + n_samples <= 2^32 - 1.  Everything else — flags = 0, f64, errors, the _device form (DEVICE
 * pointers: d_guide 16-byte aligned, d_albedo_sum 8-byte and may be NULL; it only enqueues on hip_stream and never waits or allocates; a
 * buffer that is too small is an error and nothing is launched), rt_last_query_ms, rt_last_query_launch — is as for rt_query_camera_albedo*.
 * rt_guide_from_hits_host: the specification on the host, no GPU: hits = n_samples x n_px x 16 doubles (sample-major: the stacked outputs
 * of rt_query_camera), guide_out = n_px x 16.  Errors: null arguments, n_samples = 0.
 * Not done: a coverage or depth-spread stop inside the filters (they read words [0]-[7] and [11] only), f32, rt_render_multi.  Following
 * specular chains: rt_query_camera_chain_guide* below. */
int rt_query_camera_guide(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples,
                          uint64_t seed, uint32_t flags, double* guide_out, double* albedo_sum_out);
int rt_query_camera_guide_device(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples,
                                 uint64_t seed, uint32_t flags, void* d_guide, size_t d_guide_bytes,
                                 void* d_albedo_sum, size_t d_albedo_sum_bytes, void* hip_stream);
int rt_guide_from_hits_host(const double* hits, uint32_t n_samples, uint64_t n_px, double* guide_out);
/* A progressive frame's denoising guide: guide_samples = 1 (the default) is rt_query_camera(sample 0, the frame's seed); n > 1 is
 * rt_query_camera_guide(first_sample 0, n, the frame's seed).  Setting another value drops the packed guide; the next denoised resolve of any
 * kind builds it (rt_query_camera_guide_device on the frame's device; rt_last_query_ms reports that launch then) and keeps it until
 * rt_progressive_reset or another value.  n = 0 is an error.  rt_progressive_guide_info: the value in force and how many guides the frame
 * has built so far.  The frame's albedo sums are built as before, by their own launch. */
int rt_progressive_set_guide_samples(void* frame, uint32_t n_samples);
int rt_progressive_guide_info(void* frame, uint32_t* guide_samples_out, uint64_t* builds_out);

/* ---- specular-chain guides: the record and the albedo at the first NON-specular surface along the deterministic specular path of a ray,
 * for denoising guides and albedo frames in which a mirror or a glass ball shows what is seen in it, not its own smooth surface
 * (csrc/rt_chain.h: the exact f64 definition (C1)-(C8) and the link step; csrc/rt_chain.hip: the kernel).  Briefly:
 *   (C1) link l searches world.hit(r_l, t_min, +inf) as rt_query_hits does; link 0 draws from rt_query_hits' / rt_query_camera's stream, link
 *        l >= 1 of item k from rng_for_stream(seed + ((sample_index << 8) | l) * 0x9E3779B97F4A7C15, k) (sample_index 0 for caller rays):
 *        link l of all items is one rt_query_hits call.  The step draws nothing.
 *   (C2) the chain ends at a miss, at l = max_links (0 .. 64), at a medium hit, at a material that is neither Metal nor Dielectric, at a Metal
 *        with !(fuzz <= max_fuzz) (max_fuzz >= 0 or +inf), at a new direction that is not finite, and at a Metal whose reflected direction
 *        has !(dot(new_d, n) > 0) (the frames absorb that path, main.rs:108-110).
 *   (C3) Metal: the centre of the lobe, reflect(d, n) normalised (mat.rs:280-293 without the fuzz term); the weight is multiplied by its albedo.
 *   (C4) Dielectric: mat.rs:343-374 expression for expression with `refl > 0.5` in the place of the random draw; weight unchanged.
 *   (C5) the new ray starts at the record's position, time unchanged.
 *   (C6) the record is the LAST link's, in rt_query_hits' layout, but word [1] = the path length in units of the first ray's parameter
 *        ((t_0 L_0 + t_1 L_1 + ...) / L_0, L_l the length of link l's direction; with 0 links the record's own t, bit for bit) and word [15] =
 *        the number of links followed.  A chain that ends in a miss has hit = 0.
 *   (C7) the chain albedo is the weight times rt_query_albedo's table on the last record ((1, 1, 1) for a miss).
 *   (C8) camera form: the chain records of samples first_sample .. first_sample + n_samples - 1 reduced by rt_query_camera_guide's rule
 *        (word [15] = the hit count), the chain albedos summed in ascending order, links_out (may be NULL) = per pixel the links followed
 *        over all samples.
 * With max_links = 0 the words are those of rt_query_hits, rt_query_albedo and rt_query_camera_guide.  albedo outputs may be NULL.
 * Errors: max_links > 64, a negative or NaN max_fuzz, flags != 0, and rt_query_albedo* / rt_query_camera_guide*'s own (null arguments, sizes,
 * alignment, ranges).  The _device forms take DEVICE pointers (rays, hits, guide 16-byte aligned, albedo 8-byte, links 4-byte), check the sizes,
 * only enqueue on hip_stream and never wait or allocate; a buffer that is too small is an error and nothing is launched.  rt_last_query_ms and
 * rt_last_query_launch report these launches (threads per workgroup: rt_debug_loop_limits word [12]).
 * rt_chain_step_host: the link step (C2)-(C5) on the host, no GPU, on n (ray, record) pairs; the material comes from the scene's host-side table
 * by the record's word [11].  next_rays_out n x 7: the new ray where status is 0, else the input ray; weight_out n x 3: the factor of this
 * link (a followed Metal's albedo, else (1, 1, 1)); status_out: 0 continue, 1 ended at a non-specular surface, 2 miss, 3 absorbed, 4 not
 * finite, 5 fuzz above the limit.  max_links is the caller's loop.  A word [11] that names no material is an error and nothing is written.
 * Not done: chain records in reprojection, the Fresnel split as two weighted branches, refilling ended lanes, f32, rt_render_multi. */
int rt_query_chain(rt_scene*, uint32_t n, const double* rays, double t_min, uint64_t seed, uint32_t max_links, double max_fuzz, uint32_t flags,
                   double* hits_out, double* albedo_out);
int rt_query_chain_device(rt_scene*, uint32_t n, const void* d_rays, double t_min, uint64_t seed, uint32_t max_links, double max_fuzz, uint32_t flags,
                          void* d_hits_out, size_t d_hits_bytes, void* d_albedo_out, size_t d_albedo_bytes, void* hip_stream);
int rt_query_camera_chain_guide(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                                uint32_t max_links, double max_fuzz, uint32_t flags, double* guide_out, double* albedo_sum_out, uint32_t* links_out);
int rt_query_camera_chain_guide_device(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, uint32_t first_sample, uint32_t n_samples, uint64_t seed,
                                       uint32_t max_links, double max_fuzz, uint32_t flags, void* d_guide, size_t d_guide_bytes,
                                       void* d_albedo_sum, size_t d_albedo_sum_bytes, void* d_links, size_t d_links_bytes, void* hip_stream);
int rt_chain_step_host(rt_scene*, uint32_t n, const double* rays, const double* hits, double max_fuzz,
                       double* next_rays_out, double* weight_out, uint32_t* status_out);
/* A progressive frame's guide through specular chains: after set_guide_chain(L > 0, max_fuzz) every denoised resolve builds its guide AND its
 * albedo sums from rt_query_camera_chain_guide_device(first_sample 0, the frame's guide_samples, the frame's seed, L, max_fuzz) — one launch.
 * The albedo resolves then demodulate by those sums over guide_samples: their albedo_samples argument only says that the frame is demodulated.
 * Setting another value drops the packed guide and the albedo sums, as rt_progressive_set_guide_samples does.  L = 0 (the default): the
 * frame is byte for byte what it is without this call.  rt_progressive_set_view reprojects with FIRST-hit records whatever the setting
 * (a chain record's point is not seen directly from the camera).  Checkpoints do not carry the setting.  Errors: L > 64, max_fuzz negative or NaN. */
int rt_progressive_set_guide_chain(void* frame, uint32_t max_links, double max_fuzz);
int rt_progressive_guide_chain_info(void* frame, uint32_t* max_links_out, double* max_fuzz_out);

/* What a material handle stands for (host only, no GPU): kind_texture_out[0] = the kind (0 Lambertian, 1 Metal, 2 Dielectric, 3 DiffuseLight,
 * 4 Isotropic, 5 PBR), [1] = its texture handle (-1 for Metal and Dielectric); albedo_out = Metal's albedo (0 otherwise).  A bad handle is an error. */
int rt_material_info(rt_scene*, int material, int32_t kind_texture_out[2], double albedo_out[3]);

/* ---- radiance queries: the reference's `ray_color(r, background, world, lights, depth)` (src/main.rs:41-120) as a function of its own — the
 *      radiance along rays the caller chooses, samples_per_ray samples of each: another projection than camera.rs's (360-degree panorama,
 *      orthographic, fisheye, a measured lens), a light or irradiance probe at a point, a baked light map over a surface, "how bright is it
 *      along THIS ray".  The bounce loop is the frames' own device code (csrc/rt_radiance.hip), for every kind of scene, the principled
 *      material included.  f64 and the reference's traversal order only; one device, the current one.
 * A ray is the 7 doubles of rt_query_hits: origin[3], direction[3], time.  Non-finite and zero components are legal; the direction is not
 * normalised (the reference does not normalise it either).
 * Sample s of ray k is ray_color(ray_k, background, world, lights, max_depth) drawing from the stream of rt_rng_path(seed, k, first_sample + s)
 * from its first draw on: the frames' keying with the ray's index in the pixel's place, and no camera draws.  Hence n <= 2^31 - 1 and
 * first_sample + samples_per_ray <= 2^32 - 1 (the offset is folded into the seed, as rt_render_device_pass does it).
 * rgb_sum_out = n x 3: per ray the SUM over its samples, as rt_render returns per pixel (divide by samples_per_ray, or hand to
 * rt_write_ppm / rt_format_color).  The sums are built with f64 atomic adds: a ray's samples may be spread over many waves, so a sum's
 * rounding depends on the order the partial sums arrive in — |sum - exact| <= 2 * gamma_N * sum |x_i|, gamma_N = N u / (1 - N u), u = 2^-53,
 * N = the samples added (the bound rt_progressive_read_sum states); the samples themselves are the same words in every run.
 * samples_out: NULL, or n x samples_per_ray x 3, every sample, ray-major (the layout of rt_render_samples).  nonfinite_out: NULL, or the number
 * of samples with a non-finite component (the B8 count of rt_last_stats, for this call).
 * flags: RT_STOP_ON_ZERO and RT_ISOTROPIC_SCATTER as for the frames; every other bit, RT_F32 included, is an error.
 * The host form is synchronous: the device form with (first_sample, accumulate) = (0, 0).  The _device form takes DEVICE pointers (d_rays
 * 16-byte aligned, the others 8-byte), only enqueues on hip_stream (a hipStream_t, may be NULL) and never waits; accumulate = 0: d_rgb_sum is
 * zeroed on the stream first; accumulate != 0: the pass is added to what d_rgb_sum holds.  d_samples_out (may be NULL) receives THIS pass's
 * n x samples_per_ray x 3 samples.  d_nonfinite_out (may be NULL) is one u64 that is only ever added to: the caller zeroes it.  There is no
 * global work counter, so launches on different streams may overlap.  A scene not yet prepared is flattened and uploaded first, as
 * rt_render_device does it.
 * Errors (non-zero, a message for rt_last_error, nothing launched): null arguments, samples_per_ray = 0, either limit above exceeded, a flag
 * other than the two, d_rgb_sum_bytes < 24 n, a misaligned pointer, no HIP device (there is no CPU path).  n = 0 returns 0 and touches nothing.
 * rt_last_query_ms reports this kernel too; what rt_last_kernel_ms, rt_last_stats and friends report about the frames is left alone. */
int rt_query_radiance(rt_scene*, uint32_t n, const double* rays, const double background[3],
                      uint32_t samples_per_ray, uint32_t max_depth, uint64_t seed, uint32_t flags,
                      double* rgb_sum_out, double* samples_out, uint64_t* nonfinite_out);
int rt_query_radiance_device(rt_scene*, uint32_t n, const void* d_rays, const double background[3],
                             uint32_t samples_per_ray, uint32_t max_depth, uint64_t seed, uint32_t flags,
                             uint32_t first_sample, int accumulate,
                             void* d_rgb_sum, size_t d_rgb_sum_bytes, void* d_samples_out, void* d_nonfinite_out,
                             void* hip_stream);

/* ---- denoising: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a frame of per-pixel sums, guided by the hit records
 *      of rt_query_camera (sample 0's camera ray: normal, position, hit distance, hit / material) — what the 16 .. 64 samples of a preview
 *      need.  A 5x5 B3-spline kernel, dilated by 2^i in iteration i, with stops on colour, normal, plane distance (relative to the centre's
 *      hit distance: sigma_p has no scene scale) and a hit / material key.  The filter is an exact f64 specification (csrc/rt_denoise.h: only
 *      + - * / and comparisons, a fixed order) that the HIP kernels (csrc/rt_denoise.hip) and the host twin below satisfy bit for bit.
 * rgb_sum: W*H*3 doubles in output order, as rt_render returns them; samples >= 1: how many samples they hold; hits: W*H records of 16 doubles,
 * as rt_query_camera returns them or — here and for every `hits` / `d_hits` parameter of the denoise family below — the averaged records of
 * rt_query_camera_guide (the filters read hit, t, position, normal and material only); iterations: 1 .. 8; sigma = {sigma_c, sigma_n, sigma_p}: each > 0, +inf switches that stop off (0, negative
 * and NaN are errors); flags: RT_DENOISE_SAME_MATERIAL or 0.  rgb_sum_out: W*H*3 doubles, the filtered frame in SUM units again (mean times
 * samples), so that rt_write_ppm, rt_format_color and the resolve apply to it unchanged; it may be rgb_sum itself.  W, H >= 1, W*H <= 2^31 - 1.
 * Non-finite input pixels are left out as neighbours and, as centres, take their neighbours' values: the filter repairs NaN pixels.
 * Guides beyond sample 0's camera ray — averaged over the lens, the shutter and the pixel — are rt_query_camera_guide's records; not done: a
 * coverage or depth-spread stop that would read their word [15].  Textured surfaces: this filter sees a texture as
 * colour and only sigma_c protects it — use the albedo-demodulated forms below (rt_denoise_albedo*).  Errors (non-zero, a message for rt_last_error, nothing written): null arguments and everything outside the ranges above. */
enum { RT_DENOISE_SAME_MATERIAL = 1 /* pixels are neighbours only if their hits have the same material handle (default: only hit beside hit, miss beside miss) */ };
/* The host twin: the specification as plain C++; needs no device. */
int rt_denoise_host(const double* rgb_sum, uint64_t samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations,
                    const double sigma[3], uint32_t flags, double* rgb_sum_out);
/* The same call, the same words, computed on the current HIP device (host pointers; synchronous).  Fails without a device, as rt_render does. */
int rt_denoise(const double* rgb_sum, uint64_t samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations,
               const double sigma[3], uint32_t flags, double* rgb_sum_out);
/* Bytes of device memory rt_denoise_device needs as its workspace for a W x H frame: 128 per pixel (two padded colour frames, one packed guide). */
size_t rt_denoise_workspace_bytes(uint32_t W, uint32_t H);
/* The same filter for DEVICE pointers on the current device: d_rgb_sum and d_rgb_sum_out 8-byte aligned (they may be the same buffer), d_hits and
 * d_workspace 16-byte aligned, sigma a HOST pointer.  Only enqueues on hip_stream (a hipStream_t, may be NULL): it never waits and never
 * allocates.  A workspace smaller than rt_denoise_workspace_bytes(W, H) is an error before anything is launched. */
int rt_denoise_device(const void* d_rgb_sum, uint64_t samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                      const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, void* hip_stream);
/* A progressive frame's sums as they are now, filtered and resolved on the device: rgb8_out receives W*H*3 bytes, format_color of the
 * filtered sums — byte for byte rt_format_color of rt_denoise_host(rt_progressive_read_sum, rt_progressive_samples, the frame's guide):
 * rt_query_camera(sample 0, the frame's seed), or the averaged record rt_progressive_set_guide_samples asked for.  The frame builds the packed
 * guide itself at the first call (rt_query_camera_device or rt_query_camera_guide_device on its device; what rt_last_query_ms
 * reports for the scene is that launch then) and keeps it until rt_progressive_reset; another `flags` than the guide was keyed for rebuilds it.
 * Everything happens in buffers of the frame's own, allocated at the first call (155 bytes per pixel) and freed by rt_progressive_destroy:
 * the accumulated sums, the images of rt_progressive_resolve_rgb8* and its changed-pixel count are untouched, and the two kinds of resolve may
 * be interleaved freely.  Waits for every pass enqueued so far.  Errors: the arguments of rt_denoise; a frame of 0 samples; a scene that is
 * gone, or has changed, while the frame holds no guide (with a guide the frame still resolves after its scene is destroyed). */
int rt_progressive_resolve_denoised_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out);

/* ---- albedo-demodulated denoising: the filter above applied to rgb_sum / albedo and multiplied back, so that a texture — checker, image,
 *      Perlin noise — is not "colour" the filter has to preserve: it filters irradiance.  An exact specification again (csrc/rt_albedo.h:
 *      only + - * / and comparisons, a fixed order).  Per pixel and channel, eps = 2^-8 (one output code value of format_color per unit of
 *      irradiance):  a = albedo_sum / albedo_samples;  m = a finite ? a : 1;  d = m >= eps ? m : eps;  x = rgb_sum / d;
 *      y = rt_denoise(x, ...);  out = y * m.  A black channel stays black whatever its neighbours hold; a non-finite albedo demodulates nothing.
 * albedo_sum: W*H*3 doubles, as rt_query_camera_albedo returns them; albedo_samples >= 1: how many samples they hold.  The other arguments,
 * the errors (plus albedo_samples = 0 and a null albedo) and the three forms are those of rt_denoise_host / rt_denoise / rt_denoise_device;
 * RT_DENOISE_SAME_MATERIAL is the only flag.  The device form wraps two element-wise kernels (csrc/rt_albedo.hip) around the unchanged
 * filter and needs rt_denoise_albedo_workspace_bytes(W, H) = 152 bytes per pixel; d_albedo_sum is 8-byte aligned and is only read. */
int rt_denoise_albedo_host(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                           uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out);
int rt_denoise_albedo(const double* rgb_sum, uint64_t samples, const double* albedo_sum, uint64_t albedo_samples, const double* hits,
                      uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out);
size_t rt_denoise_albedo_workspace_bytes(uint32_t W, uint32_t H);
int rt_denoise_albedo_device(const void* d_rgb_sum, uint64_t samples, const void* d_albedo_sum, uint64_t albedo_samples, const void* d_hits,
                             uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3], uint32_t flags, void* d_rgb_sum_out,
                             void* d_workspace, size_t workspace_bytes, void* hip_stream);
/* rt_progressive_resolve_denoised_rgb8 with demodulation: byte for byte rt_format_color of rt_denoise_albedo_host(rt_progressive_read_sum,
 * rt_progressive_samples, rt_query_camera_albedo(first_sample 0, albedo_samples, the frame's seed), albedo_samples, the frame's guide
 * (rt_progressive_set_guide_samples)).  The frame builds its albedo sums itself (rt_query_camera_albedo_device on its device; rt_last_query_ms reports that
 * launch then) and keeps them beside the guide until rt_progressive_reset or until another albedo_samples is asked for (48 more bytes per
 * pixel).  The accumulated sums and what the other two resolves own are untouched; the three may be interleaved freely.
 * rt_progressive_albedo_info: the albedo_samples the frame holds sums for (0: none) and how many times it has built them. */
int rt_progressive_resolve_denoised_albedo_rgb8(void* frame, uint32_t albedo_samples, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out);
int rt_progressive_albedo_info(void* frame, uint32_t* albedo_samples_out, uint64_t* builds_out);

/* ---- variance-guided denoising: the filter of rt_denoise with a colour stop measured in standard deviations of the two pixels it compares
 *      (the variance-guided a-trous filter of SVGF, Schied et al. 2017), so that no sigma_c has to be tuned per scene or per sample count.
 *      var: W*H*3 doubles, the variance of the mean of every pixel and channel (rt_moments_variance*); the filter uses their sum v per pixel
 *      (a NaN, an infinity, a negative or a zero sum counts as 0), smooths it once over 3 x 3 pixels of the same key, and in every iteration
 *      weights a tap by  wc = max(1 - |c_q - c_p|^2 / (sigma_v^2 (v_p + v_q + 2^-16)), 0)^2  beside the unchanged normal, plane and key
 *      stops, and filters v along with the colour (sum of w^2 v over the square of the sum of w): the stop tightens as the picture gets
 *      cleaner, and there is no 4^i schedule.  csrc/rt_denoise_var.h is the exact specification — + - * / and comparisons in a fixed order —
 *      which the HIP kernels (csrc/rt_denoise_var.hip) and the host twin satisfy bit for bit.
 * sigma = {sigma_v, sigma_n, sigma_p}: sigma_v is dimensionless (standard deviations); +inf switches a stop off, and with sigma_v = +inf the
 * filtered colours are the words of rt_denoise with sigma_c = +inf.  var_out: W*H doubles or NULL, the filtered v — the variance of the
 * filtered mean, were the taps independent.  The other arguments, the errors (plus a null var) and the three forms are those of
 * rt_denoise_host / rt_denoise / rt_denoise_device; the workspace is rt_denoise_variance_workspace_bytes(W, H) = 128 bytes per pixel;
 * d_var and d_var_out are 8-byte aligned, d_var is only read.
 * Not done: the combination with albedo demodulation (per-channel V / albedo^2 — which is why var is per channel; now rt_denoise_frame
 * below), temporal accumulation (now rt_reproject and, for the variance itself, rt_reproject_variance below), variance gathered inside the
 * path-tracing kernels, rt_render_multi. */
int rt_denoise_variance_host(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H,
                             uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out);
int rt_denoise_variance(const double* rgb_sum, uint64_t samples, const double* var, const double* hits, uint32_t W, uint32_t H,
                        uint32_t iterations, const double sigma[3], uint32_t flags, double* rgb_sum_out, double* var_out);
size_t rt_denoise_variance_workspace_bytes(uint32_t W, uint32_t H);
int rt_denoise_variance_device(const void* d_rgb_sum, uint64_t samples, const void* d_var, const void* d_hits, uint32_t W, uint32_t H,
                               uint32_t iterations, const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_var_out,
                               void* d_workspace, size_t workspace_bytes, void* hip_stream);
/* rt_progressive_resolve_denoised_rgb8 with the frame's own variance: byte for byte rt_format_color of rt_denoise_variance_host(
 * rt_progressive_read_sum, rt_progressive_samples, rt_moments_variance_host(the sums, rt_progressive_read_moments, samples, passes),
 * the frame's guide (rt_progressive_set_guide_samples)).  The variance, the filter and the resolve run on the device; the guide is the one the frame
 * packs once for all its denoised resolves.  The accumulated sums, the second moments, the pass count and what the other resolves own are
 * untouched.  Errors: those of rt_progressive_resolve_denoised_rgb8, and a frame without moments, with invalid moments or with fewer than
 * two passes. */
int rt_progressive_resolve_denoised_variance_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out);

/* ---- denoising a frame as it is: one sample count for the frame or a count per pixel (an adaptive frame), with or without a variance
 *      frame, with or without albedo sums — the three filters above composed, and the only denoised form an adaptive frame with differing
 *      counts has.  csrc/rt_denoise_frame.h is the exact specification: per pixel and channel, N = counts ? counts[p] : samples; m and d as in
 *      rt_denoise_albedo (m = d = 1 without albedo_sum);  c = (rgb_sum / d) / N;  Vd = (var / d) / d;  y = rt_denoise(c, samples = 1, ...) or,
 *      with var, rt_denoise_variance(c, samples = 1, Vd, ...);  out = ((N > 0 ? y * N : +0.0)) * m.  The filters in the middle are the ones
 *      above, unchanged; with equal counts every word is the one rt_denoise*, rt_denoise_albedo* and rt_denoise_variance* give.  A pixel with
 *      count 0 is left out as a neighbour, as a non-finite pixel is, and comes out 0.
 *
 * The variance frame of a frame with counts, (E) of that header: per pixel and channel, V = passes[p] >= 2 ? the V of rt_moments_variance
 * with counts[p] samples and passes[p] passes : +inf (which the variance-guided filter counts as "no information").  counts, passes: W*H
 * uint32; var_out: W*H*3 doubles.  The device form takes device pointers (doubles 8-byte aligned, counts 4-byte), never waits, never
 * allocates; var_out may be neither input. */
int rt_adaptive_variance_host(const double* rgb_sum, const double* sq_sum, const uint32_t* counts, const uint32_t* passes, uint32_t W, uint32_t H,
                              double* var_out);
int rt_adaptive_variance_device(const void* d_rgb_sum, const void* d_sq_sum, const void* d_counts, const void* d_passes, uint32_t W, uint32_t H,
                                void* d_var_out, void* hip_stream);
/* counts: W*H uint32 or NULL (then `samples` is the frame's count; with counts `samples` is ignored); var: W*H*3 doubles or NULL (NULL: the
 * colour stop of rt_denoise, sigma[0] = sigma_c; else the variance stop of rt_denoise_variance, sigma[0] = sigma_v); albedo_sum: W*H*3 doubles
 * or NULL (then albedo_samples is ignored); var_out: W*H doubles or NULL, the filtered v of rt_denoise_variance — of the DEMODULATED frame when
 * albedo_sum is given — and an error without var.  Everything else, the errors and the three forms are those of rt_denoise_host / rt_denoise /
 * rt_denoise_device.  The device form wraps two element-wise kernels (csrc/rt_denoise_frame.hip) around the unchanged filter and needs
 * rt_denoise_frame_workspace_bytes(W, H) (the filter's 128 bytes per pixel and two frames of 24); d_counts is 4-byte aligned; d_rgb_sum_out
 * may be d_rgb_sum. */
int rt_denoise_frame_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum,
                          uint64_t albedo_samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                          uint32_t flags, double* rgb_sum_out, double* var_out);
int rt_denoise_frame(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* var, const double* albedo_sum,
                     uint64_t albedo_samples, const double* hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                     uint32_t flags, double* rgb_sum_out, double* var_out);
size_t rt_denoise_frame_workspace_bytes(uint32_t W, uint32_t H);
int rt_denoise_frame_device(const void* d_rgb_sum, const void* d_counts, uint64_t samples, const void* d_var, const void* d_albedo_sum,
                            uint64_t albedo_samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations, const double sigma[3],
                            uint32_t flags, void* d_rgb_sum_out, void* d_var_out, void* d_workspace, size_t workspace_bytes, void* hip_stream);
/* rt_progressive_variance for any frame with moments: (E) with the frame's own counts on an adaptive frame (uniform or not; a pixel with
 * fewer than two passes holds +inf), rt_progressive_variance itself on any other. */
int rt_progressive_variance_counts(void* frame, double* var_out);
/* The denoised resolve of any progressive frame, adaptive frames with differing counts included: byte for byte the resolve of
 * rt_denoise_frame_host(rt_progressive_read_sum, the frame's counts or its sample count, stop = RT_DENOISE_STOP_VARIANCE ?
 * rt_progressive_variance_counts : NULL, albedo_samples ? the albedo sums of rt_progressive_resolve_denoised_albedo_rgb8 : NULL,
 * the frame's guide (rt_progressive_set_guide_samples)) — rt_format_color with the frame's sample count, or rt_adaptive_resolve_rgb8_host with its
 * counts on an adaptive frame.  On a frame without counts the three modes that have a predecessor give that predecessor's bytes.  The
 * sums, moments, counts, what the other resolves own and rt_progressive_albedo_info's behaviour are untouched.  Errors: those of
 * rt_progressive_resolve_denoised_rgb8; an unknown stop; the variance stop on a frame without (valid) moments, or — a frame without
 * counts — with fewer than two passes. */
enum { RT_DENOISE_STOP_COLOUR = 0, RT_DENOISE_STOP_VARIANCE = 1 };
int rt_progressive_resolve_denoised_frame_rgb8(void* frame, uint32_t stop, uint32_t albedo_samples, uint32_t iterations, const double sigma[3],
                                               uint32_t flags, uint8_t* rgb8_out);

/* ---- temporal accumulation: a frame's history reprojected into a new view of the same scene (the half of SVGF, Schied et al. 2017, that the
 *      variance-guided filter leaves out), so that a camera move does not throw every sample away.  For every pixel of the new view whose
 *      first-hit record (cur_hits) is a hit with an object (word [12] >= 0): its surface point is projected through the previous camera's
 *      lens centre onto the previous view's pixel grid; the four pixels around that place are the taps of a bilinear footprint; a tap counts
 *      when the previous record (prev_hits) is a hit of the same object whose normal agrees (n.m > 0 and cos^2 >= normal_min^2), whose point
 *      lies in the centre's plane within sigma_p times the distance from the previous camera, whose count is not 0 and whose sums are
 *      finite.  The history is the weighted mean of the taps' MEANS, in sum units with a count of its own:
 *          hist_counts = floor(min(sum of w * count over the taps, max_history)),   hist_sum = mean * hist_counts
 *      — the weights are not renormalised in the count, so a footprint that is only partly valid is worth less, and max_history caps what
 *      the past is worth: n new samples weigh n / (n + hist_counts).  A pixel without history holds +0.0 sums and count 0.
 *      csrc/rt_reproject.h is the exact specification — + - * /, floor and comparisons in a fixed order — which the HIP kernel
 *      (csrc/rt_reproject.hip), the host twin and a NumPy restatement (tests/reproject_cases.py) satisfy bit for bit.
 * prev_sum: W*H*3 doubles, output order; prev_counts: W*H uint32 or NULL (then prev_samples >= 1 is every pixel's count; with counts it is
 * ignored); prev_hits, cur_hits: W*H records of 16 doubles as rt_query_camera or rt_query_camera_guide write them for the previous and the
 * new view; prev_cam: the previous view's camera (the new view's is not needed: its records hold world-space points); max_history: 0 .. 2^31 - 1
 * (0: an empty history); sigma = {normal_min in [0, 1], sigma_p > 0}, +inf as sigma_p switches that stop off; flags: 0.
 * hist_sum_out: W*H*3 doubles; hist_counts_out: W*H uint32; neither may overlap an input.
 * Three forms as for rt_denoise: _host is plain C++ (no GPU), rt_reproject copies to the current device and runs the kernel there,
 * rt_reproject_device takes device pointers (records 16-byte aligned, sums 8-byte, counts 4-byte), only enqueues on hip_stream, never waits
 * and never allocates.  Errors (non-zero, rt_last_error, nothing written or launched): a null argument, W or H < 2, W*H > 2^31 - 1,
 * max_history > 2^31 - 1, normal_min outside [0, 1] or NaN, sigma_p <= 0 or NaN, flags != 0, prev_samples = 0 without counts.
 * Not done: history for pixels that miss (the background), a wider search when all four taps fail, objects that move between the views,
 * reflections and refractions (a mirror's image is reprojected as if painted on it), f32.  (A variance frame travels with
 * rt_reproject_variance below.) */
int rt_reproject_host(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_hits, const rt_camera* prev_cam,
                      const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                      double* hist_sum_out, uint32_t* hist_counts_out);
int rt_reproject(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_hits, const rt_camera* prev_cam,
                 const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                 double* hist_sum_out, uint32_t* hist_counts_out);
int rt_reproject_device(const void* d_prev_sum, const void* d_prev_counts, uint64_t prev_samples, const void* d_prev_hits, const rt_camera* prev_cam,
                        const void* d_cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2], uint32_t flags,
                        void* d_hist_sum_out, void* d_hist_counts_out, void* hip_stream);
/* The blend of a frame with a history, element-wise: sum_out = rgb_sum + hist_sum, counts_out = min(N + hist_counts, 2^32 - 1) with
 * N = counts ? counts[p] : samples (samples = 0 is allowed: a view that has no samples of its own yet).  The result is a frame with counts in
 * the adaptive frames' layout: rt_adaptive_resolve_rgb8_* and rt_denoise_frame*(counts = ...) take it unchanged.  counts: W*H uint32 or
 * NULL; sum_out may be rgb_sum and counts_out may be counts; the history may overlap no output.  The device form takes device pointers (sums
 * 8-byte aligned, counts 4-byte), only enqueues, never waits, never allocates.  Errors: a null argument, W or H < 2, W*H > 2^31 - 1. */
int rt_temporal_blend_host(const double* rgb_sum, const uint32_t* counts, uint64_t samples, const double* hist_sum, const uint32_t* hist_counts,
                           uint32_t W, uint32_t H, double* sum_out, uint32_t* counts_out);
int rt_temporal_blend_device(const void* d_rgb_sum, const void* d_counts, uint64_t samples, const void* d_hist_sum, const void* d_hist_counts,
                             uint32_t W, uint32_t H, void* d_sum_out, void* d_counts_out, void* hip_stream);
/* Temporal variance: rt_reproject with the variance of the previous frame's per-pixel mean carried along, so that the variance-guided filter
 * (rt_denoise_variance, rt_denoise_frame(var = ...)) has its stop in the instant after a camera move.  A variance is KNOWN when it is finite
 * and >= 0; NaN, +-inf and negative values are unknown, and unknown is written as +inf (what rt_adaptive_variance writes for a pixel with
 * fewer than two passes, and what the filter reads as "no information").  prev_var: W*H*3 doubles — rt_progressive_variance,
 * rt_adaptive_variance, or rt_temporal_blend_variance of an earlier view.  hist_sum_out and hist_counts_out are rt_reproject's words.  A tap
 * rt_reproject accepts whose three variances are known contributes its PER-SAMPLE variance prev_var * count (a property of the surface
 * point), and hist_var_out is the weighted mean of those divided by hist_counts: the history is hist_counts samples of that per-sample
 * variance, so max_history, which caps the count, raises the variance the history claims.  The averaging over the bilinear footprint is not
 * credited: neighbouring pixels share taps, and the filter's stop assumes independent pixels.  A pixel with history none of whose taps has a
 * known variance gets +inf; a pixel without history +0.0, like its sums.  csrc/rt_reproject_var.h is the exact specification, which the
 * fused HIP kernel (csrc/rt_reproject_var.hip: sums, counts and variances in one launch), the host twin and a NumPy restatement
 * (tests/reproject_var_cases.py) satisfy bit for bit.
 * The three forms, the alignment (variances 8-byte) and the errors are rt_reproject's, plus a null prev_var or hist_var_out; no output may
 * overlap an input.  Not done: what rt_reproject does not do; adaptive frames in rt_progressive_set_view; history in checkpoints. */
int rt_reproject_variance_host(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_var, const double* prev_hits,
                               const rt_camera* prev_cam, const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                               uint32_t flags, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out);
int rt_reproject_variance(const double* prev_sum, const uint32_t* prev_counts, uint64_t prev_samples, const double* prev_var, const double* prev_hits,
                          const rt_camera* prev_cam, const double* cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                          uint32_t flags, double* hist_sum_out, uint32_t* hist_counts_out, double* hist_var_out);
int rt_reproject_variance_device(const void* d_prev_sum, const void* d_prev_counts, uint64_t prev_samples, const void* d_prev_var, const void* d_prev_hits,
                                 const rt_camera* prev_cam, const void* d_cur_hits, uint32_t W, uint32_t H, uint32_t max_history, const double sigma[2],
                                 uint32_t flags, void* d_hist_sum_out, void* d_hist_counts_out, void* d_hist_var_out, void* hip_stream);
/* The variance of the mean of rt_temporal_blend's frame, per pixel and channel, from the frame's variance V (var: n_px*3 doubles, or NULL:
 * unknown everywhere — a frame with fewer than two passes) with N = counts ? counts[p] : samples, and the history's Vh (hist_var) with
 * h = hist_counts[p]:  h = 0: V when N > 0 and V is known, else +inf;  N = 0: Vh when known, else +inf;  both known:
 * (N^2 V + h^2 Vh) / (N + h)^2;  only Vh known: Vh h / (N + h) — the new samples borrow the history's per-sample variance Vh h, which is what
 * gives the filter a stop one pass after a move;  only V known: V N / (N + h);  neither: +inf.  var_out (n_px*3 doubles) may be var; it is
 * what rt_denoise_frame*(counts = the blend's counts, var = ...) takes.  The device form takes device pointers (variances 8-byte aligned,
 * counts 4-byte), only enqueues, never waits, never allocates.  Errors: a null hist_var, hist_counts or var_out; n_px > 2^31 - 1. */
int rt_temporal_blend_variance_host(const double* var, const uint32_t* counts, uint64_t samples, const double* hist_var, const uint32_t* hist_counts,
                                    uint64_t n_px, double* var_out);
int rt_temporal_blend_variance_device(const void* d_var, const void* d_counts, uint64_t samples, const void* d_hist_var, const void* d_hist_counts,
                                      uint64_t n_px, void* d_var_out, void* hip_stream);
/* A progressive frame moved to another view WITH its history (rt_progressive_reset moves nothing and drops the history).  Waits for the
 * passes enqueued so far.  The previous frame is the blend of the frame's sums (rt_progressive_samples samples) with the history it holds, so
 * history chains from view to view; prev_hits and cur_hits are the frame's guide records — rt_query_camera(sample 0), or
 * rt_query_camera_guide(0, guide_samples) after rt_progressive_set_guide_samples — of the old view under the old seed and of the new view
 * under the new seed; the history becomes rt_reproject of that frame (H_sum and H_cnt, 28 more bytes per pixel, allocated at first use).
 * The frame then holds 0 samples of the new camera and seed, exactly as rt_progressive_reset leaves it (moments, guide, albedo sums, the
 * first-resolve state), and keeps the history.  Give the new view a NEW SEED: a sample's random stream is keyed by pixel and sample index,
 * so the same seed under a nearby camera gives the new samples nearly the noise the history already carries, and the two do not average
 * out.  max_history = 0 is a plain change of view.  Every call that existed before ignores the history.
 * On a frame WITH MOMENTS (rt_progressive_enable_moments) the history carries its variance too: the previous frame's variance is
 * rt_temporal_blend_variance of the frame's own (rt_progressive_variance when the moments are valid and the frame holds two passes, else
 * NULL) with the history variance it holds, and rt_reproject_variance fills H_sum, H_cnt and H_var in one launch (H_var: 24 more bytes per
 * pixel, allocated at first use; +inf where a history taken before the moments were enabled has none).  A frame without moments takes the
 * path above unchanged.
 * Errors: those of rt_reproject; an adaptive frame (compose rt_reproject_device and rt_temporal_blend_device instead); a scene that has been
 * destroyed or changed.
 * rt_progressive_read_history: H_sum (W*H*3 doubles) and H_cnt (W*H uint32); all zero without a history.
 * rt_progressive_history_info: out[0] the views taken by rt_progressive_set_view over the frame's life, out[1] the pixels with H_cnt > 0.
 * rt_progressive_read_history_variance: H_var (W*H*3 doubles); all +0.0 without a history; an error on a frame without moments. */
int rt_progressive_set_view(void* frame, const rt_camera* cam, uint64_t seed, uint32_t max_history, const double sigma[2]);
int rt_progressive_read_history(void* frame, double* hist_sum_out, uint32_t* hist_counts_out);
int rt_progressive_history_info(void* frame, uint64_t out[2]);
int rt_progressive_read_history_variance(void* frame, double* hist_var_out);
/* The resolve of the frame blended with its history.  iterations = 0: byte for byte rt_adaptive_resolve_rgb8_host of rt_temporal_blend_host(
 * rt_progressive_read_sum, rt_progressive_samples, rt_progressive_read_history); sigma may be NULL.  iterations 1 .. 8: that resolve of
 * rt_denoise_frame_host(the blend's sums, counts = the blend's counts, no variance, no albedo, the frame's guide, iterations, sigma = {sigma_c,
 * sigma_n, sigma_p}, flags).  Allowed with 0 samples when a pixel has history — the preview in the instant after a camera move; an error
 * with neither samples nor history, and on an adaptive frame.  The sums, the history and what the other resolves own are untouched. */
int rt_progressive_resolve_temporal_rgb8(void* frame, uint32_t iterations, const double sigma[3], uint32_t flags, uint8_t* rgb8_out);
/* ... with the VARIANCE stop: byte for byte rt_adaptive_resolve_rgb8_host of rt_denoise_frame_host(the blend's sums, counts = the blend's
 * counts, var = rt_temporal_blend_variance_host(the frame's variance or NULL as rt_progressive_set_view takes it, rt_progressive_samples,
 * rt_progressive_read_history_variance, H_cnt), the frame's albedo sums as rt_progressive_resolve_denoised_frame_rgb8 builds them when
 * albedo_samples > 0 (else none), the frame's guide, iterations 1 .. 8, sigma = {sigma_v, sigma_n, sigma_p}, flags).  Allowed with 0 samples
 * when a pixel has history, and with one pass: the history's variance is the stop.  Errors: a frame without moments, an adaptive frame,
 * neither samples nor history, iterations = 0 or > 8, those of rt_denoise_variance.  The sums, the moments, the history and what the other
 * resolves own are untouched.  Not done: a filtered variance out. */
int rt_progressive_resolve_temporal_variance_rgb8(void* frame, uint32_t albedo_samples, uint32_t iterations, const double sigma[3], uint32_t flags,
                                                  uint8_t* rgb8_out);

/* The whole frame on several GPUs of this node from ONE call: what a host that owns the node's GPUs itself (the reference's `main`,
 * src/main.rs:767-835) calls instead of rt_render.  device_mask: bit d selects HIP device d (0 = every visible device).  The scene
 * is replicated on each selected device; tiles of tile_px output-order pixels (0 = the default, 67) are dealt round-robin, each
 * device renders its share with one persistent launch, ONE ncclGather (RCCL over xGMI; communicators from ncclCommInitAll, cached
 * with the scene; librccl is loaded on first use) brings the packed tiles to the first selected device, which un-permutes them on the
 * device; rgb_sum_out receives W*H*3 doubles in output order, as from rt_render.  Synchronous.  A failure on any device leaves
 * nothing in flight, keeps no temporary and restores the caller's current HIP device.
 * rt_last_multi_ms (waits for the frame): [0] slowest device's kernel, [1] the gather as the first device's stream sees it
 * (from the end of its own kernel: the collective including the wait for the slowest other device), [2] un-permute, [3] host clock
 * from the call's entry to the end of the wait (rt_render_multi: of the whole call, transfer included), in ms. */
int rt_render_multi(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                    uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
                    uint32_t device_mask, uint32_t tile_px, double* rgb_sum_out);
/* The same frame left in device memory: returns once every device's work is enqueued (kernels, gather, un-permute); *d_frame_out (may
 * be NULL) receives a DEVICE pointer on the first selected device to W*H*3 doubles in output order, owned by the scene.  Consecutive
 * frames alternate between TWO such buffers, so a frame's pointer stays valid (and its pixels untouched) until the next-but-one
 * rt_render_multi* call: a caller can read frame i while frame i + 1 is rendered.  Calls may follow each other without waiting: each device's work is ordered by its own
 * stream and the host runs at most one frame ahead, so the devices go from frame to frame without a launch gap (a frame of another
 * shape or device set first waits for the one in flight); timings are kept for the most recent frame.
 * rt_multi_sync waits for the frames in flight; rt_multi_copy_frame waits and copies the first n_doubles (<= W*H*3) doubles of the most
 * recent frame to host memory.
 * rt_render_multi = rt_render_multi_device + rt_multi_copy_frame. */
int rt_render_multi_device(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                           uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
                           uint32_t device_mask, uint32_t tile_px, void** d_frame_out);
int rt_multi_sync(rt_scene*);
int rt_multi_copy_frame(rt_scene*, double* rgb_sum_out, size_t n_doubles);
int rt_last_multi_ms(rt_scene*, double out4[4]);
/* The ranks of the most recent rt_render_multi* frame (waits for it): *n_ranks_out = how many launches made the frame; for the first
 * max_ranks of them device_out[r] = the HIP device rank r ran on, kernel_ms_out[r] = its path-tracing kernel's duration (HIP events
 * on its stream; -1 if no longer known); *collective_ranks_out = the size RCCL reports for the communicator the frame's gather ran
 * on (ncclCommCount), 0 when no collective ran (one device without RT_MULTI_COLLECTIVE, or the virtual-rank test hook).  What a
 * multi-GPU caller checks before it trusts a frame: N distinct devices, N ranks in the collective, no rank with a ~0 ms kernel. */
int rt_last_multi_ranks(rt_scene*, uint32_t max_ranks, uint32_t* n_ranks_out, int* device_out, double* kernel_ms_out,
                        uint32_t* collective_ranks_out);
/* How BVH objects are built when the scene is flattened (at the first render / rt_scene_prepare after a change).
 * RT_BVH_MEDIAN (default) is BVH::new, src/bvh.rs:18-73: widest axis, object median.  RT_BVH_SAH is an opt-in fast mode
 * (binned surface-area heuristic, one object per leaf as in the reference): same closest hits; the order in which
 * exactly-equal-t hits are met, and last-ulp box culls, may differ — like RT_NEAR_FIRST_BVH. */
enum rt_bvh_builder { RT_BVH_MEDIAN = 0, RT_BVH_SAH = 1 };
/* Tuning knob of the persistent-traversal loop (scheduling only, never results): a traversal pass starts once `start_at` lanes of a
 * wavefront are inside a BVH and runs until fewer than `stop_below` are still walking; primitives are tested once `leaf_share64`/64
 * of the walking lanes hold a pending leaf.  Defaults 56, 16, 32 (measured best on the teapot room; the optimum is flat). */
int rt_scene_set_traversal_schedule(rt_scene*, uint32_t start_at, uint32_t stop_below, uint32_t leaf_share64);
int rt_scene_set_bvh_builder(rt_scene*, int mode);
/* Optional: do now what the first render of this scene would do once inside its call (flatten, upload for the precision in
 * `flags`, load the kernel's code object).  Launches nothing. */
int rt_scene_prepare(rt_scene*, uint32_t flags);
/* Mesh scenes (triangle-mesh BVHs beside other top-level objects) run a persistent-traversal or a lock-step loop — bit-identical samples;
 * which is faster depends on what the rays of a VIEW do inside the trees, not on the trees' size.  rt_scene_calibrate measures it:
 * the same view at <= 1024 x 1024 x 16 samples, twice in each shape (four launches, ~30 ms), SYNCHRONOUSLY on the calling thread's
 * current device, and keeps the faster shape for that view (camera, W, H, precision; another view falls back to the size rule until it
 * is calibrated itself; a change to the scene forgets everything).  A no-op for every other kind of scene and for a view already
 * measured.  rt_render, rt_render_samples and rt_render_multi do this themselves at a scene's first frame of >= 1e8 samples;
 * rt_render_device and rt_render_multi_device — asynchronous — never do.
 * The same call (and the same three synchronous entry points, for every new view) tunes the filter tree of a world that is ONE bare BVH —
 * the random-spheres scene — for the view: which inner nodes the kernels' box steps skip over is decided by the nodes' estimated pass
 * rates (a few thousand rays through the tree on the host, < 1 ms) instead of by box areas; random spheres +6 %, samples unchanged
 * (rt_flatten.cpp tune_filter_tree).
 * rt_scene_set_loop_shape: 1 persistent traversal, 0 lock-step, for every view until the scene changes, -1 forgets (how the ranks of a
 * one-process-per-GPU job all run the shape rank 0 measured).
 * rt_last_loop_info: what the most recent launch ran — out4[0] loop shape (0: a list scene's kernel, 1: lock-step BVH, 2: persistent
 * traversal), [1] the FEATS template argument of the instantiation (its name in a profile: rt::pathtrace_kernel<double, FEATSu>),
 * [2] how the shape was chosen (0 the scene leaves no choice, 1 size rule, 2 calibration, 3 the caller's flag, 4 rt_scene_set_loop_shape),
 * [3] precision (0 f64, 1 f32); calibration_ms2 (may be NULL): the stored calibration's kernel times {lock-step, persistent}, 0 if none. */
int rt_scene_calibrate(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                       uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags);
int rt_scene_set_loop_shape(rt_scene*, int shape);
int rt_scene_loop_shape(rt_scene*);      /* the stored shape: 1 / 0, -1 none (a calibration's result applies to the view it measured) */
int rt_last_loop_info(rt_scene*, int32_t out4[4], float calibration_ms2[2]);
/* Milliseconds of the most recent path-tracing kernel launched by this library on this thread's scene,
 * from HIP events recorded on the launch stream (blocks until that kernel finishes). */
int rt_last_kernel_ms(rt_scene*, float* ms_out);
/* Total duration (ms, HIP events on the launch streams) and number of this scene's path-tracing kernels since the last
 * reset; waits for launches still in flight.  Launches of one scene on different streams may overlap (up to four streams; a
 * frame's drain then hides behind the next frame's start); launches on one stream are ordered by the stream. */
int rt_kernel_time_total(rt_scene*, double* ms_total, unsigned long long* n_launches, int reset);
/* Counters of the most recent FRAME — one launch for rt_render / rt_render_device, the N launches of an rt_render_multi* frame summed
 * (N devices or virtual ranks) —: [0] samples whose radiance was not finite (the reference's
 * 0*inf / x/0 cases), [1] bounce-loop iterations summed over wavefronts, [2] lane-iterations
 * that carried a live path ([2] / (64*[1]) = lane utilisation). */
int rt_last_stats(rt_scene*, unsigned long long out3[3]);
/* Geometry of the most recent launch: [0] workgroups, [1] threads per workgroup, [2] dynamic LDS bytes per workgroup, [3] BVH nodes
 * staged in LDS by each workgroup (the top levels of the trees), [4] BVH nodes in the scene, [5] resident workgroups per CU. */
int rt_last_launch_info(rt_scene*, uint32_t out6[6]);
/* The first-hit ring of the most recent launch (the lean f64 list-scene kernels): [0] entries per wave, [1] bytes per entry
 * (98 x 80: the compact form, 76 x 104: the wide one; both 0 for every other kernel), [2] 1 when the launch ran the lean f64 kernel with
 * the wide ring, whose symbol is rt::pathtrace_wide_ring_kernel<double> and not the instantiation rt_last_loop_info names, 0 otherwise. */
int rt_last_ring_info(rt_scene*, uint32_t out3[3]);
/* Per-pixel accumulator flushes of the most recent finished launch; each is three f64 atomic adds to the frame — the
 * kernel's only global write traffic (used to calibrate the WRITE_SIZE counter). */
int rt_last_flush_count(rt_scene*, unsigned long long* out);
/* Scenes with a BVH (persistent-traversal kernel): [0] advance passes, [1] lanes taking part in them, [2] traversal
 * steps, [3] lanes stepping, all summed over wavefronts ([3] / (64*[2]) = lane utilisation of the traversal). */
int rt_last_traversal_stats(rt_scene*, unsigned long long out4[4]);
/* Persistent-traversal kernels: of the traversal steps above, [0] the leaf steps (primitive tests) and [1] the lanes in them. */
int rt_last_leaf_steps(rt_scene*, unsigned long long out2[2]);
/* Diagnostic builds (-DRT_DIAG) only (zeros in a normal build): [0..5] wave-cycle sums of the six kernel sections, [6] rect tests
 * counted per wavefront, [7] those among them in which no lane's plane distance lay in [t_min, closest] (-DRT_DIAG_RECTS builds). */
int rt_debug_section_cycles(rt_scene*, unsigned long long out8[8]);
/* Test aid (host only, no GPU): the compiled-in launch limits of the element-wise kernels, so that a test can choose the smallest frame that takes
 * a loop into its second trip and can tell that it did.  Writes min(max_words, RT_LOOP_LIMITS_WORDS) words and returns RT_LOOP_LIMITS_WORDS:
 * [0] [1] workgroups at most / threads of the kernels of rt_denoise_frame_device (a lane takes one PAIR of doubles per trip), [2] [3] the same
 * for the variance kernels (rt_moments_variance_device), [4] pixels per workgroup of the selection's compaction, [5] workgroup counts its
 * scan takes per trip (one workgroup of that many lanes), [6] workgroups at most of the error and counts-aware resolve kernels, [7] threads of
 * the adaptive element-wise kernels (the resolve takes 4 pixels per lane and trip), [8] workgroups at most of the others, [9] [10] [11]
 * workgroups at most / threads / pixels per lane and trip of rt_progressive_resolve_rgb8, [12] threads of the ray and albedo query kernels,
 * [13] [14] threads / default paths per chunk of the radiance queries, [15] [16] the same for the pixel-list kernel. */
#define RT_LOOP_LIMITS_WORDS 17u
int rt_debug_loop_limits(uint32_t* out, uint32_t max_words);
/* Measuring aid (tools/denoise_probe.py): rt_denoise_device on the null stream, synchronously, once to warm up and once with HIP events between its
 * launches: ms_out[0] = the pack kernel, ms_out[1 + i] = iteration i (iterations + 1 floats). */
int rt_debug_denoise_ms(const void* d_rgb_sum, uint64_t samples, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                        const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, float* ms_out);
/* The same for rt_denoise_variance_device (d_var_out NULL): ms_out[0] = the guide and colour packs, ms_out[1] = the 3 x 3 prefilter of v,
 * ms_out[2 + i] = iteration i (iterations + 2 floats). */
int rt_debug_denoise_variance_ms(const void* d_rgb_sum, uint64_t samples, const void* d_var, const void* d_hits, uint32_t W, uint32_t H, uint32_t iterations,
                                 const double sigma[3], uint32_t flags, void* d_rgb_sum_out, void* d_workspace, size_t workspace_bytes, float* ms_out);
/* Measuring aid (tools/denoise_probe.py): the two element-wise kernels of rt_denoise_albedo_device on the null stream, synchronously, once to
 * warm up and once with HIP events between them: ms_out[0] = demodulate (d_rgb_sum, d_albedo_sum -> d_x), ms_out[1] = remodulate (d_x in place).
 * DEVICE pointers of n_doubles doubles (3 per pixel), 8-byte aligned. */
int rt_debug_albedo_modulate_ms(const void* d_rgb_sum, const void* d_albedo_sum, uint64_t albedo_samples, void* d_x, uint64_t n_doubles, float ms_out[2]);
/* Test aid (host only, no GPU): what rt_scene_calibrate does to the filter tree of a world that is ONE bare BVH — inner nodes leave it by
 * their estimated pass rate for the view instead of by box areas (rt_flatten.cpp tune_filter_tree; scheduling only: any conservative
 * hierarchy over the leaves gives the same samples) — without touching a device copy.  1: rebuilt, 0: not that kind of scene, -1: error. */
int rt_debug_tune_filter(rt_scene*, const rt_camera*);
/* Test aid (host only, no GPU): the flattened object table, out[8 i ..] = {geometry kind (0 rect, 1 sphere, 2 moving sphere, 3 triangle,
 * 4 BVH root), first primitive / root node, count, first wrapper op, number of wrapper ops, medium index (0xFFFFFFFF: none), is_cube
 * (1: the six rects are one Cube's faces; 2 | map << 8: a ROOM — bare AARects of a list scene that are exact faces of one axis-aligned box,
 * searched as one object where the last of them stood, through the Cube fast path with a face map: three bits per face in cube.rs:17-24
 * order = the wall's place in the room's run of rect records, 7 = no such wall; first_op then holds five bits per wall, the index of the
 * first object that stood after that wall and is searched before the room — an exact tie with an object at or beyond it goes to that
 * object, as hit.rs:62-68 gives it to the later item; rt_flatten.cpp form_room), nest (sub-objects: wrapper ops outside the enclosing BVH | ops outside the medium << 8; bit 16:
 * every wrapper is a FlipNormal)}: the
 * world's top-level objects (HittableList push order,
 * runs of bare primitives merged) first — *n_top_out of them — then the sub-objects BVH leaves of other Hittable kinds refer to, or — a list
 * scene in which a room was formed — the world list as the reference has it (what a wave searches when one of its rays could produce a NaN
 * plane distance, rt_kernel.hip world_hit_list).
 * Returns the number of objects or -1. */
int rt_debug_objects(rt_scene*, uint32_t* out, uint32_t max_objects, uint32_t* n_top_out);
/* Test aid (host only, no GPU): the flattened BVH's link words, out[4*i..] = node i's {a, b, c, skip}: `a` bit 31 marks a leaf (then kind
 * and first primitive; b = count, c = the leaf's rank in the reference's depth-first order), otherwise a = split axis, b = right child,
 * c = left child; skip = the node BVH::hit's recursion (src/bvh.rs:77-91) reaches next once this node's subtree is finished or culled
 * (0xFFFFFFFF: the search is over).  roots_out: root node of every BVH object of the world list.  Returns the node count or -1. */
int rt_debug_bvh_links(rt_scene*, uint32_t* out, uint32_t max_nodes, uint32_t* roots_out, uint32_t max_roots, uint32_t* n_roots_out);
/* Test aid (host only, no GPU): the filter tree the kernels' box steps walk — the f32 companion of every node of the tree above
 * (same ids): boxes6_out[6 i ..] = {min.x, max.x, min.y, max.y, min.z, max.z} rounded OUTWARD to f32, links2_out[2 i ..] = {skip, info}
 * (info: the first child, or for a leaf its own id | 0x40000000; near-duplicate inner nodes have been taken out of these links),
 * f64_boxes_out[6 i ..] = the exact box {min[3], max[3]}; *filter_m_out >= every |coordinate| of the f32 boxes (0: filter off).
 * Any of the output pointers may be NULL.  Returns the node count or -1. */
int rt_debug_filter_nodes(rt_scene*, float* boxes6_out, uint32_t* links2_out, double* f64_boxes_out, uint32_t max_nodes, float* filter_m_out);
/* Test aid: AABB::hit (src/aabb.rs:19-36) evaluated on the device for n (box, ray, [t_min, t_max]) triples given as host arrays
 * (boxes: min[3] max[3]; rays: origin[3] direction[3]).  out[i] bit 0: hit by the reference's form; bit 1: by the NaN-free form the
 * leaf steps use for tame rays; bit 2: the ray qualifies for that form (finite 1/d, |origin| < 1e300); bit 3: ray and box are inside the
 * ranges of the box steps' conservative f32 filter (rt_kernel.hip: make_filter); bit 4: that filter lets the box through (it must
 * wherever bit 0 is set; it may elsewhere); bits 5, 6, 7: for the f32 kernels (RT_F32) — AABB::hit's form in f32 on the inputs rounded to
 * nearest (what their leaf steps run), tame ray and filter ranges, their filter's verdict (it must pass wherever bit 5 is set).
 * Non-zero on a HIP error. */
int rt_debug_aabb_hit(uint32_t n, const double* boxes, const double* rays, const double* tlim, int* out);
/* Test aid: Cube::hit (src/cube.rs:14-36: HittableList::hit over six AARects) on the device for n (cube, ray, [t_min, t_max]) triples
 * given as host arrays (boxes: min[3] max[3]; rays: origin[3] direction[3]); rect_m as KParams::rect_m (>= every |coordinate|).
 * out[4 i ..] = t of the six exact rect tests in cube.rs order (NaN: no face accepted), the accepted face (0..5 in cube.rs:17-24 order,
 * -1), t of the fast path (rt_kernel.hip: cube_fast; NaN: no hit), 8 * clear + (face + 1) of the fast path (clear:
 * the lane's outcome is outside the approximation's margin — otherwise the kernels run the six tests).  Non-zero on a HIP error. */
int rt_debug_cube_hit(uint32_t n, double rect_m, const double* boxes, const double* rays, const double* tlim, double* out);
/* The same for the fast path's ROOM form (round 6: walls of a list scene that are faces of one box, rt_flatten.cpp form_room): masks[i]
 * says which of the six faces exist (bit f = face f in cube.rs:17-24 order); the exact side is HittableList::hit (hit.rs:59-71) over
 * the AARects of those faces.  out as above. */
int rt_debug_room_hit(uint32_t n, double rect_m, const double* boxes, const double* rays, const double* tlim, const uint32_t* masks, double* out);
/* Known-answer access to the closest-hit search of a LIST scene (no feature bit: what the lean kernels serve — rects, Cubes, wrapped ones):
 * world.hit (main.rs:48, HittableList::hit hit.rs:59-71) and the hit record for n given rays through the kernels' own search.  rays: n x
 * (origin[3], direction[3]); t_min: n; out: n x 12 = hit (0 / 1), t, position[3], normal[3], front_face, object index, primitive index,
 * material.  Host pointers.  What the room form's order argument rests on is tested through this: rays that start ON planes, with zero
 * direction components (0 / 0 plane distances), non-finite rays. */
int rt_debug_list_hit(rt_scene*, uint32_t n, const double* rays, const double* t_min, double* out);
/* The same through the search as the lean f64 kernel's primary pass runs it: top-level objects whose bit of `mask` is clear are not
 * searched — except by a wave (64 consecutive rays of the array) in which some ray has a zero, denormal or non-finite direction component
 * or a non-finite origin: that wave searches the list as the reference has it, in full.  Arguments and out as rt_debug_list_hit. */
int rt_debug_list_hit_masked(rt_scene*, uint32_t n, const double* rays, const double* t_min, uint32_t mask, double* out);
/* Known-answer access to the scene's `lights` pdf_value (HittableList::pdf_value, hit.rs:90-92, nested lists included) on the device, through
 * the function the all-features kernel with object leaves runs (the instantiation every scene with a list inside `lights` gets).  origins,
 * dirs: n x 3; out: n.  Host pointers. */
int rt_debug_light_pdf(rt_scene*, uint32_t n, const double* origins, const double* dirs, double* out);
/* Known-answer access to the per-face ONB memo of the lean f64 list-scene kernel (rt_kernel.hip onb_memo_probe / onb_memo_load: the
 * device functions its Lambertian arm calls) for n pairs of (rect index, normal).  rects: n doubles, each a rect record's index;
 * normals: n x 3; out: n x 7 = memo hit (0 / 1), then v[3], u[3] of ONB::build_from_w(normal) (onb.rs:8-20) as the table holds them
 * (zeros on a miss).  A hit requires |normal| to equal the entry's magnitudes bit for bit.  Host pointers. */
int rt_debug_onb(rt_scene*, uint32_t n, const double* rects, const double* normals, double* out);
/* Test aid (host only, no GPU): the per-face ONB memo as flattened, one entry per rect record: mag_out[3 i ..] = the bit patterns of
 * |n.x|, |n.y|, |n.z| of the hit normal the rect's owner produces (all ones: no valid entry — an f32-only use, a scene with a feature bit,
 * a chain other than bare / FlipNormals / Translate(RotateY(..)), a rect reachable through more than one chain, RT_NO_ONB_TABLE),
 * slots_out[48 i + 6 s ..] = {v[3], u[3]} for the sign bits s = sx | sy << 1 | sz << 2.  Either pointer may be NULL.  Returns the number
 * of rect records, *n_valid_out the number of valid entries; -1 on error. */
int rt_debug_onb_table(rt_scene*, uint64_t* mag_out, double* slots_out, uint32_t max_rects, uint32_t* n_valid_out);
/* Test aid (host only, no GPU): the form of the first-hit ring this scene's frames get from the lean f64 kernels: *entries_out per wave of
 * *entry_bytes_out each.  98 x 80, the compact form, where every rect record has a valid ONB-table entry (the normal of a queued hit is then
 * three sign bits: the table holds its magnitudes); 76 x 104, the wide form, for every other list scene and under RT_NO_PRIMARY_PASS; 0 x 0
 * where those kernels do not run (a scene with a feature bit, RT_F32 in flags).  Returns 1 for the compact form, 0 otherwise, -1 on error. */
int rt_debug_ring_form(rt_scene*, uint32_t flags, uint32_t* entries_out, uint32_t* entry_bytes_out);
/* Known-answer access to the normal of a compact first-hit record (rt_kernel.hip ring_pack_signs / ring_normal, the device functions the
 * lean f64 kernel's loop calls): world.hit and the hit record for n given rays, the record's normal packed into three sign bits and rebuilt
 * from the ONB table.  rays: n x (origin[3], direction[3]); t_min: n; out: n x 8 = hit (0 / 1), rect index (-1 on a miss), the hit record's
 * normal[3], the rebuilt normal[3] (zeros on a miss).  Only for scenes whose ring is compact (rt_debug_ring_form).  Host pointers. */
int rt_debug_ring_normal(rt_scene*, uint32_t n, const double* rays, const double* t_min, double* out);
/* Test aid (host only, no GPU): the ONB table's companion records, one per rect record: wmag_out[3 i ..] = the bit patterns of
 * |w.x|, |w.y|, |w.z| of w = normalized(n) (onb.rs:10) for the hit normal n the rect's owner produces — the normalisation sees no sign, so
 * these are constants of the rect as rt_debug_onb_table's mag are; all ones exactly where that entry is invalid.  wmag_out may be NULL.
 * Returns the number of rect records; -1 on error. */
int rt_debug_onb_table_w(rt_scene*, uint64_t* wmag_out, uint32_t max_rects);
/* Known-answer access to w as the compact lean f64 kernel's material section takes it from those records (rt_kernel.hip ring_w): world.hit
 * and the hit record for n given rays, then normalized(the record's normal) by the kernel's own normalisation, and the table's magnitudes
 * with the normal's sign bits.  rays, t_min as rt_debug_ring_normal; out: n x 8 = hit (0 / 1), rect index (-1 on a miss),
 * normalized(normal)[3], the table's w[3] (zeros on a miss).  Only for scenes whose ring is compact.  Host pointers. */
int rt_debug_ring_w(rt_scene*, uint32_t n, const double* rays, const double* t_min, double* out);
/* The pixel classifier of the lean f64 list-scene kernel's primary pass (csrc/rt_primary.h): the kernel runs the first level of the camera
 * paths of a refill together and does not search top-level objects that every ray it can generate for their pixel provably misses.  For
 * n pixels (pixels: n x (i, j), j counted from the bottom row) out_masks[p] has bit k set when object k of the flattened top-level list may
 * be hit (a clear bit is a proof; a list of more than 32 objects gives all ones).  rt_debug_primary_mask runs the kernel that writes a
 * frame's masks before its launch, one thread per pixel (needs a GPU); rt_debug_primary_mask_host is its host twin (no GPU).  Host
 * pointers.  Environment, read once per launch like RT_NO_SHORT_DIV (A/B runs, tests): RT_NO_PRIMARY_PASS renders without the pass — the
 * other list kernels' loop, its queue refilled with camera paths; samples are the same 64-bit words; it is a switch for comparing
 * samples, no timing stand-in for an earlier build; RT_NO_PRIMARY_MASK keeps the pass and treats every object as a candidate. */
int rt_debug_primary_mask(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint32_t* out_masks);
int rt_debug_primary_mask_host(rt_scene*, const rt_camera*, uint32_t W, uint32_t H, const uint32_t* pixels, uint32_t n, uint32_t* out_masks);
/* Known-answer access to the exact short forms of the lean f64 list-scene kernel (csrc/rt_short.h; rt_kernel.hip div_pi_pair, div_frame,
 * rng_u01_of, rect_absdot: the device functions its sites call) on n caller operands, one per lane, waves of 64 — the guards vote per wave.
 * op 0, the Lambertian arm's two divisions by pi: a = n cosines, b = n values of max(dot, 0); out = n x 3: cosine > 0 ? cosine / pi : 0,
 *       b / pi, and 1 if the record's wave took the three-instruction form (0: the plain divisions).
 * op 1, the camera's division by W - 1 or H - 1: a = n numerators, b = n x 2: the divisor and its reciprocal as the host enabled it (0: the
 *       plain division); out = n quotients.
 * op 2, U01: a = n 64-bit words (each a u64 as drawn, stored in the double's place), b unused (may be NULL); out = n values of U01.
 * op 3, AARect::pdf_value after its hit test: a = n x 3 directions v, b = n x 3: t, the plane's axis k (0, 1, 2), the area; out = n x 2: the
 *       pdf, and 1 if the record's wave took |v_k| for |dot(v, n)| (0: the two dot products).
 * Host pointers; no scene.  Returns 0, -1 on a bad argument or a device error. */
int rt_debug_short_forms(uint32_t op, uint32_t n, const double* a, const double* b, double* out);
/* Known-answer access to the arithmetic of the SHADING side (csrc/rt_kat.hip over rt_kernel.hip's device functions): one device function per
 * lane on n caller operands, f64.  The two units the frames are built from compile the shared source in two code shapes; op selects the
 * lean (list-scene) unit's, op | RT_KAT_REST_SHAPE the other unit's.  Doubles per record of a / b / out:
 *   0 sincos_0_2pi(phi): 1 / 0 / 2 (sin, cos);  1 sin, 2 cos, 3 tan, 4 atan, 6 acos, 7 log, 8 log2: 1 / 0 / 1;  5 atan2(a, b), 9 pow(a, b): 1 / 1 / 1;
 *   10 Vec3 / f64: 3 / 1 / 4 (the quotients, then 1 if the lane took the shared-denominator form, 0 for the three plain divisions);
 *   11 onb_from_w(n): 3 / 0 / 9 (u, v, w);  12 GTR_1(n_dot_h, a): 1 / 1 / 1;  13 GTR_2_aniso(n_dot_h, h_dot_x, h_dot_y; ax, ay): 3 / 2 / 1;
 *   14 smithG_GGX(n_dot_v, alphaG): 1 / 1 / 1;  15 smithG_GGX_aniso(n_dot_v, v_dot_x, v_dot_y; ax, ay): 3 / 2 / 1;  16 schlick_fresnel(u): 1 / 0 / 1.
 * b may be NULL where its record is empty.  Host pointers; no scene.  Returns 0, -1 on a bad argument or a device error. */
#define RT_KAT_REST_SHAPE 0x100u
int rt_debug_math(uint32_t op, uint32_t n, const double* a, const double* b, double* out);
/* Material::brdf (mat.rs:133-195) and PDF::BRDF value (pdf.rs:97-130, on ONB::build_from_w(normal)) of one PBR material of the scene, on the
 * device through the functions shade_hit's principled arm calls (pbr_brdf, brdf_pdf_value), for n caller records.  r_in, r_out, normal,
 * base (the base colour the texture would give): n x 3 each; out: n x 4 = brdf[3], pdf value.  shape: 0 or RT_KAT_REST_SHAPE, as above.
 * Host pointers. */
int rt_debug_brdf(rt_scene*, uint32_t n, int material, const double* r_in, const double* r_out, const double* normal, const double* base, double* out, uint32_t shape);
/* ONE level of ray_color after the hit (main.rs:50-116) per record, through the function the frames' bounce loops call (rt_kernel.hip shade_hit).
 * records: n x 16 in rt_query_hits' layout (every one a hit; in a list scene the primitive index names the rect whose ONB memo entry the
 * Lambertian arm probes); rays: n x 7, the incoming rays; beta: the throughput every lane starts with; record k draws from
 * rt_rng_path(seed, k, 0); depth_left >= 1.  flags: RT_STOP_ON_ZERO, RT_ISOTROPIC_SCATTER; RT_KAT_REST_SHAPE — the all-features instantiation
 * under the other unit's code shape (with object leaves and nested light lists where the scene has them) instead of the lean one (list scenes
 * only); RT_KAT_NO_ONB_TABLE — the lean one without the ONB memo; RT_KAT_TABLE_W — the call as the COMPACT lean f64 kernel's material section
 * makes it, the one the frames of every scene with the compact first-hit ring run: the rect word packed with `front_face` and the normal's
 * three sign bits, the normal rebuilt from the ONB table, then the instantiation whose Lambertian / Metal arm takes w, v and u from the
 * table (rt_kernel.hip ring_pack_signs, ring_normal, shade_hit<double, 0, true>).  It is refused, before any device call and with the
 * record's number in the message, together with either of the other two RT_KAT_ flags, for a scene whose ring is not compact
 * (rt_debug_ring_form), for a record whose material is neither Lambertian nor Metal (that kernel ends every other path before the call) and
 * for a record whose sign-masked normal words are not its rect's magnitudes in the ONB table (the compact record carries the normal as three
 * sign bits: rt_debug_onb_table).  out: n x 19 = the ray afterwards (7; the incoming ray where nothing scatters), beta[3], e[3] (the terminal
 * radiance beta multiplies), done (0 / 1), depth_left, the stream's four state words afterwards.  Host pointers. */
#define RT_KAT_NO_ONB_TABLE 0x200u
#define RT_KAT_TABLE_W 0x400u
int rt_debug_shade(rt_scene*, uint32_t n, const double* records, const double* rays, const double beta[3], uint64_t seed, uint32_t depth_left,
                   uint32_t flags, double* out);
/* Debugging aid for parity work: the hits of ONE camera path, level by level.  rt_debug_trace_path chooses the path (local pixel index =
 * output-order pixel for an unsharded render, sample index; -1 switches it off); the following renders record, per level of ray_color
 * that found a hit, 16 doubles at out[16 * level]: t, position[3], normal[3], front_face, object, primitive kind, primitive index,
 * material, incoming direction[3], 1.0 (a level without a hit stays all zero); rt_debug_get_trace fetches n_levels of them.  Only the
 * lock-step kernels of a -DRT_TRACE_PATH build of the library write the record (tools/mkab.sh trace "-DRT_TRACE_PATH" "-DRT_TRACE_PATH";
 * the shipped build leaves it zero) — tests/sweeps/fuzz_probe.py compares it with the oracle's orc_trace_path. */
int rt_debug_trace_path(rt_scene*, long long local_pixel, long long sample);
int rt_debug_get_trace(rt_scene*, double* out, uint32_t n_levels);
/* Debug/parity aid: like rt_render but also returns every sample's radiance (W*H*spp*3 doubles). */
int rt_render_samples(rt_scene*, const rt_camera*, const double background[3], uint32_t W, uint32_t H,
                      uint32_t samples_per_pixel, uint32_t max_depth, uint64_t seed, uint32_t flags,
                      double* rgb_sum_out, double* samples_out);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
