/*
 * ipt.h -- C ABI of the MI355X-native inverse path tracer
 * (inverse_path_tracer_amd/lib/libipt_amd.so, also installed as
 * build/libpt.so and build/libipt.so so the reference's ipt_cuda.py loads it
 * unchanged).
 *
 * Part 1 is the reference's own FFI surface, symbol for symbol, with the
 * reference's signatures (the reference's ctypes caller sets no argtypes, so
 * these are plain C ints and pointers).  Part 2 is the explicit-parameter API
 * the reference hard-codes at compile time (scene.h:3-13), plus the adjoint.
 *
 * Errors: the reference exit(1)s on bad input and ignores CUDA errors.  Here
 * no entry point exits; failures return -1 (or leave outputs untouched for the
 * void legacy symbols) and ipt_last_error() says why (thread-local).
 */
#ifndef IPT_H
#define IPT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Part 1: reference symbols                                           */
/* ------------------------------------------------------------------ */

/* Replaces scene.h:177-193 loadScene.  Builds the scene from n object
 * records (pos/ori/scl float[3] each, OBJ path, MTL path or inline
 * "*Kd r g b*") and uploads it to the current HIP device.  Returns the
 * triangle count nT (the reference's return value) or -1 on error, in which
 * case *scenePtr = NULL. */
int loadScene(float **poss, float **oris, float **scls, char **obj_fs, char **mtl_fs, int n,
              void **scenePtr);

/* Replaces scene.h:195-199 freeScene. */
void freeScene(void *scenePtr);

/* Replaces path_trace.cu:227-234 createImage: renders the legacy
 * configuration (500x500, 100 spp, unbounded bounces, seed = time(NULL)
 * unless ipt_legacy_config() set one) and writes an RGB8 PNG tonemapped
 * with 255*x/(1+x). */
void createImage(void *scenePtr, char *img_file);

/* Replaces inv_path_trace.cu:195-208 createGraph: renders the transport
 * graph against the target PNG (must match the legacy image size) and
 * writes (nT+1)*nT*7 floats: weights[(nT+1)*nT] | pixel[(nT+1)*nT*3] |
 * light[(nT+1)*nT*3] (ipt_cuda.py:145-163 layout; eye row last). */
void createGraph(void *scenePtr, char *imgFile, float *data);

/* Replace inv_path_trace.cu:210-221: per-triangle diffuse Kd, nT*3 floats,
 * object-major then triangle, RGB inner (scene.h:145-162). */
void getMaterials(void *scenePtr, float *materials);
void setMaterials(void *scenePtr, float *materials);

/* ------------------------------------------------------------------ */
/* Part 2: explicit API                                                */
/* ------------------------------------------------------------------ */

/* Render configuration.  max_bounces < 0 reproduces the reference
 * (paths end only by Russian roulette or a miss); max_bounces = B allows B
 * continuation rays and does next-event estimation at the (B+1)-th vertex.
 * Sample s of pixel (r,c) has global index (r*width + c)*spp + s and RNG
 * seed `seed + index` (curand_init(seed+index, 0, 0)).  Only rows
 * row_begin, row_begin + row_step, ... < row_end are traced (sharding:
 * row_step 1 = a contiguous band, row_step = world = a rank's interleaved
 * share); images and sample buffers hold those rows, in that order.
 * ABI 2 added row_step; ABI 3 dropped the quantised-node export of
 * ipt_scene_export_wide; ABI 4 added ipt_debug_fail_launches; ABI 5 added
 * ipt_debug_adju_ring; ABI 6 added ipt_debug_last_launch
 * (ipt_abi_version).  Bindings must check the version
 * before passing this struct. */
typedef struct ipt_params {
  int32_t width, height, spp, max_bounces;
  uint64_t seed;
  int32_t row_begin, row_end;
  int32_t row_step;
} ipt_params_t;

const char *ipt_last_error(void);
void ipt_clear_error(void);
int ipt_abi_version(void);            /* 6 */
int ipt_device_count(void);
/* Diagnostic: bitwise self-test of the kernels' in-range sqrt/division cores
 * against the IEEE operations over n random operands per test; counts[8]
 * receives mismatch counts (0 expected; counts[6] is the number of unit()
 * fast-path hits, not a mismatch).  No reference counterpart. */
int ipt_selftest_math(uint64_t n, uint64_t seed, uint64_t *counts);
/* Diagnostic (tests): the next n trace-kernel launches fail with an error
 * just before their kernel is enqueued -- after the launch's chunk counters
 * and scratch are allocated.  A later launch on the same stream must be
 * unaffected (the counters reset themselves on the device).  No reference
 * counterpart. */
void ipt_debug_fail_launches(int n);
/* Diagnostic (tests): the number of trace launches since the library was
 * loaded that read a small scene's shading data from the LDS tables (the
 * trace_shade_kernel instances).  No reference counterpart. */
int ipt_debug_shade_launches(void);
/* Diagnostic (tests): the numbers the host decided for the last trace launch
 * of the process, so that a test can assert which kernel instance and which
 * LDS layout a scene got.  Writes the first n of these int32 fields to out and
 * returns how many fields there are (18):
 *    0 launches recorded since the library was loaded
 *    1 MODE  (0 forward, 1 bounded adjoint, 2 graph, 3 unbounded adjoint,
 *            4 forward with the fused pixel mean, 5 six-wave bounded adjoint)
 *    2 SPEC  (the Phong-lobe instance)      3 BVH (1) or the pair loop (0)
 *    4 KIND  (0 trace, 1 material adjoint, 2 batch forward, 3 views forward,
 *            4 views adjoint, 5 view-sets forward, 6 view-sets adjoint,
 *            7 shading tables in LDS, 8 tangents)
 *    5 kd_tables: Kd and Kd/pi (and a tangent launch's tangents) in LDS
 *    6 small_pairs: bit 0 unrolled pair loop, bit 1 shading tables in LDS
 *    7 grad_slots: gradient bins in LDS (nT: all of them)
 *    8 bvh_wide_lds: wide BVH nodes staged in LDS (0: none)
 *    9 rec_lds: unbounded adjoint, ring slots per lane in LDS
 *   10 lds_edges: graph bins in LDS
 *   11 LDS bytes per workgroup             12 rec_cap (vertex records per lane)
 *   13 bvh_big_lds: large pairs copied to LDS
 *   14 BVH emitter records in LDS           15 grid (workgroups)
 *   16 nT   17 nE
 * The record is taken just before the kernel is enqueued; a launch that was
 * refused, failed earlier or traced no sample leaves it unchanged.  No
 * reference counterpart. */
int ipt_debug_last_launch(int32_t *out, int n);
/* Diagnostic (tests): the unbounded adjoint's record ring at reduced sizes --
 * pool_chunks 16-slot chunks per wave pool (1..63) and lds_slots LDS slots
 * per lane (>= 1); 0 restores the launch's own choice.  Small pools make
 * lanes find the pool empty and shorten their rings (replays), the paths the
 * default sizes almost never take.  Gradients are unchanged.  No reference
 * counterpart. */
void ipt_debug_adju_ring(int pool_chunks, int lds_slots);

/* Legacy-symbol configuration (defaults 500, 500, 100, -1, seed -1 = time). */
void ipt_legacy_config(int width, int height, int spp, int max_bounces, int64_t seed);

/* Same as loadScene with flat arrays (pos/ori/scl: n*3 floats). */
int ipt_load_scene(int n, const float *pos, const float *ori, const float *scl, const char **obj_files,
                   const char **mtl_files, void **scenePtr);
/* Host-only scene (no device buffers): export / materials only; render
 * entry points fail on it.  Lets CPU-only tooling check scene ingest. */
int ipt_load_scene_host(int n, const float *pos, const float *ori, const float *scl, const char **obj_files,
                        const char **mtl_files, void **scenePtr);
int ipt_scene_num_triangles(void *scene);
int ipt_scene_num_emissives(void *scene);
/* nT*57 floats: v0..v2, vertex normals, face normal, centre, area, Kd, Ks,
 * Ke, shininess, three edge planes, sampling frame, emissive index. */
int ipt_scene_export_triangles(void *scene, float *out);
/* getMaterials / setMaterials with a status (nT*3 floats, host memory). */
int ipt_scene_get_materials(void *scene, float *kd);
int ipt_scene_set_materials(void *scene, const float *kd);
int ipt_scene_camera(void *scene, float *out16);

/* Acceleration structure for closest-hit queries.  The reference's BVH
 * (bvh.h:109-205) is over objects and, for its <= 4-object scenes, one leaf:
 * brute force over all triangles, ties to the lowest index
 * (scene_basics.h:426-459, bvh.h:55-77).  Here scenes of >= 64 triangles
 * trace a triangle BVH that returns exactly the same hits;
 * AUTO picks it, BRUTE/BVH force either (BVH fails if the scene has none). */
#define IPT_ACCEL_AUTO 0
#define IPT_ACCEL_BRUTE 1
#define IPT_ACCEL_BVH 2
int ipt_scene_set_accel(void *scene, int mode);
/* info8 = {nodes, leaf pairs, depth, accel in use (IPT_ACCEL_BRUTE/BVH),
 * large-triangle pairs tested before the traversal, 8-wide nodes, 8-wide
 * levels, leaf triangles of the 8-wide tree}; returns 1 if
 * the scene has a BVH, 0 if not (ipt_last_error says why). */
int ipt_scene_bvh_info(void *scene, int32_t *info8);
/* nodes: info8[0]*16 floats (BvhNode), pairs: info8[1]*40 floats (BvhPair:
 * 18 field pairs, then 2 int32 triangle indices, 2 pad), big_idx:
 * info8[4]*2 int32 (the pre-pass triangles, 0x7fffffff = padding); each
 * nullable. */
int ipt_scene_export_bvh(void *scene, float *nodes, float *pairs, int32_t *big_idx);
/* The 8-wide nodes of the cooperative traversal (info8[5] of them): wide
 * receives info8[5]*64 floats (WideNode: per child lo.xyz, hi.xyz, ref bits,
 * pad; nullable). */
int ipt_scene_export_wide(void *scene, float *wide);
/* The shadow rays' potential occluders (bvh.cpp shadow_occluder_masks):
 * masks receives nT * max(nE, 1) words, word [s * nE + e] = the pairs (bit j
 * = triangles 2j, 2j+1) that may occlude a shadow ray from a vertex on
 * triangle s to a point on emitter e (all pairs when not bounded). */
int ipt_scene_shadow_masks(void *scene, uint32_t *masks);
/* Closest hit of n rays (origins, dirs: n*3 floats) through the kernels'
 * own cast: idx = triangle index or -1, t = its distance.  targets
 * (nullable, n ints): >= 0 marks a next-event shadow ray towards that
 * emitter triangle, for which only "idx == target" and then t are defined
 * (the BVH stops once the target is known to be occluded; small scenes use
 * the megakernel's culled shadow cast, which reports -1 when occluded);
 * < 0 a path ray through the megakernel's path cast (small scenes: the
 * culled pair loop).  Without targets small scenes run the full pair loop.
 * Directions need not be unit vectors (t is then in units of |dir|): the
 * BVH's tree-entry culls that assume |dir| = 1, as the megakernel's rays
 * have, are applied only to rays with |dot(dir, dir) - 1| <= 2^-20. */
int ipt_closest_hit_host(void *scene, int64_t n, const float *origins, const float *dirs, const int32_t *targets,
                         float *t, int32_t *idx);
int ipt_closest_hit_dev(void *scene, int64_t n, const float *origins_dev, const float *dirs_dev,
                        const int32_t *targets_dev, float *t_dev, int32_t *idx_dev, void *stream);
/* Rays exactly as the megakernel casts them from a path vertex:
 * sources[i] >= 0 is the triangle the origin lies on (a point its hit test
 * accepted), which selects the static potential-occluder mask of (source,
 * emitter) on top of the culled shadow cast, and in BVH scenes the tree's
 * source-plane skip; < 0 = none.  targets[i] >= 0 = a shadow ray towards that
 * emitter, < 0 = a bounce ray (the path cast), as in ipt_closest_hit_host
 * (both arrays required). */
int ipt_shadow_hit_host(void *scene, int64_t n, const float *origins, const float *dirs, const int32_t *targets,
                        const int32_t *sources, float *t, int32_t *idx);

/* Host-memory entry points (synchronous). */
int ipt_render_samples_host(void *scene, const ipt_params_t *p, float *samples); /* rows*W*spp*3 */
int ipt_render_host(void *scene, const ipt_params_t *p, float *hdr, uint8_t *ldr); /* rows*W*3 */
int ipt_adjoint_host(void *scene, const ipt_params_t *p, const float *adj /*H*W*3*/, double *grad /*nT*3*/);
int ipt_graph_host(void *scene, const ipt_params_t *p, const uint8_t *target /*H*W*3*/,
                   double *acc /*nullable, (nT+1)*nT*8*/, float *data /*nullable, (nT+1)*nT*7*/);
/* DataWrapper::compress (inv_scene.h:87-115) of fp64 accumulators. */
int ipt_compress(int nT, const double *acc, float *data);

/* Device-memory entry points: pointers are device pointers, `stream` a
 * hipStream_t (NULL = null stream); asynchronous.  kd_dev (nT*3) overrides
 * the scene's materials when non-NULL.  grad_dev / acc_dev ACCUMULATE (zero
 * them first). */
int ipt_render_dev(void *scene, const ipt_params_t *p, const float *kd_dev, float *hdr_dev, uint8_t *ldr_dev,
                   void *stream);
int ipt_render_samples_dev(void *scene, const ipt_params_t *p, const float *kd_dev, float *samples_dev,
                           void *stream);
int ipt_pixel_mean_dev(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev,
                       void *stream);
/* The same two steps over a sample-major buffer ([s][pixel][3], rows*W*spp*3
 * floats): the layout ipt_render_dev uses internally (coalesced mean). */
int ipt_render_samples_sm_dev(void *scene, const ipt_params_t *p, const float *kd_dev, float *samples_dev,
                              void *stream);
int ipt_pixel_mean_sm_dev(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev,
                          void *stream);
int ipt_adjoint_dev(void *scene, const ipt_params_t *p, const float *kd_dev, const float *adj_dev, double *grad_dev,
                    void *stream);
int ipt_graph_dev(void *scene, const ipt_params_t *p, const uint8_t *target_dev, double *acc_dev, void *stream);

/* Scene batch (BASELINE config C5 over scenes/0..99.txt, which share their
 * geometry and differ only in the cube's Kd; the reference renders them one
 * loadScene/createImage at a time, ipt_cuda.py:115-134): n_scenes material
 * sets over ONE loaded geometry in one launch.  Set b uses kd_dev + b*nT*3
 * and seed p->seed + b*seed_stride, and equals ipt_render_dev /
 * ipt_adjoint_dev of that kd and seed (images bit for bit, gradients to fp64
 * summation order).  hdr_dev: n_scenes*rows*W*3; adj_dev: n_scenes*H*W*3
 * (full frames, indexed by global pixel like ipt_adjoint_dev); grad_dev:
 * n_scenes*nT*3, accumulated. */
int ipt_render_batch_dev(void *scene, const ipt_params_t *p, int n_scenes, uint64_t seed_stride, const float *kd_dev,
                         float *hdr_dev, void *stream);
int ipt_adjoint_batch_dev(void *scene, const ipt_params_t *p, int n_scenes, uint64_t seed_stride, const float *kd_dev,
                          const float *adj_dev, double *grad_dev, void *stream);

/* Material parameters beyond Kd: specular Ks (with its Phong exponent Ns)
 * and emission Ke, per triangle.  STRUCTURE IS FROZEN AT LOAD: which
 * triangles are emitters (the emitter list, cdf and pmf) and which carry a
 * Phong lobe (and its exponent) are decided by the MTL files; these entry
 * points change values only.  Ke rows of non-emitters and Ks rows of
 * lobe-less triangles are ignored and stay 0, and their gradient rows are
 * exactly 0.  An emitter or lobe triangle may be given all-zero values (the
 * kernels branch on the load-time flags).  Ns is not differentiated.
 * (Additive symbols: ipt_abi_version stays 5.)
 *
 * get/set: host arrays, nT*3 floats each (ns: nT), each nullable; set
 * re-uploads the scene's tables and leaves setMaterials' behaviour as is. */
int ipt_scene_get_material_params(void *scene, float *kd, float *ks, float *ke, float *ns);
int ipt_scene_set_material_params(void *scene, const float *kd, const float *ks, const float *ke);
/* ipt_render_dev with per-launch overrides: kd_dev / ks_dev / ke_dev are
 * device arrays of nT*3 floats, NULL = the scene's own. */
int ipt_render_mat_dev(void *scene, const ipt_params_t *p, const float *kd_dev, const float *ks_dev,
                       const float *ke_dev, float *hdr_dev, uint8_t *ldr_dev, void *stream);
/* d(sum adj*I)/d(Kd, Ks, Ke) of the bounded estimator in one launch:
 * grad_dev is 3*nT*3 doubles, [Kd | Ks | Ke], ACCUMULATED (zero it first).
 * The Kd block equals ipt_adjoint_dev's.  Refused with an error:
 * max_bounces < 0 (the unbounded estimator: ipt_adjoint_mat_unbounded_dev
 * below) and max_bounces > 62. */
int ipt_adjoint_mat_dev(void *scene, const ipt_params_t *p, const float *kd_dev, const float *ks_dev,
                        const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream);
int ipt_adjoint_mat_host(void *scene, const ipt_params_t *p, const float *adj /*H*W*3*/, double *grad /*3*nT*3*/);
/* Forward mode of the same estimator: n_tangents directions in material space
 * -> n_tangents tangent images in ONE launch (the paths are traced once).
 * tkd_dev / tks_dev / tke_dev: n_tangents*nT*3 floats [k][tri][c], each
 * nullable as a whole (NULL = all zero; at least one must be given); Ks rows
 * of lobe-less triangles and Ke rows of non-emitters are never read (the
 * frozen structure).  tan_dev: n_tangents*rows*W*3 doubles [k][row][col][c]
 * over the rows of p's band in band order, like hdr, ACCUMULATED (zero it
 * first).  tan[k][p][c] = <ipt_adjoint_mat_dev's gradient under the one-hot
 * adjoint image at pixel p, tangent k> in channel c, up to fp64 summation
 * order: every fp32 term a*g of the adjoint's sweep (a = 1/spp), widened to
 * double, times the tangent's entry of the bin it would have gone to.  It is
 * the derivative of ipt_render_mat_dev's HDR mean along tangent k under the
 * forward's own paths.  One material set, the scene's own camera.  Refused
 * with an error before anything is enqueued: n_tangents outside 1..16, all
 * three tangent pointers NULL, max_bounces < 0 or > 62, more than 65535
 * triangles, a host-only scene, an LDS footprint (tangent tables of scenes up
 * to 512 triangles: n_tangents*(2*nT + nE)*12 bytes at most, plus tables and
 * vertex records) over 160 KiB.  The host form takes the scene's own material
 * values.  (Additive symbols: ipt_abi_version stays 5.) */
int ipt_tangent_mat_dev(void *scene, const ipt_params_t *p, const float *kd_dev, const float *ks_dev,
                        const float *ke_dev, int n_tangents, const float *tkd_dev, const float *tks_dev,
                        const float *tke_dev, double *tan_dev, void *stream);
int ipt_tangent_mat_host(void *scene, const ipt_params_t *p, int n_tangents, const float *tkd /*K*nT*3*/,
                         const float *tks, const float *tke, double *tan /*K*rows*W*3*/);
/* The same for the reference's own estimator (max_bounces = -1: no bounce cap,
 * Russian roulette at 0.9), whose forward is ipt_render_mat_dev with
 * max_bounces = -1: one launch of the unbounded adjoint's ring-and-replay
 * sweep, emitting all three blocks.  grad_dev as above (3*nT*3 doubles,
 * [Kd | Ks | Ke], ACCUMULATED); the Kd block equals ipt_adjoint_dev's at
 * max_bounces = -1; p's row band and row_step are honoured.  One material
 * set.  Refused with an error before anything is enqueued: max_bounces >= 0
 * (ipt_adjoint_mat_dev is the bounded call), a host-only scene, more than
 * 65535 triangles, LDS tables that leave no room for one record slot per lane
 * within 160 KiB.  (Additive symbols: ipt_abi_version stays 5.) */
int ipt_adjoint_mat_unbounded_dev(void *scene, const ipt_params_t *p, const float *kd_dev, const float *ks_dev,
                                  const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream);
int ipt_adjoint_mat_unbounded_host(void *scene, const ipt_params_t *p, const float *adj /*H*W*3*/,
                                   double *grad /*3*nT*3*/);
/* The scene batch of the two, with ipt_render_batch_dev's conventions:
 * n_scenes material sets over one geometry in one launch, set b with seed
 * p->seed + b*seed_stride.  kd_dev / ks_dev / ke_dev: n_scenes*nT*3 floats
 * [set][tri][c], each nullable (NULL = the scene's own values in every set).
 * hdr_dev: n_scenes*rows*W*3; adj_dev: n_scenes full frames indexed by global
 * pixel; p's row band and row_step are honoured.  grad_dev: n_scenes*3*nT*3
 * doubles, [set][Kd | Ks | Ke][tri][c], ACCUMULATED.  Set b equals
 * ipt_render_mat_dev / ipt_adjoint_mat_dev of its arrays and seed (images bit
 * for bit, gradients to fp64 summation order); n_scenes == 1 is the
 * single-set call.  Refused with an error before anything is enqueued:
 * n_scenes < 1, a host-only scene, max_bounces < 0 or > 62, more than 65535
 * triangles, an LDS footprint (one set's: a workgroup holds one set) over
 * 160 KiB.  (Additive symbols: ipt_abi_version stays 5.) */
int ipt_render_mat_batch_dev(void *scene, const ipt_params_t *p, int n_scenes, uint64_t seed_stride,
                             const float *kd_dev, const float *ks_dev, const float *ke_dev, float *hdr_dev,
                             void *stream);
int ipt_adjoint_mat_batch_dev(void *scene, const ipt_params_t *p, int n_scenes, uint64_t seed_stride,
                              const float *kd_dev, const float *ks_dev, const float *ke_dev, const float *adj_dev,
                              double *grad_dev, void *stream);

/* Views: caller-supplied cameras over one loaded scene.
 * Every other entry point looks through the scene's own camera, the
 * reference's constant Camera(CameraParams_t(true)); these render V cameras
 * in one launch and sum ONE material gradient over them.  (Additive symbols:
 * ipt_abi_version stays 5.)
 *
 * ipt_camera_look_at: the reference's camera matrix (scene.h:35-77) with its
 * constants as arguments, in ipt_scene_camera's layout (16 floats, row
 * major); eye 0, look +z, up +y, 90 degrees, aspect 1 gives ipt_scene_camera
 * bit for bit.  As in the reference the eye lands in ROW 3, which rays never
 * read: a ray starts at column 3 of rows 0..2 (out16[3], [7], [11]) and its
 * direction is rows 0..2 times the camera-space direction -- to move a
 * camera, write its position there.
 *
 * ipt_views_create validates n_views matrices once and uploads one device
 * table (a host-only scene: validation only).  Refused with a message, *views
 * = NULL: n_views outside 1..65535, a non-finite entry in rows 0..2, a 3x3
 * part with zero determinant, an origin with a component beyond
 * ipt_scene_camera_bound -- the acceleration structures are exact only for
 * ray origins inside the coordinate bound fixed at load (scene extent and the
 * scene's own camera); they are not rebuilt per view.  A
 * handle belongs to its scene and is freed with ipt_views_free (before or
 * after the scene); a NULL or freed handle is refused by every call. */
int ipt_camera_look_at(const float eye[3], const float look[3], const float up[3], float fov_deg, float aspect,
                       float *out16);
int ipt_scene_camera_bound(void *scene, float *bound);
int ipt_views_create(void *scene, int n_views, const float *cams /* n_views*16 */, void **views);
void ipt_views_free(void *views);
int ipt_views_count(void *views);
/* One launch renders all V views with ONE material set (kd_dev / ks_dev /
 * ke_dev: nT*3 device floats, NULL = the scene's own); view b uses seed
 * p->seed + b*seed_stride and equals ipt_render_mat_dev through its camera
 * bit for bit.  hdr_dev: V*rows*W*3.  max_bounces -1 or 0..62.
 * ipt_adjoint_views_dev: d(sum_b sum adj_b*I_b)/d(Kd, Ks, Ke) -- adj_dev V
 * full frames (V*H*W*3), grad_dev ONE block of 3*nT*3 doubles [Kd | Ks | Ke],
 * ACCUMULATED over the views (zero it first).  Bounded estimator only
 * (max_bounces 0..62); otherwise ipt_adjoint_mat_dev's refusals.  Every
 * refusal happens before anything is enqueued. */
int ipt_render_views_dev(void *scene, void *views, const ipt_params_t *p, uint64_t seed_stride, const float *kd_dev,
                         const float *ks_dev, const float *ke_dev, float *hdr_dev, void *stream);
int ipt_adjoint_views_dev(void *scene, void *views, const ipt_params_t *p, uint64_t seed_stride, const float *kd_dev,
                          const float *ks_dev, const float *ke_dev, const float *adj_dev, double *grad_dev,
                          void *stream);
/* Views x material sets: ONE launch traces n_sets material
 * sets through all V views.  kd_dev / ks_dev / ke_dev: n_sets*nT*3 device
 * floats (NULL = the scene's own values in every set).  Pair (s, b) uses seed
 * p->seed + (s*V + b)*seed_stride and equals view b of ipt_render_views_dev
 * with set s's arrays at that seed, bit for bit.  grad_dev: one [Kd | Ks | Ke]
 * block of 3*nT*3 doubles per set, ACCUMULATED over the set's views (zero it
 * first).  Bounded estimator only, for the pair: max_bounces 0..62.  Refused
 * with a message before anything is enqueued: n_sets < 1, n_sets*V > 65535,
 * max_bounces outside 0..62, more than 65535 triangles, a views handle of
 * another scene (or one not live), an LDS footprint above 160 KiB. */
int ipt_render_views_batch_dev(void *scene, void *views, const ipt_params_t *p, int n_sets, uint64_t seed_stride,
                               const float *kd_dev, const float *ks_dev, const float *ke_dev, /* n_sets*nT*3 or NULL */
                               float *hdr_dev /* [n_sets][V][rows][W][3] */, void *stream);
int ipt_adjoint_views_batch_dev(void *scene, void *views, const ipt_params_t *p, int n_sets, uint64_t seed_stride,
                                const float *kd_dev, const float *ks_dev, const float *ke_dev,
                                const float *adj_dev /* [n_sets][V][H][W][3], full frames */,
                                double *grad_dev /* [n_sets][Kd|Ks|Ke][nT][3], accumulated */, void *stream);
/* The same pair for the reference's own estimator (no bounce cap; DESIGN.md
 * §21): p->max_bounces must be -1.  Layouts, seeds, NULL arrays, the row band
 * and row_step as above; pair (s, b) of the render equals view b of
 * ipt_render_views_dev at -1 bit for bit, and with the scene's own camera as
 * the one view the adjoint equals ipt_adjoint_mat_unbounded_dev's per set.
 * Refused with a message before anything is enqueued: max_bounces >= 0 (the
 * bounded pair above takes 0..62), n_sets < 1, n_sets*V > 65535, more than
 * 65535 triangles, a views handle of another scene (or one not live), bins
 * and tables that leave no room for one record slot per lane in 160 KiB. */
int ipt_render_views_batch_unbounded_dev(void *scene, void *views, const ipt_params_t *p, int n_sets,
                                         uint64_t seed_stride, const float *kd_dev, const float *ks_dev,
                                         const float *ke_dev, /* n_sets*nT*3 or NULL */
                                         float *hdr_dev /* [n_sets][V][rows][W][3] */, void *stream);
int ipt_adjoint_views_batch_unbounded_dev(void *scene, void *views, const ipt_params_t *p, int n_sets,
                                          uint64_t seed_stride, const float *kd_dev, const float *ks_dev,
                                          const float *ke_dev,
                                          const float *adj_dev /* [n_sets][V][H][W][3], full frames */,
                                          double *grad_dev /* [n_sets][Kd|Ks|Ke][nT][3], accumulated */,
                                          void *stream);
/* Host-memory forms with the scene's own materials (synchronous). */
int ipt_render_views_host(void *scene, void *views, const ipt_params_t *p, uint64_t seed_stride,
                          float *hdr /*V*rows*W*3*/);
int ipt_adjoint_views_host(void *scene, void *views, const ipt_params_t *p, uint64_t seed_stride,
                           const float *adj /*V*H*W*3*/, double *grad /*3*nT*3*/);
/* Diagnostic: the camera rays of view `view` for n global sample indices
 * (pixel * spp + sample, pixel row major, each in [0, W*H*spp)), from the
 * trace kernels' own generator and camera code at seed p->seed. */
int ipt_views_rays_host(void *scene, void *views, int view, const ipt_params_t *p, int64_t n,
                        const int64_t *sample_index, float *org /* n*3 */, float *dir /* n*3 */);

/* PNG helpers (RGB8). ipt_png_read with rgb == NULL only reports the size. */
int ipt_png_write(const char *path, int width, int height, const uint8_t *rgb);
int ipt_png_read(const char *path, int *width, int *height, uint8_t *rgb, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif
