// gpu_api.h -- host-callable interface of the HIP side (ipt_hip.hip).
// Plain C++ (no HIP types) so the C-ABI layer compiles without HIP headers.
#pragma once
#include <stdint.h>

#include <string>

#include "../../include/ipt.h"  // IPT_ACCEL_* modes
#include "scene_io.h"

namespace ipt {

struct GpuScene;  // device-resident scene + workspace

GpuScene *gpu_upload(const HostScene &host, std::string *err);
// Host-only handle: no device buffers (export / materials only).
GpuScene *gpu_host_only(const HostScene &host);
bool gpu_on_device(const GpuScene *s);
void gpu_free(GpuScene *s);
const HostScene &gpu_host(const GpuScene *s);
HostScene &gpu_host_mut(GpuScene *s);
int gpu_set_kd(GpuScene *s, const float *kd_host);  // re-upload materials

// All `*_dev` pointers are device pointers; `stream` is a hipStream_t
// (nullptr = the null stream).  kd_dev == nullptr uses the scene's own Kd.
// Return 0 on success, -1 on error (gpu_last_error()).
int gpu_render_samples(GpuScene *s, const RenderParams &p, const float *kd_dev, float *samples_dev,
                       void *stream);
int gpu_pixel_mean(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev,
                   void *stream);
// Same pair over a sample-major buffer [s][pixel][3] (what gpu_render uses).
int gpu_render_samples_sm(GpuScene *s, const RenderParams &p, const float *kd_dev, float *samples_dev,
                          void *stream);
int gpu_pixel_mean_sm(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev,
                      void *stream);
int gpu_render(GpuScene *s, const RenderParams &p, const float *kd_dev, float *hdr_dev, uint8_t *ldr_dev,
               void *stream);
int gpu_adjoint(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *adj_dev,
                double *grad_dev, void *stream);
int gpu_graph(GpuScene *s, const RenderParams &p, const uint8_t *target_dev, double *acc_dev, void *stream);

// Material parameters beyond Kd.  Structure is frozen at load: the emitter
// list and the lobe flags stay, values change; Ke rows of non-emitters and Ks
// rows of lobe-less triangles are forced to 0.  Host arrays nT*3, nullable.
int gpu_set_material_params(GpuScene *s, const float *kd, const float *ks, const float *ke);
// Forward with per-launch overrides (device arrays nT*3; nullptr = the scene's own).
int gpu_render_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                   float *hdr_dev, uint8_t *ldr_dev, void *stream);
// Bounded adjoint in Kd, Ks and Ke: grad_dev is 3 x nT x 3 doubles [Kd | Ks | Ke], accumulated.
// Refuses max_bounces < 0 and the scene batch.
int gpu_adjoint_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                    const float *adj_dev, double *grad_dev, void *stream);
int gpu_adjoint_mat_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad);
// Forward mode of the same estimator: n_tangents directions in material space (tkd / tks / tke, each
// n_tangents x nT x 3 floats, nullptr = zero, at least one given; 1 <= n_tangents <= 16) -> tan_dev,
// n_tangents x band rows x W x 3 doubles, accumulated: tangent image k is the derivative of the HDR mean
// along direction k under the forward's own paths.  One launch of trace_tan_kernel; refuses what
// gpu_adjoint_mat refuses.  The host form takes the scene's own values.
int gpu_tangent_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                    int n_tangents, const float *tkd_dev, const float *tks_dev, const float *tke_dev, double *tan_dev,
                    void *stream);
int gpu_tangent_mat_host(GpuScene *s, const RenderParams &p, int n_tangents, const float *tkd, const float *tks,
                         const float *tke, double *tan);
// The same three blocks for the unbounded estimator (max_bounces < 0; one launch of
// trace_matu_kernel).  Refuses max_bounces >= 0 and the scene batch.
int gpu_adjoint_mat_unbounded(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                              const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream);
int gpu_adjoint_mat_unbounded_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad);
// The scene batch of the two (p.nscenes sets, p.seed_stride): kd / ks / ke are n_scenes*nT*3
// (nullptr = the scene's own values in every set); hdr_dev n_scenes images, grad_dev
// n_scenes x 3 x nT x 3 doubles [set][Kd | Ks | Ke], accumulated.  Set b is the single-set
// call with its arrays and seed + b * seed_stride.  Bounded estimator only.
int gpu_render_mat_batch(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                         const float *ke_dev, float *hdr_dev, void *stream);
int gpu_adjoint_mat_batch(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                          const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream);

// Views: V caller-supplied cameras (ipt_scene_camera's layout, n*16 floats) over one scene, validated
// once and uploaded as one device table (host-only scene: validated only).  nullptr + gpu_last_error()
// when a view is refused.  gpu_camera_bound: the largest admissible |component| of a view's origin.
struct GpuViews;
GpuViews *gpu_views_create(GpuScene *s, int n, const float *cams);
void gpu_views_free(GpuViews *v);
int gpu_views_count(const GpuViews *v);
float gpu_camera_bound(const GpuScene *s);
// One launch over all views with ONE material set (kd / ks / ke nT*3, nullptr = the scene's own); view b
// uses seed + b * p.seed_stride.  hdr_dev: V images; adj_dev: V full frames; grad_dev: ONE 3 x nT x 3
// block [Kd | Ks | Ke], accumulated over the views.  The adjoint is bounded (max_bounces 0..62).
int gpu_render_views(GpuScene *s, const GpuViews *v, RenderParams p, const float *kd_dev, const float *ks_dev,
                     const float *ke_dev, float *hdr_dev, void *stream);
int gpu_adjoint_views(GpuScene *s, const GpuViews *v, RenderParams p, const float *kd_dev, const float *ks_dev,
                      const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream);
// Views x material sets: n_sets material sets (kd / ks / ke n_sets*nT*3, nullptr = the scene's
// own in every set) through every view in one launch; pair (m, b) traces seed + (m*V + b)*seed_stride; hdr_dev
// [n_sets][V] images, grad_dev one [Kd | Ks | Ke] block per set, accumulated.  Bounded (max_bounces 0..62) for both.
int gpu_render_views_batch(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                           const float *ks_dev, const float *ke_dev, float *hdr_dev, void *stream);
int gpu_adjoint_views_batch(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                            const float *ks_dev, const float *ke_dev, const float *adj_dev, double *grad_dev,
                            void *stream);
// The same pair at max_bounces = -1: the forward runs the view sets' forward kernels, the
// adjoint one launch of trace_matu_views_batch_kernel.  Both refuse max_bounces >= 0.
int gpu_render_views_batch_unbounded(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                                     const float *ks_dev, const float *ke_dev, float *hdr_dev, void *stream);
int gpu_adjoint_views_batch_unbounded(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                                      const float *ks_dev, const float *ke_dev, const float *adj_dev,
                                      double *grad_dev, void *stream);
int gpu_render_views_host(GpuScene *s, const GpuViews *v, const RenderParams &p, float *hdr);
int gpu_adjoint_views_host(GpuScene *s, const GpuViews *v, const RenderParams &p, const float *adj, double *grad);
// The camera rays of view `view` for n global sample indices (host arrays; diagnostic).
int gpu_views_rays_host(GpuScene *s, const GpuViews *v, int view, RenderParams p, int64_t n, const int64_t *index,
                        float *org, float *dir);

// Host-memory conveniences (allocate, copy, run, copy back, synchronize).
int gpu_render_samples_host(GpuScene *s, const RenderParams &p, float *samples);
int gpu_render_host(GpuScene *s, const RenderParams &p, float *hdr, uint8_t *ldr);
int gpu_adjoint_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad);
int gpu_graph_host(GpuScene *s, const RenderParams &p, const uint8_t *target, double *acc);

// Acceleration structure (IPT_ACCEL_AUTO / _BRUTE / _BVH) and the one in use.
int gpu_set_accel(GpuScene *s, int mode);
int gpu_accel_in_use(const GpuScene *s);
// Closest hit of n caller-supplied rays (origins, directions: n*3 floats;
// targets: nullable, n ints, >= 0 = shadow ray towards that emitter;
// sources: nullable, n ints, >= 0 = the shadow ray starts on that triangle).
int gpu_closest_hit(GpuScene *s, int64_t n, const float *org_dev, const float *dir_dev, const int *targets_dev,
                    const int *sources_dev, float *t_dev, int *idx_dev, void *stream);
int gpu_closest_hit_host(GpuScene *s, int64_t n, const float *org, const float *dir, const int *targets,
                         const int *sources, float *t, int *idx);

int gpu_device_count();
int gpu_selftest_math(uint64_t n, uint64_t seed, uint64_t *counts);  // 8 mismatch counters
int gpu_debug_last_launch(int32_t *out, int n);  // host-decided numbers of the last trace launch (include/ipt.h)
int gpu_debug_shade_launches();  // trace launches so far that ran a trace_shade_kernel instance
void gpu_debug_fail_launches(int n);  // the next n trace launches fail before their kernel is enqueued
void gpu_debug_adju_ring(int pool_chunks, int lds_slots);  // unbounded adjoint ring sizes (0: default)
const char *gpu_last_error();
void gpu_set_error(const std::string &e);

}  // namespace ipt
