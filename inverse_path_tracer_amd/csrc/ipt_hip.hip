// ipt_hip.hip -- MI355X (gfx950) kernels of the inverse path tracer.
//
// One persistent megakernel traces paths for three integrators that share the
// reference's sampling (template MODE):
//   MODE_FWD    path_trace.cu:111-184  (renderSample/radiance): per-sample
//               radiance to a sample buffer, then pixel_mean_kernel
//               (path_trace.cu:186-198 toneMap) averages it;
//   MODE_ADJ    new: dLoss/dKd of the same estimator under common random
//               numbers (path replay with per-lane vertex records in LDS and
//               a backward sweep when the path ends);
//   MODE_GRAPH  inv_path_trace.cu:109-191 (createGraph): triangle->triangle
//               transport edges accumulated in LDS-privatised fp64 bins.
//
// MI355X-first structure:
//   * one ray per lane, 256-thread workgroups, a grid of exactly the resident
//     workgroups (persistent); each wave owns a contiguous range of global
//     sample indices and refills finished lanes from it with
//     ballot + mbcnt (wave-level compaction, no atomics), so lanes stay busy
//     whatever the path-length spread (the reference's one-thread-per-sample
//     launch idles a wave until its longest path ends);
//   * one loop iteration is one path vertex for the whole wave, in
//     wave-synchronous phases (path cast, shading with all of the vertex's
//     random numbers, shadow cast, emitter term, finish), so each phase --
//     above all the closest-hit loop -- runs once per iteration with most
//     lanes on;
//   * the closest-hit loop walks the triangle table with a wave-uniform
//     index: 80-B records arrive through scalar loads and the test is
//     branch-free per lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "bvh.h"
#include "gpu_api.h"
#include "ipt_device.h"

namespace ipt {

static thread_local std::string g_gpu_err;
void gpu_set_error(const std::string &e) { g_gpu_err = e; }
const char *gpu_last_error() { return g_gpu_err.c_str(); }
// ipt_debug_fail_launches(n): the next n trace launches fail just before
// their kernel is enqueued (after the chunk counters and the launch's scratch
// are allocated) -- the tests' way to check that a failed launch leaves
// nothing behind that a later launch on the stream depends on
static std::atomic<int> g_fail_launches{0};
void gpu_debug_fail_launches(int n) { g_fail_launches.store(n > 0 ? n : 0); }
// ipt_debug_shade_launches(): trace launches since the library was loaded that
// ran a trace_shade_kernel instance (the shading tables in LDS)
static std::atomic<int> g_shade_launches{0};
int gpu_debug_shade_launches() { return g_shade_launches.load(); }
// ipt_debug_last_launch(out, n): the host-decided numbers of the process's
// last trace launch (what IPT_DEBUG_GRID prints, kept in every build) -- the
// tests' way to assert which kernel instance and which LDS layout a scene got.
// Field order: include/ipt.h.  Written under a lock just before the kernel is
// enqueued; word 0 counts the launches recorded since the library was loaded.
constexpr int kLastLaunchFields = 18;
static std::mutex g_last_launch_mu;
static int32_t g_last_launch[kLastLaunchFields] = {0};
int gpu_debug_last_launch(int32_t *out, int n) {
  std::lock_guard<std::mutex> lk(g_last_launch_mu);
  for (int i = 0; i < n && i < kLastLaunchFields; ++i) out[i] = g_last_launch[i];
  return kLastLaunchFields;
}
// ipt_debug_adju_ring(chunks, slots): the unbounded adjoint's pool chunks per
// wave and LDS slots per lane forced small (0: the launch's choice) -- the
// tests' way to run the empty-pool and short-ring paths
static std::atomic<int> g_adju_pool{0}, g_adju_lds{0};
void gpu_debug_adju_ring(int pool_chunks, int lds_slots) {
  g_adju_pool.store(pool_chunks > 0 ? std::min(pool_chunks, 63) : 0);
  g_adju_lds.store(lds_slots > 0 ? lds_slots : 0);
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      gpu_set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                      \
      return -1;                                                                             \
    }                                                                                        \
  } while (0)

// MODE_ADJU: the adjoint of the reference's own estimator (no bounce cap,
// paths end by Russian roulette or a miss, path_trace.cu:172-181).  Vertex
// records live in an LDS ring of rec_cap slots; a path longer than the ring
// is swept in chunks from its end, each earlier chunk re-recorded by
// replaying the path from its camera ray (same seed, same draws, so the same
// floats) -- see trace_kernel.
// MODE_FWDM: MODE_FWD with the pixel mean fused in (gpu_render, TraceArgs::fused).
// MODE_ADJW: MODE_ADJ compiled for 6 waves/SIMD instead of 5 (80 VGPRs), for
// full-size launches (gpu_adjoint: C2 adjoint 1.914 -> 1.862 ms, scenes/0
// 2.316 -> 2.275; a C2 1/8 share is slower with it, 0.307 -> 0.320 ms,
// profiles/r04/variants_chain_adj6_r04l.log, envab_adjw_r04m.log); brute-force diffuse scenes only.
enum { MODE_FWD = 0, MODE_ADJ = 1, MODE_GRAPH = 2, MODE_ADJU = 3, MODE_FWDM = 4, MODE_ADJW = 5 };
template <int MODE>
constexpr bool is_badj() {  // the bounded adjoint (either occupancy)
  return MODE == MODE_ADJ || MODE == MODE_ADJW;
}
template <int MODE>
constexpr bool is_adj() {
  return is_badj<MODE>() || MODE == MODE_ADJU;
}
template <int MODE>
constexpr bool is_fwd() {
  return MODE == MODE_FWD || MODE == MODE_FWDM;
}
constexpr int kBlock = 256;
// Adjoint vertex record (per lane, in LDS): tri | et << 16, the emitter factor
// s (lo = Ke[et] * s is rebuilt bit-identically in the sweep; s = 0 when the
// shadow ray failed), coeff; with a Phong lobe also specd and speci.  The
// prefix throughputs are not recorded (3 more words per vertex cost a wave
// of occupancy and measured slower, profiles/r02_variants_adj_sweep.log):
// the sweep rebuilds them with the forward's own operations.
constexpr int kRecSD = 3;  // specd, then speci
constexpr int kRecFieldsDiffuse = 3;
constexpr int kRecFieldsSpec = kRecFieldsDiffuse + 2;
constexpr int kMaxAdjTris = 65535;  // tri and et share one 32-bit field
constexpr int kEdgeW = 8;      // graph bin: w, w*f, pix[3]*w*f, light[3]*w*f
// LDS form of the graph bins: 5 doubles per (dst, src) (w, w*f, pix[3]*w*f)
// plus 3 light doubles per (dst, emitter) -- only next-event updates, whose
// source is an emitter, touch the light fields.  60 -> 39 KB for scenes/0.txt
// (2 -> 4 workgroups per CU); flushed into the global kEdgeW-wide layout.
constexpr int kEdgeL = 5;
__host__ __device__ inline size_t graph_lds_doubles(int nT, int nE) {
  return (size_t)(nT + 1) * nT * kEdgeL + (size_t)(nT + 1) * (nE > 0 ? nE : 0) * 3;
}
// LDS bins of the material adjoint (trace_mat_kernel), in doubles: the Kd
// slots, as many Ks slots when the instance has the Phong lobe, and 3 per
// emitter for Ke.
__host__ __device__ inline size_t mat_lds_doubles(int grad_slots, int nE, bool spec) {
  return (size_t)grad_slots * 3 * (spec ? 2 : 1) + (size_t)(nE > 0 ? nE : 0) * 3;
}
// LDS tangent tables of the tangent launch (trace_tan_kernel), in doubles (the
// accumulators' place: it has no bins): for scenes with kd tables, ntan x
// (nT x 3 Kd, as many Ks with the Phong lobe, nE x 3 Ke by emitter) floats,
// rounded up to whole doubles; larger scenes read the tangents from global memory.
constexpr int kMaxTangents = 16;
__host__ __device__ inline size_t tan_lds_doubles(int ntan, int nT, int nE, bool spec, bool tables) {
  return tables ? ((size_t)ntan * 3 * ((size_t)nT * (spec ? 2 : 1) + (size_t)(nE > 0 ? nE : 0)) + 1) / 2 : 0;
}
// The unbounded material adjoint's brute-force instances keep the owner
// lane's carried state (Scar, Mlo, the first triangle, the work item) in LDS:
// words per lane, in front of the owner markers (trace_body.h, kCarryLds).
constexpr int kCarryWords = 9;
__host__ __device__ inline size_t mat_carry_bytes(bool bvh) {
  return bvh ? 0 : (size_t)kCarryWords * kBlock * sizeof(uint32_t);
}
constexpr int kMaxAdjBounces = 62;
// ADJU ring slots per lane (3 words each, like ADJ's records: tri | et,
// emitter factor, coeff; the prefix throughputs are rebuilt by the sweep's
// chain from the chunk's first one, Mlo).  Round 3 kept 64 six-word slots
// (with the recorded M_k) per lane in global memory (503 MB at C3 for 327 680
// resident lanes): the records of the live paths overflowed the XCDs' L2s --
// 7.5 GB fetched and 6.7 GB written per C3 launch, 48% L2 hits
// (profiles/r04/unbounded_pmc_r04g.txt) -- and the unbounded adjoint took 1.7x
// the unbounded forward.  Now the first IPT_ADJU_LDS_SLOTS slots of every lane
// are in LDS (a path of up to 8 vertices never touches global memory) and the
// rest of the ring is global, IPT_ADJU_RING = 63 slots in all (round 4: 56
// global slots per lane, 220 MB at C3 for 327 680 resident lanes; now pool
// chunks per wave, below).  The ring's size is what bounds the
// launch's tail: a path longer than the ring replays from its camera ray, and
// the longest paths of a launch (~65 vertices in 16.8 M Russian-roulette
// paths) then run alone at its end -- a 24-slot ring (64 MB) left the average
// wave idle for a quarter of the C3 launch; 63 slots: C3 4.32 -> 4.08 ms,
// Cornell 3.26 -> 3.08, north star 8.21 -> 8.00
// (profiles/r04/variants_adju_rings_r04x.log).  Only the slots a path reaches
// are ever written (the AoS layout below), so the HBM traffic follows the
// path lengths, not the allocation.  Chunks are aligned to the ring: a path of K vertices is swept in chunks
// [j R, min((j+1) R, K)), R = ring slots, the last one straight after the
// first pass (its prefix throughput captured there at vertex j R), every
// earlier one after a replay from the camera ray to its end (K = 30, R = 24:
// 24 replayed vertex traces; a path of K costs about K^2 / 2R, DESIGN.md
// §10.3).  Round 2 kept an 8-slot ring in LDS (24 KB
// per workgroup): every path longer than 8 vertices replayed, C3 unbounded
// adjoint 5.97 ms for a 2.73 ms forward.
#ifndef IPT_ADJU_RING
#define IPT_ADJU_RING 63
#endif
// The ring's global slots come from a pool per wave, in chunks of
// kPoolSlots slots handed out as a lane's path reaches them (a lane holds at
// most kPoolMaxChunks, their ids packed 6 bits each in `ctab`, 63 = none).
// Most lanes never leave the LDS slots (a path of K vertices uses
// ceil((K - rec_lds) / 16) chunks), so a pool of up to 63 chunks
// (TraceArgs::pool_chunks, sized to IPT_ADJU_POOL_MB) serves 64 lanes: 12 KB
// per wave, 62 MB at C3 (5120 resident waves) for the 220 MB of round 4's
// per-lane ring.  A lane that finds the pool empty makes its current slot
// count its ring size for the rest of the path (its chunks stay aligned to it,
// the usual replays follow) -- with 4 LDS slots (the BVH instances) and 32
// chunks that happened to 0.8% of the paths of a q = 0.8 simulation, and the
// north star's unbounded adjoint lost 3%; with 48 or more, never
// (tests/test_adju_protocol.py models the hand-out).
constexpr int kPoolSlots = 16, kPoolMaxChunks = 4;
#ifndef IPT_ADJU_POOL_MB
#define IPT_ADJU_POOL_MB 64
#endif
// LDS ring slots only while the workgroup's LDS stays under this (bytes): at
// equal occupancy (5 blocks/CU) scenes/0's unbounded adjoint ran 4.33 ms with
// 8 slots (32.2 KB) and 4.10 with 6 (26.1 KB), Cornell's 3.26 with 8 (30.0 KB)
// and 3.40 with 6 (profiles/r04/envab_adjulds_r04w.log, _r04x.log)
#ifndef IPT_ADJU_LDS_CAP
#define IPT_ADJU_LDS_CAP (31 * 1024)
#endif
#ifndef IPT_ADJU_LDS_SLOTS
#define IPT_ADJU_LDS_SLOTS 8
#endif
// (BVH instance, at 4 waves/SIMD since round 5: 6 slots -- north-star 6.43
// -> 6.37 ms against 4; 7 loses the fourth workgroup, 7.13 ms;
// profiles/r05/variants_bvh_adju_lds_slots*.log)
#ifndef IPT_ADJU_LDS_SLOTS_BVH
#define IPT_ADJU_LDS_SLOTS_BVH 6
#endif
constexpr int kAdjuRing = IPT_ADJU_RING;
// Sub-chunked sweep of the unbounded adjoint (IPT_ADJU_SUB = G > 0): a chunk
// is swept G vertices at a time from its end, one sub-chunk per loop
// iteration, the lane tracing nothing meanwhile (its suffix carried in Scar,
// as between chunks), so a sweep round's chain runs at most G - 1 steps
// instead of as long as the round's longest path.  The forward's M at every
// G-th slot of a chunk (k > 0) is captured to a per-lane global array
// (TraceArgs::mring, kMrEnt entries), which also replaces the chunk's Mlo
// register.  0: whole chunks per round (round 5).
#ifndef IPT_ADJU_SUB
#define IPT_ADJU_SUB 0
#endif
constexpr int kSub = IPT_ADJU_SUB;
constexpr int kMrEnt = kSub > 0 ? (kAdjuRing + kSub - 1) / kSub : 1;
// Dynamic work distribution across the waves of a launch (TraceArgs::chunk):
// static per-wave ranges left each launch's tail to the waves whose pixels
// hold the longest paths -- C2 forward 2.41 -> 2.11 ms, sphere 6.61 -> 4.63 ms,
// north-star 8.52 -> 5.79 ms, adjoints 1.16-1.63x
// (profiles/r02_variants_dynamic_chunks.log).  IPT_DYN_CHUNKS_PER_WAVE sets
// the chunk size (items per launch / waves / this, a multiple of 64).
#ifndef IPT_DYN_CHUNKS_PER_WAVE
#define IPT_DYN_CHUNKS_PER_WAVE 32
#endif
#ifndef IPT_DYN_MIN_CHUNK
#define IPT_DYN_MIN_CHUNK 128
#endif
constexpr int kMaxTableTris = 512;  // kd/kd-over-pi LDS tables up to 12 KB
// (an LDS table of the emission Ke next to them -- vertex 0's Le, the
// emitter's lo, the sweep's lo -- measured neutral, profiles/r03/variants_ke_ring_r03n.log)
#ifndef IPT_LDS_GRAD_KB
#define IPT_LDS_GRAD_KB 12
#endif
// ADJ gradient bins in LDS (12 KB: all of them up to nT = 512, else the hot
// set).  12 rather than 16 KB lets the BVH adjoint (bins + vertex records +
// tree + group stacks) keep 3 workgroups per CU: sphere scene 16.3 -> 12.1 ms.
constexpr int kLdsGradBytes = IPT_LDS_GRAD_KB * 1024;
// Scenes of at least this many triangles trace through the BVH (auto mode).
// Below it the unrolled / packed brute-force loop wins (a few pairs per cast).
#ifndef IPT_BVH_MIN_TRIS
#define IPT_BVH_MIN_TRIS 64
#endif
constexpr int kBvhMinTris = IPT_BVH_MIN_TRIS;
#ifndef IPT_BVH_LDS_KB
#define IPT_BVH_LDS_KB 32
#endif
constexpr int kBvhLdsNodeBytes = IPT_BVH_LDS_KB * 1024;  // stage the whole tree in LDS up to 512 nodes

struct TraceArgs {
  int W, H, spp, max_bounces;
  uint64_t seed;
  uint64_t n_samples;
  int nT, nE;
  int lds_edges;  // GRAPH: bins privatised in LDS
  int sample_major;  // FWD: sample buffer [s][pixel][3] (else [pixel][s][3])
  int kd_tables;     // kd and kd/pi staged in LDS
  const float *kdpi_g;  // kd/pi in global memory (large scenes: no LDS tables), per launch
  int small_pairs;   // bit 0: nT <= 2*kSmallPairs: unrolled closest-hit, plane offsets in LDS; bit 1 (kSmallShade): the shading tables too
  uint64_t npix;     // pixels of the launch (its rows x W)
  int row0, row_step;  // traced rows: row0, row0 + row_step, ... (row_step 1: a contiguous band)
  // index arithmetic: when every global sample index of the frame is below
  // 2^32, g / spp and pixel / W use Lemire's multiply-high division
  // (M = ceil(2^64 / d), exact for 32-bit n and d > 1) instead of the ~40
  // instruction 64-bit division sequence
  int idx32;
  uint64_t m_spp, m_W, m_npix;
  // BVH (BVH instances only): nodes staged in LDS (0: read from global),
  // traversal stack entries per lane
  int bvh_nbig;                 // large-triangle pairs tested before the traversal
  // cooperative traversal (IPT_BVH_COOP): 8-wide nodes (first bvh_wide_lds of
  // them staged in LDS: all or none), leaf triangles, group-stack entries
  const float4 *bvh_wide;  // WideNode or QWideNode records (kWideF4 float4 each)
  const TriIsect *bvh_wtris;
  int bvh_wide_lds, coop_stride;
  int bvh_big_lds;  // culled path pre-pass: the large pairs' LDS copy is built (launch_bvh_pick chooses)
  float root_box[6];
  float tree_sphere[4];     // bvh.cpp tree_cull
  const float4 *src_cull;   // per triangle {face normal, tau} (ipt_device.h tree_skip)
  const TriPair *bvh_big;
  const int32_t *bvh_big_idx;
  const PairBox2 *bvh_big_boxes;
  // ADJ gradient bins: grad_slots triangles accumulate in LDS fp64 (all of
  // them when they fit, else the largest -- the most-hit -- ones, mapped by
  // grad_map[tri] -> slot or -1, slot_tri[slot] -> tri); the rest go to
  // global fp64 atomics directly
  int grad_slots;
  const int *grad_map;
  const int *slot_tri;
  float cam[16];
  float cam_org[3];
  // per emitter: 1/pmf when pmf is a power of two (then x * (1/pmf) == x / pmf
  // exactly), else 0 -- the emitter term's double division becomes a multiply
  const double *emit_pmfr;  // the camera origin M * (0,0,0,1) with camera_ray's own operations (host, same IEEE ops)
  // 1/spp when spp is a power of two (then x * rc_spp == x / spp for every
  // float x: both are the correctly rounded x * 2^-k), else 0
  float rc_spp;
  float rc_W, rc_H;  // 1/W, 1/H for power-of-two sizes, else 0 (camera_ray divides)
  int rec_cap;   // ADJ: vertex records per lane (max_bounces + 1); ADJU: ring slots
  // ADJU: ring slots 0 .. rec_lds-1 of every lane live in LDS ([field][slot]
  // [lane], like ADJ's records), slots rec_lds .. rec_cap-1 in pool chunks in
  // global memory (grec: grec_stride floats per wave, pool_chunks chunks)
  int rec_lds;
  float *grec;
  uint64_t grec_stride;
  int pool_chunks;  // ADJU: chunks per wave pool (<= 63)
  // ADJU with IPT_ADJU_SUB: per wave [kMrEnt][64 lanes][3] floats, entry e
  // = the forward's M before the update of the vertex in ring slot e * kSub
  float *mring;
  // scene batch (C5): blocks b, b + nscenes, ... (bps of them) trace material
  // set b -- interleaved, not contiguous ranges: the dispatcher fills a CU
  // with consecutive workgroups, so contiguous ranges gave some sets fewer
  // CUs and the launch waited on them (C5 forward 5.77 -> 4.81 ms, adjoint
  // 6.66 -> 5.29 ms, profiles/r02_batch_interleave.log) --
  // kd + b*3nT, seed + b*seed_stride, outputs at b * (out|adj)_stride,
  // gradient at b*3nT -- so each workgroup holds ONE set's tables and bins
  // (the single-scene LDS footprint) and every set is the single-scene
  // launch of its own kd and seed
  int nscenes, bps;
  uint64_t seed_stride, out_stride, adj_stride;
  // dynamic work distribution: a wave starts with chunk `wave` of `chunk`
  // items and then takes chunk nwaves + atomicAdd(ctr[set]) until the launch's
  // items are used up (every launch sets chunk > 0; the kernels still read 0
  // as static per-wave ranges)
  uint32_t chunk;
  // guided sizes: the first chunk_big_n chunks hold `chunk` units, the rest
  // chunk_small (units: work items, or pixels in MODE_FWDM), so a launch ends
  // on small chunks and its waves run dry close together (chunk_range)
  uint32_t chunk_small, chunk_big_n;
  // scene batch with per-set TriMat tables (the material overrides' batch):
  // set b reads mat + b * mat_stride records; 0 = one table for every set.
  // (Here, in what was padding before chunk_ctr: the kernarg layout of every
  // other field is the one the single-set instances were tuned with.)
  uint32_t mat_stride;
  // the launch's grab counters (one word per material set or XCD region).
  // Each wave grabs until one grab fails, so a word ends a launch at
  // `grabs` (launch_grabs: a function of the launch's shape, like the chunk
  // sizes); the wave whose grab returns grabs - 1 zeroes the word.  Each
  // launch on a stream thus starts from zeroed counters in stream order -- no
  // host-side copy of device state, no memset launch per launch, no extra
  // atomic (a count of finished waves cost 2% on the adjoints)
  uint32_t *chunk_ctr;  // word j at chunk_ctr[j * kCtrStride]
  uint32_t grabs;
  // small scenes: acceptance boxes of the pairs (culled shadow casts)
  const PairBox2 *pboxes;
  // small scenes: potential occluders per (source triangle, emitter), nT*nE
  // words (bvh.cpp shadow_occluder_masks), copied to LDS; nullptr = none
  const uint32_t *pomask;
  // BVH scenes: the same masks over the large-triangle pairs (nullptr = none)
  const uint32_t *big_pomask;
  // FWD with the pixel mean fused in (gpu_render): a chunk of
  // `chunk` (then chunk_small) launch-local pixels is issued in groups of
  // `group` pixels x spp samples;
  // each pixel of a group gets one of the wave's nslots LDS slots (spp x 3
  // floats), a finished sample goes to its pixel's slot, and a slot whose
  // last sample is in is summed in sample order (toneMap) into out_samples
  // (HDR, npix x 3) and ldr.  Per wave, at byte mean_off + wave *
  // mean_wstride * 4 of the dynamic LDS: the slots' unfinished counts
  // [nslots], their pixels [nslots], then the slots
  int fused;
  uint32_t group;
  uint32_t mean_off, mean_wstride;
  int nslots;
  uint8_t *ldr;
};
static_assert(alignof(TraceArgs) == 8, "TraceArgs sits right after the ten 8-B scene pointers in the kernarg segment");
static_assert(offsetof(TraceArgs, chunk_ctr) == offsetof(TraceArgs, mat_stride) + sizeof(uint32_t), "mat_stride fills the padding");

__device__ __forceinline__ uint32_t udiv32(uint32_t n, uint64_t m, uint32_t d) {
  return d == 1u ? n : (uint32_t)__umul64hi(m, (uint64_t)n);
}

// Work item w of a launch -> (launch-local pixel lp, sample sj).  Pixel-major:
// w = lp * spp + sj (a wave traces consecutive samples of one pixel).
// Sample-major: w = sj * npix + lp (lane i of a wave writes slot base + i of a
// [s][pixel][3] buffer -- one contiguous store run).
__device__ __forceinline__ void item_split(const TraceArgs &a, uint64_t w, uint64_t &lp, uint64_t &sj) {
  if (a.idx32) {
    if (a.sample_major) {
      const uint32_t q = udiv32((uint32_t)w, a.m_npix, (uint32_t)a.npix);
      sj = q;
      lp = (uint32_t)w - q * (uint32_t)a.npix;
    } else {
      const uint32_t q = udiv32((uint32_t)w, a.m_spp, (uint32_t)a.spp);
      lp = q;
      sj = (uint32_t)w - q * (uint32_t)a.spp;
    }
  } else if (a.sample_major) {
    sj = w / a.npix;
    lp = w - sj * a.npix;
  } else {
    lp = w / (uint64_t)a.spp;
    sj = w - lp * (uint64_t)a.spp;
  }
}
// launch-local pixel -> image row and column
__device__ __forceinline__ void local_rc(const TraceArgs &a, uint64_t lp, int &r, int &c) {
  uint64_t lr;
  if (a.idx32) {
    const uint32_t q = udiv32((uint32_t)lp, a.m_W, (uint32_t)a.W);
    lr = q;
    c = (int)((uint32_t)lp - q * (uint32_t)a.W);
  } else {
    lr = lp / (uint64_t)a.W;
    c = (int)(lp - lr * (uint64_t)a.W);
  }
  r = a.row0 + (int)lr * a.row_step;
}

// Guided chunk sizes for the brute-force instances too (IPT_BF_BIG = the big
// chunks' size in small ones, > 1; see launch_inst): every grab is a
// device-scope atomic, performed at the memory side (the XCDs' L2s are not
// coherent), and the launch's grabs queue there -- C2 adjoint 131 072 -> 77 824
// grabs, 1.816 -> 1.764 ms, the sample-buffer forward 1.629 -> 1.525, scenes/0
// adjoint 2.276 -> 2.243; 3 or 4 (fewer grabs still) lose some of it, and the
// fused render's 256-sample grabs are neutral (profiles/r06/variants_bf_r06c.log,
// variants_ctr_stride_r06e.log)
#ifndef IPT_BF_BIG
#define IPT_BF_BIG 2
#endif
#ifndef IPT_BF_TAIL
#define IPT_BF_TAIL 4
#endif
// The grab counters' spacing in words: the device-scope atomics on one line
// are serialised at the memory side, so each word (material set) gets a
// 128-B line of its own.  Eight words on one line (round 6's XCD bands,
// DESIGN.md §12.2) doubled a C2 1/8 share's adjoint (0.31 -> 0.70 ms), one
// line each: 0.32; the C2 adjoint 1.796 -> 1.768 ms with it
// (profiles/r06/variants_bands_r06d.log, variants_ctr_stride_r06e.log,
// variants_grab_r06h.log)
#ifndef IPT_CTR_STRIDE
#define IPT_CTR_STRIDE 32
#endif
constexpr int kCtrStride = IPT_CTR_STRIDE;
constexpr int kViewFloats = 20;  // floats per entry of the views' table (trace_fwd_views_kernel)
template <bool BVH>
constexpr bool kGuided() {
  return BVH || IPT_BF_BIG > 1;
}
// Chunk g of a launch (TraceArgs::chunk_big_n) -> units [start, end).
// GUIDED: the BVH instances (guided_tail); the others take `chunk` units.
template <bool GUIDED>
__device__ __forceinline__ void chunk_range(const TraceArgs &a, uint64_t g, uint64_t units, uint64_t &start,
                                            uint64_t &end) {
  const uint64_t nb = a.chunk_big_n;
  uint64_t len;
  if (!GUIDED || g < nb) {
    start = g * a.chunk;
    len = a.chunk;
  } else {
    start = nb * a.chunk + (g - nb) * a.chunk_small;
    len = a.chunk_small;
  }
  end = start + len < units ? start + len : units;
}

// The failed grab that returned c: the launch's last grab of that word
// (TraceArgs::grabs) zeroes it.
__device__ __forceinline__ void grab_failed(uint32_t *word, uint32_t c, uint32_t grabs) {
  if (c + 1u == grabs) __hip_atomic_store(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// global pixel index (r * W + c) of this launch's work item w
__device__ __forceinline__ uint64_t item_pixel(const TraceArgs &a, uint64_t w) {
  uint64_t lp, sj;
  item_split(a, w, lp, sj);
  int r, c;
  local_rc(a, lp, r, c);
  if (a.idx32) return (uint32_t)r * (uint32_t)a.W + (uint32_t)c;
  return (uint64_t)r * (uint64_t)a.W + (uint64_t)c;
}

using namespace dev;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// Work item w of a launch -> global sample g, pixel (r, c), XORWOW state
// after the two camera draws and the camera ray (path_trace.cu:150-165); the
// enumeration is described in trace_kernel.
__device__ __forceinline__ void item_ray_ls(const TraceArgs &a, uint64_t seed, uint64_t lp, uint64_t sj, Rng &st, V3 &p,
                                            V3 &d, int &r, int &c) {
  local_rc(a, lp, r, c);
  uint64_t g;  // global sample index
  if (a.idx32) {  // every index of the frame fits 32 bits: one 32x32->64 multiply-add
    const uint32_t pixel = (uint32_t)r * (uint32_t)a.W + (uint32_t)c;
    g = (uint64_t)pixel * (uint32_t)a.spp + sj;
  } else {
    g = ((uint64_t)r * (uint64_t)a.W + (uint64_t)c) * (uint64_t)a.spp + sj;
  }
  rng_init(st, seed + g);
  camera_ray(a.cam, a.cam_org, st, r, c, a.W, a.H, a.rc_W, a.rc_H, p, d);
}
__device__ __forceinline__ void item_ray(const TraceArgs &a, uint64_t seed, uint64_t w, Rng &st, V3 &p, V3 &d, int &r,
                                         int &c) {
  uint64_t lp, sj;
  item_split(a, w, lp, sj);
  item_ray_ls(a, seed, lp, sj, st, p, d, r, c);
}

// The fused forward's brute-force instances (MODE_FWDM && !BVH) give a lane
// whose path has just ended its next sample inside the shading phase, where
// the continuing lanes sample their next direction: draws, rotation and
// unit() then run once for both groups, and the refill at the loop top is
// entered only at group boundaries.  With it the pixel part
// of item_ray_ls is evaluated once per group of pixels, not per sample.
template <int MODE, bool BVH>
constexpr bool kInphase() {
  return MODE == MODE_FWDM && !BVH;
}
// Small scenes' shading data -- normals, sampling frames, Ke, the emitters'
// vertices, CDF and pmf -- read from the packed LDS records of scene_layout.h
// instead of per-lane global loads of TriGeom, TriMat and the emitter arrays
// (trace_shade_kernel).
constexpr int kSmallShade = 2;  // TraceArgs::small_pairs bit 1: the launch carries the shading tables
// Words per pixel of a group's entry table: seed + pixel * spp (lo, hi),
// (float)c, (float)r -- item_ray_ls's pixel part; a sample adds its index s.
constexpr int kEntryWords = 4;
static inline uint32_t fused_entry_words(uint32_t group, bool bvh) {
  return !bvh ? kEntryWords * group : 0u;
}
__device__ __forceinline__ void pixel_entry(const TraceArgs &a, uint64_t seed, uint64_t lp, uint32_t e[kEntryWords]) {
  int r, c;
  local_rc(a, lp, r, c);
  uint64_t g0;  // the pixel's first global sample index
  if (a.idx32) {
    const uint32_t pixel = (uint32_t)r * (uint32_t)a.W + (uint32_t)c;
    g0 = (uint64_t)pixel * (uint32_t)a.spp;
  } else {
    g0 = ((uint64_t)r * (uint64_t)a.W + (uint64_t)c) * (uint64_t)a.spp;
  }
  g0 += seed;
  e[0] = (uint32_t)g0;
  e[1] = (uint32_t)(g0 >> 32);
  e[2] = __float_as_uint((float)c);
  e[3] = __float_as_uint((float)r);
}

// ---------------------------------------------------------------------------
// Minimum resident 256-thread blocks per CU (= waves per SIMD) requested per
// integrator; 0 lets the compiler choose.  Round 1 measured 6 best (80 VGPRs,
// 20 B of cold spill); with the dynamic chunks, the culled shadow cast and
// the batch fields the 80-VGPR build spills 72-76 B per lane inside the loop
// and 5 (96 VGPRs, 12-20 B) wins: C2 forward 2.11 -> 1.98 ms, adjoint 2.49 ->
// 2.41, scenes/0 2.66 -> 2.53 / 2.98 -> 2.95; 4 (108-115 VGPRs, no spill)
// loses (profiles/r02_variants_occupancy.log).
#ifndef IPT_MIN_BLOCKS_FWD
#define IPT_MIN_BLOCKS_FWD 5
#endif
#ifndef IPT_MIN_BLOCKS_ADJ
#define IPT_MIN_BLOCKS_ADJ 5
#endif
#ifndef IPT_MIN_BLOCKS_ADJU
#define IPT_MIN_BLOCKS_ADJU 5
#endif
#ifndef IPT_MIN_BLOCKS_ADJW
#define IPT_MIN_BLOCKS_ADJW 6
#endif
#ifndef IPT_MIN_BLOCKS_GRAPH
#define IPT_MIN_BLOCKS_GRAPH 0
#endif
// The BVH instances hold the traversal state on top (slab parameters, stack
// pointer, node) and their LDS (node copy + stack) caps residency anyway:
// 4 waves/SIMD, 128 VGPRs, no spill.
#ifndef IPT_MIN_BLOCKS_BVH
#define IPT_MIN_BLOCKS_BVH 4
#endif
// The adjoint's BVH instance: its LDS (gradient bins + vertex records + tree
// + group stacks, ~55 KB for the sphere scene) allows only 2 workgroups per
// CU, i.e. 2 waves/SIMD, so it may use up to 256 VGPRs without losing
// residency (at 4 waves/SIMD it spilled).
#ifndef IPT_MIN_BLOCKS_BVH_ADJ
#define IPT_MIN_BLOCKS_BVH_ADJ 2
#endif
// The unbounded adjoint's BVH instance: its LDS (4 ring slots, the gradient
// hot set, the tree stage) leaves room for 4 workgroups per CU, and at 131
// VGPRs it ran 3 waves/SIMD; held to 128 (4 waves) it spills nothing and the
// north-star unbounded adjoint runs 7.08 -> 6.4x ms.
#ifndef IPT_MIN_BLOCKS_BVH_ADJU
#define IPT_MIN_BLOCKS_BVH_ADJU 4
#endif
// The forward's BVH instance at 5 waves/SIMD (96 VGPRs, ~116 B of spill,
// mostly outside the casts) beats 4 (121 VGPRs, none): sphere scene 9.92 ->
// 9.48 ms (profiles/r01_variants_bvh_occupancy.log); 6 spills in the
// traversal and loses (14.5 ms).
#ifndef IPT_MIN_BLOCKS_BVH_FWD
#define IPT_MIN_BLOCKS_BVH_FWD 5
#endif
template <int MODE, bool BVH>
constexpr int min_blocks() {
  return BVH ? (MODE == MODE_ADJU ? IPT_MIN_BLOCKS_BVH_ADJU
                                  : (is_adj<MODE>() ? IPT_MIN_BLOCKS_BVH_ADJ
                                                    : (is_fwd<MODE>() ? IPT_MIN_BLOCKS_BVH_FWD : IPT_MIN_BLOCKS_BVH)))
             : (is_fwd<MODE>() ? IPT_MIN_BLOCKS_FWD
                                : (MODE == MODE_ADJU   ? IPT_MIN_BLOCKS_ADJU
                                   : MODE == MODE_ADJW ? IPT_MIN_BLOCKS_ADJW
                                                       : (is_adj<MODE>() ? IPT_MIN_BLOCKS_ADJ : IPT_MIN_BLOCKS_GRAPH)));
}
// Rejected and removed (round 3; the A/B logs under profiles/ keep the
// evidence): a traversal-server wave per workgroup fed through an LDS ray
// queue (r01_bvh_server.log: 21.0 vs 13.3 ms), the one-lane-per-ray binary
// traversal (r01_variants_coop_notrav.log), the per-lane backward sweep
// (r02_variants_adj_knobs_final.log: 7% slower), recorded prefix throughputs
// (r02_variants_adj_sweep.log), quantised wide nodes (r02_variants_qnodes.log),
// the forward's camera-ray ring (r02_variants_occupancy_after_cull.log), the
// shadow target tested with its pair partner (r02_variants_shadow_target_pair.log)
// the tolerance-mode fast cast (r02_variants_fastcast.log: fails the
// 1e-3 gradient bar), a per-wave LDS queue that parked the forward's path
// rays with their path state until a full cooperative round of 8 was waiting
// (r03/variants_queue_chsweep_r03f.log: north-star forward 4.70 vs 3.75 ms;
// r03/variants_r03e.log for the first form, 4.30 ms) and a channel-split
// adjoint sweep, lane 3i + c walking path i in channel c (same log: C2
// adjoint 2.33 vs 2.16 ms, north-star 6.57 vs 5.02 ms at one wave less);
// round 5: the four waves of a workgroup pooling their tree rays in an LDS
// queue and sharing out full rounds of 8 (two barriers per cast, the waves in
// step): north-star forward 3.71 -> 4.25 ms, unbounded adjoint 8.06 -> 13.6 --
// the lockstep waits cost more than the fuller rounds save
// (profiles/r05/variants_coop_wg_r05i.log, _r05j.log).
// Graph bins stay in LDS up to this size (KB), else global fp64 atomics.
#ifndef IPT_GRAPH_LDS_KB
#define IPT_GRAPH_LDS_KB 64
#endif
// Work enumeration of the adjoint and graph integrators.  Round 1 chose
// sample-major (a wave's 64 lanes trace 64 different pixels, so the LDS
// atomics of a vertex step hit different bins and few lanes need the BVH tree
// at once: C2 adjoint 3.29 -> 3.24 ms, sphere 23.8 -> 16.3 ms,
// profiles/r01_variants_adj_sample_major.log).  Since the culled casts and the
// wave-parallel sweep, pixel-major is the faster adjoint (a wave's coherent
// rays skip more pair blocks; C2 1.747 -> 1.734 ms, scenes/0 unbounded
// 3.554 -> 3.502, north star 3.905 -> 3.835, profiles/r06/variants_adj_enumeration_r06t.log)
// and each pixel's adjoint value is fetched by one chunk, i.e. one XCD's L2
// (DESIGN.md §12.10).  adjoint_args and gpu_graph clear
// TraceArgs::sample_major; only the forward's sample buffer sets it.
#define IPT_TRACE_BOUNDS __attribute__((amdgpu_flat_work_group_size(1, kBlock), amdgpu_waves_per_eu(min_blocks<MODE, BVH>() ? min_blocks<MODE, BVH>() : 1)))
// Profiling-only build (make variant DEFS=-DIPT_PHASE_TIMING): each wave
// accumulates s_memtime cycles per phase of the loop; read with
// ipt_debug_phase_cycles (tools/phase_timing.py).
#ifdef IPT_PHASE_TIMING
constexpr int kPhaseWords = 26;
__device__ unsigned long long g_phase_cycles[kPhaseWords];
// [8], [9]: the tree (coop_cast) part of phases 1 and 3 (BVH scenes);
// [10..21]: per phase, the lanes that take part summed over the wave
// iterations that run it, and those iterations (PHASE_LANES): refill,
// shade, shadow cast, emitter term, finalise, adjoint sweep rounds (valid
// tasks per round); [22] the sweep's chain steps (wave-level), [23] the
// rounds that run a chain, [24] the lanes' own chain steps summed (the
// useful part of [22] x 64); the path cast's lanes are [7]
#define PHASE_LANES(i, cond)                             \
  {                                                      \
    const uint64_t b_ = __ballot(cond);                  \
    if (b_) {                                            \
      tacc[i] += (uint64_t)__popcll(b_);                 \
      tacc[(i) + 1] += 1;                                \
    }                                                    \
  }
#define SUBPHASE_BEGIN const uint64_t ts_ = __builtin_amdgcn_s_memtime();
#define SUBPHASE_END(i) tacc[i] += __builtin_amdgcn_s_memtime() - ts_;
#define PHASE(i)                                     \
  {                                                  \
    const uint64_t tn_ = __builtin_amdgcn_s_memtime(); \
    tacc[i] += tn_ - tp_;                            \
    tp_ = tn_;                                       \
  }
#else
#define PHASE(i)
#define SUBPHASE_BEGIN
#define SUBPHASE_END(i)
#define PHASE_LANES(i, cond)
#endif

// Path ray of the brute-force scenes: the unrolled pair loop with plane
// offsets from LDS (nT <= 2 * kSmallPairs), else the packed pair loop.
__device__ __forceinline__ int cast_bf(const TriPair *__restrict__ pairs, const f2 *e3, int nT, V3 p, V3 d, float &t) {
  if (e3) return closest_hit_pairs_small(pairs, e3, nT, p, d, t);
  return closest_hit_pairs(pairs, nT, p, d, t);
}

// Entry i of the small-scene LDS table (kE3Floats per pair): the three
// edge-plane offsets of the pair as (A, B) float pairs.
__device__ __forceinline__ float small_table_entry(const TriPair *__restrict__ pairs, int i) {
  const int j = i / kE3Floats, k = i % kE3Floats, h = k & 1;
  return pairs[j].f[9 + 4 * (k >> 1)][h];
}

// LDS carve-out of the BVH instances (16-B aligned): wide nodes, large-pair
// copies, emitter records, group stacks.
__host__ __device__ inline size_t bvh_lds_offset(size_t base) { return (base + 15) & ~(size_t)15; }
// Bytes of the culled path pre-pass's LDS copy of the large pairs (16-B
// aligned, 36 floats per pair) and their original indices (2 ints per pair).
// The emitters' TriIsect records for the BVH shadow target test (nE <= 16).
constexpr int kEmitLdsMax = 16;
__host__ __device__ inline size_t emit_lds_bytes(int nE) {
  return nE > 0 && nE <= kEmitLdsMax ? (size_t)nE * sizeof(TriIsect) : 0;
}
__host__ __device__ inline size_t big_lds_bytes(int nbig) {
  return nbig > 0 ? 12 + (size_t)nbig * (sizeof(TriPair) + 2 * sizeof(int32_t)) : 0;
}
// Fill that copy at `at` (rounded up to 16 B from the LDS base); returns the
// first float after it.
__device__ __forceinline__ float *big_lds_copy(const TraceArgs &a, float *at, float *base, int tid, int nthr,
                                               BvhView &bv) {
  if (!(a.bvh_nbig > 0 && a.bvh_big_lds)) return at;
  float *pl = at + ((4 - (int)((at - base) & 3)) & 3);
  const float *g = reinterpret_cast<const float *>(a.bvh_big);
  for (int i = tid; i < 36 * a.bvh_nbig; i += nthr) pl[i] = g[i];
  int32_t *il = reinterpret_cast<int32_t *>(pl + 36 * a.bvh_nbig);
  for (int i = tid; i < 2 * a.bvh_nbig; i += nthr) il[i] = a.bvh_big_idx[i];
  bv.big_lds = pl;
  return at + big_lds_bytes(a.bvh_nbig) / sizeof(float);
}

// Wave-wide inclusive scans (GFX9 DPP: row_shr 1..8 inside each 16-lane
// row, then row_bcast:15 / row_bcast:31 carry the rows' totals; lanes a
// stage does not write add / max the identity 0).
// The adjoint sweep's task scan and owner search use them (an LDS scatter of
// owner markers + a max-scan) instead of six dependent ds_bpermute steps
// each: C2 adjoint 2.11 -> 2.05 ms, scenes/0 2.53 -> 2.47, north-star 4.96 ->
// 4.88 (profiles/r03/variants_ke_ring_r03n.log, `scan0`).
template <int CTRL, int ROW, int BANK>
__device__ __forceinline__ int dpp0(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW, BANK, true);
}
__device__ __forceinline__ int wave_scan_add(int v) {
  int s = v + dpp0<0x111, 0xf, 0xf>(v);
  s += dpp0<0x112, 0xf, 0xf>(v);
  s += dpp0<0x113, 0xf, 0xf>(v);
  s += dpp0<0x114, 0xf, 0xe>(s);
  s += dpp0<0x118, 0xf, 0xc>(s);
  s += dpp0<0x142, 0xa, 0xf>(s);
  s += dpp0<0x143, 0xc, 0xf>(s);
  return s;
}
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t v) {
  v = max(v, (uint32_t)dpp0<0x111, 0xf, 0xf>((int)v));
  v = max(v, (uint32_t)dpp0<0x112, 0xf, 0xf>((int)v));
  v = max(v, (uint32_t)dpp0<0x114, 0xf, 0xf>((int)v));
  v = max(v, (uint32_t)dpp0<0x118, 0xf, 0xf>((int)v));
  v = max(v, (uint32_t)dpp0<0x142, 0xa, 0xf>((int)v));
  v = max(v, (uint32_t)dpp0<0x143, 0xc, 0xf>((int)v));
  return v;
}

// TraceArgs is the kernel's FIRST parameter, so it sits at offset 0 of the
// kernarg segment -- the in-loop reload below depends on that (IPT_ARGS_RELOAD).
// The explicit arguments of trace_kernel as the kernarg segment holds them
// (in order, each at its natural alignment): karg() re-reads one of them at
// its point of use.  The adjoint's adj / grad pointers are used only by the
// sweep and the final flush; kept live across the loop they sit in SGPRs
// the pair loops need, and the compiler spills them to VGPR lanes and reloads
// them (v_readlane, VALU work) after every pair block.
struct TraceKernArgs {
  TraceArgs a;
  const TriIsect *isect;
  const TriPair *pairs;
  const TriGeom *geom;
  const TriMat *mat;
  const float *kd;
  const int *emit_tri;
  const float *emit_cdf;
  const float *emit_pmf;
  float *out_samples;
  const float *adj;
  double *grad;
  const uint8_t *target;
  double *edges;
};
static_assert(offsetof(TraceKernArgs, isect) == sizeof(TraceArgs), "pointers follow TraceArgs");
template <typename T>
__device__ __forceinline__ T karg(size_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(4))) const char cst_char;
  typedef __attribute__((address_space(4))) const T cst_t;
  const cst_char *k = (const cst_char *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));  // read here, not hoisted to the kernel's entry
  return *(const cst_t *)(k + off);
#else
  (void)off;
  return T();
#endif
}
// The kernels' body is trace_body.h, included as text inside each __global__
// entry point (trace_kernel's 21 instances compile exactly as they did with
// the body written here).
template <int MODE, bool SPEC, bool BVH>
__global__ IPT_TRACE_BOUNDS void trace_kernel(
    const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
    const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
    const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
    float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
    const uint8_t *__restrict__ target, double *__restrict__ edges) {
  constexpr bool MATG = false;
  constexpr bool MATB = false;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
  const int *const tri_emit = nullptr;
#include "trace_body.h"
}

// Small scenes (nT <= 32, 0 < nE <= 16): trace_kernel's brute-force forwards
// and bounded adjoints reading the shading tables of scene_layout.h from LDS
// (SHADE).  Instances of their own: with both reads in one body
// behind a wave-uniform branch, the launches that took the old reads ran
// 1.5-2% slower than before (the branch's SGPRs and code), which is what the
// tables gain.  trace_kernel's instances stay what they were.
template <int MODE, bool SPEC, bool BVH>
__global__ IPT_TRACE_BOUNDS void trace_shade_kernel(
    const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
    const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
    const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
    float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
    const uint8_t *__restrict__ target, double *__restrict__ edges) {
  static_assert(!BVH, "the shading tables serve the brute-force instances");
  constexpr bool MATG = false;
  constexpr bool MATB = false;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = true;
  constexpr bool TANG = false;
  const int *const tri_emit = nullptr;
#include "trace_body.h"
}

// The forward of a scene batch whose sets have their own TriMat tables (the
// material overrides' batch): trace_kernel's forward instances
// with mat offset per set (MATB).  Instances of their own, because that one
// offset inside trace_kernel's body moved the register allocation and the
// schedule of the tuned single-set forwards (the C2 headline +0.10%, three
// sessions alike); so trace_kernel's 21 instances stay what they were.
template <int MODE, bool SPEC, bool BVH>
__global__ IPT_TRACE_BOUNDS void trace_fwd_mat_kernel(
    const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
    const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
    const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
    float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
    const uint8_t *__restrict__ target, double *__restrict__ edges) {
  static_assert(is_fwd<MODE>(), "forward instances only");
  constexpr bool MATG = false;
  constexpr bool MATB = true;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
  const int *const tri_emit = nullptr;
#include "trace_body.h"
}

// The material adjoint: the bounded adjoint's tracing and records, its sweep
// also emitting dL/dKs and dL/dKe (grad: 3 x nT x 3 doubles, [Kd | Ks | Ke]).
// Same leading parameters as trace_kernel (karg() reads adj and grad by their
// TraceKernArgs offsets); tri_emit follows them.
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJ, BVH>()))) void
trace_mat_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                 const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
                 const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf,
                 const float *__restrict__ emit_pmf, float *__restrict__ out_samples, const float *__restrict__ adj,
                 double *__restrict__ grad, const uint8_t *__restrict__ target, double *__restrict__ edges,
                 const int *__restrict__ tri_emit) {
  constexpr int MODE = MODE_ADJ;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
#include "trace_body.h"
}

// The unbounded material adjoint: MODE_ADJU's tracing, ring
// and replays with the material sweep.  Its owner lanes carry the path's first
// triangle across replays (trace_body.h, kTri0Carry).  A __global__ of its
// own, so trace_kernel's and trace_mat_kernel's instances stay what they were;
// bounds as the unbounded adjoint's.
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJU, BVH>()))) void
trace_matu_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                  const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
                  const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf,
                  const float *__restrict__ emit_pmf, float *__restrict__ out_samples, const float *__restrict__ adj,
                  double *__restrict__ grad, const uint8_t *__restrict__ target, double *__restrict__ edges,
                  const int *__restrict__ tri_emit) {
  constexpr int MODE = MODE_ADJU;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
#include "trace_body.h"
}

// Views: the scene batch's grid split with the sets being V
// cameras over ONE material set.  Set b renders with seed + b * seed_stride
// into out + b * out_stride (the adjoint reads adj + b * H*W*3), but kd, mat,
// kd/pi and the gradient carry no per-set offset, and the camera is entry b
// of the views' table -- kViewFloats floats per view: the 16 of the matrix,
// the origin's 3 (make_args' fmaf chain, evaluated at ipt_views_create), one
// of padding (16-B entries).  The table is the TRAILING parameter: TraceArgs
// and the leading parameters keep their kernarg offsets, and the shipped
// instances their code.  __global__s of their own for the same reason.
template <int MODE, bool SPEC, bool BVH>
__global__ IPT_TRACE_BOUNDS void trace_fwd_views_kernel(
    const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
    const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
    const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
    float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
    const uint8_t *__restrict__ target, double *__restrict__ edges, const float *__restrict__ views) {
  static_assert(is_fwd<MODE>(), "forward instances only");
  constexpr bool MATG = false;
  constexpr bool MATB = false;
  constexpr bool VIEWS = true;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
  const int *const tri_emit = nullptr;
#include "trace_body.h"
}
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJ, BVH>()))) void
trace_mat_views_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                       const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat,
                       const float *__restrict__ kd, const int *__restrict__ emit_tri,
                       const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
                       float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
                       const uint8_t *__restrict__ target, double *__restrict__ edges,
                       const int *__restrict__ tri_emit, const float *__restrict__ views) {
  constexpr int MODE = MODE_ADJ;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = true;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
#include "trace_body.h"
}

// Views x material sets: the views' grid split over S * V
// (set, view) pairs.  Launch set i traces material set i / V through camera
// i % V: seed, image, adjoint image, grab counter and bps go by i as in every
// batch, kd, mat, kd/pi and the gradient slice by i / V, the camera by i % V.
// V follows the views' table as one more TRAILING parameter (TraceArgs keeps
// its layout).  __global__s of their own, so the view kernels stay what they
// were.
template <int MODE, bool SPEC, bool BVH>
__global__ IPT_TRACE_BOUNDS void trace_fwd_views_batch_kernel(
    const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
    const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
    const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
    float *__restrict__ out_samples, const float *__restrict__ adj, double *__restrict__ grad,
    const uint8_t *__restrict__ target, double *__restrict__ edges, const float *__restrict__ views,
    const int nviews) {
  static_assert(is_fwd<MODE>(), "forward instances only");
  constexpr bool MATG = false;
  constexpr bool MATB = false;
  constexpr bool VIEWS = true;
  constexpr bool VSETS = true;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
  const int *const tri_emit = nullptr;
#include "trace_body.h"
}
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJ, BVH>()))) void
trace_mat_views_batch_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                             const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat,
                             const float *__restrict__ kd, const int *__restrict__ emit_tri,
                             const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
                             float *__restrict__ out_samples, const float *__restrict__ adj,
                             double *__restrict__ grad, const uint8_t *__restrict__ target,
                             double *__restrict__ edges, const int *__restrict__ tri_emit,
                             const float *__restrict__ views, const int nviews) {
  constexpr int MODE = MODE_ADJ;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = true;
  constexpr bool VSETS = true;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
#include "trace_body.h"
}

// The unbounded material adjoint over (material set, view) pairs (DESIGN.md
// §21): trace_matu_kernel's ring, replays and carried words with the view
// sets' keying -- seed, adjoint image and grab counter by the launch set, kd,
// mat, kd/pi and the gradient slice by the material set, the camera (the
// replays' too: they restart through the loop's own copy of the arguments) by
// the view.  Bounds as trace_matu_kernel's, trailing parameters as
// trace_mat_views_batch_kernel's.  A __global__ of its own, named so that no
// count of the other families by prefix sees it.
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJU, BVH>()))) void
trace_matu_views_batch_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                              const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat,
                              const float *__restrict__ kd, const int *__restrict__ emit_tri,
                              const float *__restrict__ emit_cdf, const float *__restrict__ emit_pmf,
                              float *__restrict__ out_samples, const float *__restrict__ adj,
                              double *__restrict__ grad, const uint8_t *__restrict__ target,
                              double *__restrict__ edges, const int *__restrict__ tri_emit,
                              const float *__restrict__ views, const int nviews) {
  constexpr int MODE = MODE_ADJU;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = true;
  constexpr bool VSETS = true;
  constexpr bool SHADE = false;
  constexpr bool TANG = false;
#include "trace_body.h"
}

// Forward-mode material derivatives: trace_mat_kernel's
// tracing, records, chains and fp32 terms; the sweep's last step multiplies
// each term by the tangents' entry for the bin the adjoint would have added it
// to and sums per pixel.  No adjoint image (the weights are 1/spp) and no bins:
// `grad` is the tangent images, ntan x npix x 3 doubles, accumulated.  The
// tangents (ntan x nT x 3 floats each, nullptr: zero) follow tri_emit, read by
// their kernarg offsets (TanKernArgs).  A __global__ of its own, named so that
// no count of the other families by prefix sees it.
template <bool SPEC, bool BVH>
__global__ __attribute__((amdgpu_flat_work_group_size(1, kBlock),
                          amdgpu_waves_per_eu(min_blocks<MODE_ADJ, BVH>()))) void
trace_tan_kernel(const TraceArgs a, const TriIsect *__restrict__ isect, const TriPair *__restrict__ pairs,
                 const TriGeom *__restrict__ geom, const TriMat *__restrict__ mat, const float *__restrict__ kd,
                 const int *__restrict__ emit_tri, const float *__restrict__ emit_cdf,
                 const float *__restrict__ emit_pmf, float *__restrict__ out_samples, const float *__restrict__ adj,
                 double *__restrict__ grad, const uint8_t *__restrict__ target, double *__restrict__ edges,
                 const int *__restrict__ tri_emit, const float *__restrict__ tkd_arg, const float *__restrict__ tks_arg,
                 const float *__restrict__ tke_arg, const int ntan_arg) {
  constexpr int MODE = MODE_ADJ;
  constexpr bool MATG = true;
  constexpr bool MATB = false;
  constexpr bool VIEWS = false;
  constexpr bool VSETS = false;
  constexpr bool SHADE = false;
  constexpr bool TANG = true;
#include "trace_body.h"
}

// The diagnostic of ipt_views_rays_host: the megakernel's own rng_init and
// camera_ray for caller-chosen global sample indices g (pixel = g / spp, row
// major) of view `view`, written out as rays.
__global__ __launch_bounds__(kBlock) void view_rays_kernel(const float *__restrict__ views, int view, int W, int H,
                                                           int spp, float rcW, float rcH, uint64_t seed, int64_t n,
                                                           const int64_t *__restrict__ index,
                                                           float *__restrict__ org, float *__restrict__ dir) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = (uint64_t)index[i], pixel = g / (uint64_t)spp;
  const float *cam = views + (size_t)view * kViewFloats;
  Rng st;
  rng_init(st, seed + g);
  V3 p, d;
  camera_ray(cam, cam + 16, st, (int)(pixel / (uint64_t)W), (int)(pixel % (uint64_t)W), W, H, rcW, rcH, p, d);
  org[3 * i] = p.x, org[3 * i + 1] = p.y, org[3 * i + 2] = p.z;
  dir[3 * i] = d.x, dir[3 * i + 1] = d.y, dir[3 * i + 2] = d.z;
}

// Per-launch TriMat tables of the material overrides (stream scratch): the
// scene's entries with ks / ke replaced from nT*3 device arrays (nullptr: the
// scene's own); flags and shininess are kept, and rows outside the lobe /
// emitter masks fixed at load are forced to 0.  Scene batch: blockIdx.y =
// material set, ks / ke [set][tri][c], one table of nT records per set.
__global__ __launch_bounds__(kBlock) void pack_mat_kernel(const TriMat *__restrict__ src, const float *__restrict__ ks,
                                                          const float *__restrict__ ke,
                                                          const int *__restrict__ tri_emit, int nT,
                                                          TriMat *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= nT) return;
  const size_t row = (size_t)blockIdx.y * (size_t)nT + (size_t)i;
  TriMat m = src[i];
  if (ks) {
    const bool lobe = (m.flags & MAT_HAS_KS) != 0;
    for (int c = 0; c < 3; ++c) m.ks[c] = lobe ? ks[3 * row + c] : 0.f;
  }
  if (ke) {
    const bool em = tri_emit[i] >= 0;
    for (int c = 0; c < 3; ++c) m.ke[c] = em ? ke[3 * row + c] : 0.f;
  }
  out[row] = m;
}

// out[i] = src[i % n], i < total: the scene's own kd for every set of a batch
// whose caller gave none (the kernels read kd + set * 3 nT).
__global__ __launch_bounds__(kBlock) void replicate_kernel(const float *__restrict__ src, int n, size_t total,
                                                           float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < total) out[i] = src[i % (size_t)n];
}

// toneMap over a sample-major buffer [s][pixel][3]: same per-pixel
// sequential sum, but lane l reads pixel base+l, so every load of a wave is
// one contiguous 768-byte run (the pixel-major form below strides 12*spp B).
__global__ __launch_bounds__(kBlock) void pixel_mean_sm_kernel(const float *__restrict__ samples, int64_t npix,
                                                               int spp, float *__restrict__ hdr,
                                                               uint8_t *__restrict__ ldr) {
  const int64_t px = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  // scene batch: blockIdx.y = material set, each with its own [s][pixel][3] buffer and image
  samples += (size_t)blockIdx.y * (size_t)npix * spp * 3;
  hdr += (size_t)blockIdx.y * (size_t)npix * 3;
  if (ldr) ldr += (size_t)blockIdx.y * (size_t)npix * 3;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  const float fs = (float)spp;
  if ((spp & (spp - 1)) == 0 && spp <= (1 << 24)) {
    // x / spp == x * (1/spp) for a power of two (both the correctly rounded
    // x * 2^-k); the loads of 16 samples are issued before their sums (the
    // kernel is latency-bound: one pixel per thread, spp dependent adds)
    const float rc = 1.0f / fs;
    int i = 0;
    for (; i + 16 <= spp; i += 16) {
      float v[48];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float *s = samples + ((int64_t)(i + u) * npix + px) * 3;
        v[3 * u] = s[0];
        v[3 * u + 1] = s[1];
        v[3 * u + 2] = s[2];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        tx += v[3 * u] * rc;
        ty += v[3 * u + 1] * rc;
        tz += v[3 * u + 2] * rc;
      }
    }
    for (; i < spp; ++i) {
      const float *s = samples + ((int64_t)i * npix + px) * 3;
      tx += s[0] * rc;
      ty += s[1] * rc;
      tz += s[2] * rc;
    }
  } else {
    for (int i = 0; i < spp; ++i) {
      const float *s = samples + ((int64_t)i * npix + px) * 3;
      tx += s[0] / fs;
      ty += s[1] / fs;
      tz += s[2] / fs;
    }
  }
  hdr[px * 3] = tx;
  hdr[px * 3 + 1] = ty;
  hdr[px * 3 + 2] = tz;
  if (ldr) {
    ldr[px * 3] = (uint8_t)(255.f * tx / (1 + tx));
    ldr[px * 3 + 1] = (uint8_t)(255.f * ty / (1 + ty));
    ldr[px * 3 + 2] = (uint8_t)(255.f * tz / (1 + tz));
  }
}

// toneMap, path_trace.cu:186-198: sequential divide-then-sum per pixel.
__global__ __launch_bounds__(kBlock) void pixel_mean_kernel(const float *__restrict__ samples, int64_t npix,
                                                            int spp, float *__restrict__ hdr,
                                                            uint8_t *__restrict__ ldr) {
  const int64_t px = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (px >= npix) return;
  const float *s = samples + px * spp * 3;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  const float fs = (float)spp;
  for (int i = 0; i < spp; ++i) {
    tx += s[3 * i] / fs;
    ty += s[3 * i + 1] / fs;
    tz += s[3 * i + 2] / fs;
  }
  hdr[px * 3] = tx;
  hdr[px * 3 + 1] = ty;
  hdr[px * 3 + 2] = tz;
  if (ldr) {
    ldr[px * 3] = (uint8_t)(255.f * tx / (1 + tx));
    ldr[px * 3 + 1] = (uint8_t)(255.f * ty / (1 + ty));
    ldr[px * 3 + 2] = (uint8_t)(255.f * tz / (1 + tz));
  }
}

// ---------------------------------------------------------------------------
// TraceArgs::emit_pmfr: 1/pmf for the power-of-two pmfs (exact multiply), else 0.
static std::vector<double> pmf_reciprocals(const std::vector<float> &pmf) {
  std::vector<double> r(pmf.size(), 0.0);
  for (size_t e = 0; e < pmf.size(); ++e) {
    int ex = 0;
    const double m = std::frexp((double)pmf[e], &ex);
    if (pmf[e] > 0.f && m == 0.5 && ex > -1000) r[e] = std::ldexp(1.0, 1 - ex);
  }
  return r;
}

// The kernel a launch runs: trace_kernel<MODE, SPEC, BVH>, or the material
// adjoint (MODE_ADJ: trace_mat_kernel<SPEC, BVH>, MODE_ADJU: the unbounded
// trace_matu_kernel<SPEC, BVH>), or (the forwards only) the batch forward with
// per-set tables trace_fwd_mat_kernel<MODE, SPEC, BVH>.
// KIND_VFWD / KIND_VMAT: the views' forward and bounded material adjoint
// (trace_fwd_views_kernel, trace_mat_views_kernel).
// KIND_VBFWD / KIND_VBMAT: the same over (material set, view) pairs
// (trace_fwd_views_batch_kernel, trace_mat_views_batch_kernel);
// KIND_VBMAT at MODE_ADJU: the unbounded trace_matu_views_batch_kernel (§21).
// KIND_SHADE: trace_shade_kernel, the small scenes' forwards and bounded adjoints.
// KIND_TANG: trace_tan_kernel, the bounded material adjoint's tangent launch.
enum { KIND_TRACE = 0, KIND_MATG = 1, KIND_FWDB = 2, KIND_VFWD = 3, KIND_VMAT = 4, KIND_VBFWD = 5, KIND_VBMAT = 6, KIND_SHADE = 7, KIND_TANG = 8 };
constexpr int kKindLast = KIND_TANG;
constexpr bool shade_mode(int mode) { return mode == MODE_FWD || mode == MODE_FWDM || mode == MODE_ADJ || mode == MODE_ADJW; }
constexpr bool kind_views(int kind) { return kind == KIND_VFWD || kind == KIND_VMAT; }  // ONE material set
constexpr bool kind_view_sets(int kind) { return kind == KIND_VBFWD || kind == KIND_VBMAT; }
// The (MODE, KIND) pairs that have kernels (kernel_of's static_asserts).
constexpr bool inst_valid(int mode, int kind) {
  return kind == KIND_TRACE  ? mode >= MODE_FWD && mode <= MODE_ADJW
         : kind == KIND_MATG ? mode == MODE_ADJ || mode == MODE_ADJU
         : kind == KIND_VMAT ? mode == MODE_ADJ
         : kind == KIND_VBMAT ? mode == MODE_ADJ || mode == MODE_ADJU
         : kind == KIND_SHADE ? shade_mode(mode)
         : kind == KIND_TANG ? mode == MODE_ADJ
                             : mode == MODE_FWD || mode == MODE_FWDM;
}
// An instance's slot in GpuScene::inst.  0..23: trace_kernel<mode, spec, bvh>;
// 24..27: trace_mat_kernel<spec, bvh>; 28..35: trace_fwd_mat_kernel<FWD | FWDM,
// spec, bvh>; 36..39: trace_matu_kernel<spec, bvh>; 40..47:
// trace_fwd_views_kernel<FWD | FWDM, spec, bvh>; 48..51: trace_mat_views_kernel<spec, bvh>;
// 52..59: trace_fwd_views_batch_kernel<FWD | FWDM, spec, bvh>; 60..63:
// trace_mat_views_batch_kernel<spec, bvh>; 64..67:
// trace_matu_views_batch_kernel<spec, bvh>; 68..91: trace_shade_kernel<mode, spec, false>
// (one formula for every kind: the BVH slots of KIND_SHADE stay unused);
// 92..95: trace_tan_kernel<spec, bvh>.
constexpr int inst_slot(int mode, bool spec, bool bvh, int kind) {
  static_assert(MODE_ADJW == 5, "KIND_SHADE's slots end at 91");
  return (kind == KIND_MATG   ? (mode == MODE_ADJU ? 36 : 24)
          : kind == KIND_TANG ? 92
          : kind == KIND_FWDB ? 28 + (mode == MODE_FWDM ? 4 : 0)
          : kind == KIND_VFWD ? 40 + (mode == MODE_FWDM ? 4 : 0)
          : kind == KIND_VMAT ? 48
          : kind == KIND_VBFWD ? 52 + (mode == MODE_FWDM ? 4 : 0)
          : kind == KIND_VBMAT ? (mode == MODE_ADJU ? 64 : 60)
          : kind == KIND_SHADE ? 68 + mode * 4
                              : mode * 4) +
         (spec ? 2 : 0) + (bvh ? 1 : 0);
}
// One past the largest slot of a valid instance, or -1 when two share a slot.
constexpr int inst_slot_count() {
  bool seen[128] = {};
  int n = 0;
  for (int kind = KIND_TRACE; kind <= kKindLast; ++kind)
    for (int mode = MODE_FWD; mode <= MODE_ADJW; ++mode)
      for (int sb = 0; sb < 4 && inst_valid(mode, kind); ++sb) {
        const int slot = inst_slot(mode, (sb & 2) != 0, (sb & 1) != 0, kind);
        if (slot < 0 || slot >= 128 || seen[slot]) return -1;
        seen[slot] = true;
        n = slot + 1 > n ? slot + 1 : n;
      }
  return n;
}
constexpr int kInstSlots = inst_slot_count();
static_assert(kInstSlots > 0, "two instances share a slot of GpuScene::inst (inst_slot)");

// What the launch path remembers per kernel instance and scene.
struct InstCache {
  int grid = 0;  // resident workgroups (0 = not queried) ...
  size_t grid_lds = 0;  // ... for this many bytes of LDS per workgroup (resident_grid)
  size_t pick_base = 0;  // launch_bvh_pick's choice of LDS extras (kept in the BVH = false slot): base bytes it was made for
  size_t pick_tail = 0;  // ... and the per-block tail (fused pixel mean slots) behind it
  int pick_opt = -1;     // ... the choice (-1 = not made)
};

struct GpuScene {
  HostScene host;
  int device = 0;
  bool on_device = false;
  TriIsect *isect = nullptr;
  TriPair *pairs = nullptr;
  TriGeom *geom = nullptr;
  TriMat *mat = nullptr;
  float *kd = nullptr;
  int *emit_tri = nullptr;
  float *emit_cdf = nullptr, *emit_pmf = nullptr;
  double *emit_pmfr = nullptr;  // TraceArgs::emit_pmfr
  bool has_ks = false;      // some material has a Phong lobe
  TriPair *big_pairs = nullptr;
  int32_t *big_idx = nullptr;
  PairBox2 *big_boxes = nullptr;
  float4 *wide = nullptr;  // WideNode records
  float4 *src_cull = nullptr;  // HostScene::bvh_src_cull
  TriIsect *wtris = nullptr;
  PairBox2 *pboxes = nullptr;  // pair acceptance boxes (small scenes' culled shadow casts)
  uint32_t *pomask = nullptr;  // shadow rays' potential occluders (small scenes)
  uint32_t *big_pomask = nullptr;  // ... over the large-triangle pairs (BVH scenes)
  int accel = IPT_ACCEL_AUTO;
  size_t adju_base = 0;  // gpu_adjoint's choice of LDS ring slots (unbounded, brute force) ...
  int adju_nl = 0;       // ... made for this LDS base
  size_t matu_base = 0;  // gpu_adjoint_mat_unbounded's own choice (trace_matu_kernel's occupancy) ...
  int matu_nl = 0;       // ... for its LDS base
  size_t vbmatu_base = 0;  // gpu_adjoint_views_batch_unbounded's (trace_matu_views_batch_kernel's occupancy) ...
  int vbmatu_nl = 0;       // ... for its LDS base
  int *grad_map = nullptr, *slot_tri = nullptr;  // ADJ hot-set LDS slots (large scenes)
  int *tri_emit = nullptr;  // triangle -> emitter index or -1 (material overrides and adjoint)
  InstCache inst[kInstSlots];  // by inst_slot()
  // dynamic-chunk counters per stream (stream_counters): `words` grab words,
  // zeroed once; every launch leaves them zero (TraceArgs::chunk_ctr)
  struct Counters {
    hipStream_t stream;
    int words;
    uint32_t *dev;
  };
  std::vector<Counters> counters;
  // buffers a grow replaced: a launch on another host thread may hold one it
  // took before the grow and not have enqueued its kernel yet, so they live
  // until gpu_free
  std::vector<uint32_t *> counters_retired;
  std::mutex counters_mu;
};

#ifdef IPT_PHASE_TIMING
extern "C" int ipt_debug_phase_cycles(unsigned long long *out) {  // read and reset (kPhaseWords words)
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_cycles), kPhaseWords * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  unsigned long long z[kPhaseWords] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

#ifdef IPT_BVH_STATS
extern "C" int ipt_debug_bvh_stats(unsigned long long *out) {  // read and reset (kBvhStats counters)
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bvh_stats), kBvhStats * sizeof(unsigned long long)) != hipSuccess)
    return -1;
  unsigned long long z[kBvhStats] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_bvh_stats), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

const HostScene &gpu_host(const GpuScene *s) { return s->host; }
HostScene &gpu_host_mut(GpuScene *s) { return s->host; }

template <typename T>
static int upload(T **dst, const std::vector<T> &v) {
  const size_t n = std::max<size_t>(v.size(), 1) * sizeof(T);
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), n));
  if (!v.empty()) HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <typename T>
static int upload_as_f4(float4 **dst, const std::vector<T> &v) {
  static_assert(sizeof(T) % sizeof(float4) == 0, "record is not a whole number of float4");
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), std::max<size_t>(v.size(), 1) * sizeof(T)));
  if (!v.empty()) HIP_TRY(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

static std::vector<float4> src_cull_f4(const HostScene &host) {
  std::vector<float4> v(host.bvh_src_cull.size() / 4);
  for (size_t i = 0; i < v.size(); ++i)
    v[i] = make_float4(host.bvh_src_cull[4 * i], host.bvh_src_cull[4 * i + 1], host.bvh_src_cull[4 * i + 2],
                       host.bvh_src_cull[4 * i + 3]);
  return v;
}

GpuScene *gpu_upload(const HostScene &host, std::string *err) {
  GpuScene *s = new GpuScene();
  s->host = host;
  if (hipGetDevice(&s->device) != hipSuccess) {
    *err = "no HIP device available";
    delete s;
    return nullptr;
  }
  std::vector<TriPair> pairs((host.isect.size() + 1) / 2);
  pack_pairs(host.isect.data(), (int)host.isect.size(), pairs.data());
  // record nT of the device's TriGeom array: the camera's rotation as a
  // sampling frame, gathered by the in-phase refill's lanes where a
  // continuing lane gathers its triangle's R (trace_body.h)
  std::vector<TriGeom> geom(host.geom);
  geom.resize((size_t)host.nT + 1, TriGeom());
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) geom[(size_t)host.nT].R[i][j] = host.cam[4 * i + j];
  if (upload(&s->isect, host.isect) || upload(&s->pairs, pairs) || upload(&s->geom, geom) || upload(&s->mat, host.mat) ||
      upload(&s->kd, host.kd) || upload(&s->emit_tri, host.emit_tri) || upload(&s->emit_cdf, host.emit_cdf) ||
      upload(&s->emit_pmf, host.emit_pmf) || upload(&s->emit_pmfr, pmf_reciprocals(host.emit_pmf)) ||
      upload(&s->big_pairs, host.bvh_big_pairs) || upload(&s->big_idx, host.bvh_big_idx) ||
      upload(&s->big_boxes, host.bvh_big_boxes) ||
      upload_as_f4(&s->wide, host.bvh_wide) || upload(&s->src_cull, src_cull_f4(host)) ||
      upload(&s->wtris, host.bvh_wtris) || upload(&s->pboxes, pair_boxes(host)) ||
      upload(&s->pomask, shadow_occluder_masks(host)) ||
      upload(&s->big_pomask, host.bvh_big_idx.empty()
                                 ? std::vector<uint32_t>()
                                 : shadow_occluder_masks(host, std::vector<int>(host.bvh_big_idx.begin(),
                                                                                host.bvh_big_idx.end())))) {
    *err = gpu_last_error();
    gpu_free(s);
    return nullptr;
  }
  for (const TriMat &m : host.mat) s->has_ks |= (m.flags & MAT_HAS_KS) != 0;
  {
    std::vector<int> te((size_t)host.nT, -1);
    for (int e = 0; e < host.nE; ++e) te[(size_t)host.emit_tri[(size_t)e]] = e;
    if (upload(&s->tri_emit, te)) {
      *err = gpu_last_error();
      gpu_free(s);
      return nullptr;
    }
  }
  {  // keep stream-ordered scratch blocks in the pool between launches
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, s->device) == hipSuccess) {
      uint64_t keep = ~0ull;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
  }
  if ((size_t)host.nT * 3 * sizeof(double) > (size_t)kLdsGradBytes) {
    // adjoint gradient bins: the largest triangles (most path vertices land on
    // them, so their bins are the contended ones) get LDS slots
    const int slots = kLdsGradBytes / (3 * (int)sizeof(double));
    std::vector<int> order(host.nT), map(host.nT, -1), inv(slots);
    for (int i = 0; i < host.nT; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](int x, int y) { return host.geom[(size_t)x].area > host.geom[(size_t)y].area; });
    for (int k = 0; k < slots; ++k) {
      map[(size_t)order[(size_t)k]] = k;
      inv[(size_t)k] = order[(size_t)k];
    }
    if (upload(&s->grad_map, map) || upload(&s->slot_tri, inv)) {
      *err = gpu_last_error();
      gpu_free(s);
      return nullptr;
    }
  }
  s->on_device = true;
  return s;
}

GpuScene *gpu_host_only(const HostScene &host) {
  GpuScene *s = new GpuScene();
  s->host = host;
  return s;
}
bool gpu_on_device(const GpuScene *s) { return s->on_device; }

void gpu_free(GpuScene *s) {
  if (!s) return;
  if (!s->on_device) {
    delete s;
    return;
  }
  (void)hipFree(s->isect);
  (void)hipFree(s->pairs);
  (void)hipFree(s->geom);
  (void)hipFree(s->mat);
  (void)hipFree(s->kd);
  (void)hipFree(s->emit_tri);
  (void)hipFree(s->emit_cdf);
  (void)hipFree(s->emit_pmf);
  (void)hipFree(s->emit_pmfr);
  (void)hipFree(s->big_pairs);
  (void)hipFree(s->big_idx);
  (void)hipFree(s->big_boxes);
  (void)hipFree(s->wide);
  (void)hipFree(s->src_cull);
  (void)hipFree(s->wtris);
  (void)hipFree(s->pboxes);
  (void)hipFree(s->pomask);
  (void)hipFree(s->big_pomask);
  (void)hipFree(s->grad_map);
  (void)hipFree(s->slot_tri);
  (void)hipFree(s->tri_emit);
  for (auto &c : s->counters) (void)hipFree(c.dev);
  for (uint32_t *p : s->counters_retired) (void)hipFree(p);
  delete s;
}

int gpu_set_kd(GpuScene *s, const float *kd_host) {
  std::memcpy(s->host.kd.data(), kd_host, s->host.kd.size() * sizeof(float));
  if (!s->on_device) return 0;
  HIP_TRY(hipMemcpy(s->kd, kd_host, s->host.kd.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

int gpu_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static int check_frame(const GpuScene *s, const RenderParams &p);
static int check_device(const GpuScene *s) {
  if (!s->on_device) {
    gpu_set_error("scene was loaded host-only (ipt_load_scene_host); it cannot be rendered");
    return -1;
  }
  return 0;
}
static int check_params(const GpuScene *s, const RenderParams &p) { return check_device(s) || check_frame(s, p) ? -1 : 0; }
// (the frame alone: an entry point that refuses on its own arguments before it asks for a device)
static int check_frame(const GpuScene *s, const RenderParams &p) {
  if (p.width <= 0 || p.height <= 0 || p.spp <= 0 || p.row_begin < 0 || p.row_end > p.height ||
      p.row_begin > p.row_end || p.row_step < 1) {
    gpu_set_error("invalid render parameters (width/height/spp > 0, 0 <= row_begin <= row_end <= height, row_step >= 1)");
    return -1;
  }
  if ((uint64_t)p.width * (uint64_t)p.height * (uint64_t)p.spp >= (1ull << 40)) {
    gpu_set_error("too many samples (width*height*spp must be < 2^40)");
    return -1;
  }
  if (s->host.nT <= 0) {
    gpu_set_error("scene has no triangles");
    return -1;
  }
  if (p.nscenes < 1) {
    gpu_set_error("scene batch needs n_scenes >= 1");
    return -1;
  }
  return 0;
}

#ifndef IPT_DEBUG_GRID
#define IPT_DEBUG_GRID 0
#endif
// The one table of trace kernels: the __global__ of (MODE, SPEC, BVH, KIND).
// Occupancy queries and the launch itself go through it.
template <int MODE, bool SPEC, bool BVH, int KIND>
constexpr auto kernel_of() {
  if constexpr (KIND == KIND_TANG) {
    static_assert(MODE == MODE_ADJ, "the tangent launch is the bounded material adjoint's");
    return &trace_tan_kernel<SPEC, BVH>;
  } else if constexpr (KIND == KIND_SHADE) {
    static_assert(shade_mode(MODE), "the shading tables: forwards and bounded adjoints only");
    return &trace_shade_kernel<MODE, SPEC, BVH>;
  } else if constexpr (KIND == KIND_VBMAT) {
    static_assert(MODE == MODE_ADJ || MODE == MODE_ADJU, "the view sets' adjoint is the material adjoint, MODE_ADJ or MODE_ADJU");
    if constexpr (MODE == MODE_ADJU) return &trace_matu_views_batch_kernel<SPEC, BVH>;
    else return &trace_mat_views_batch_kernel<SPEC, BVH>;
  } else if constexpr (KIND == KIND_VBFWD) {
    static_assert(is_fwd<MODE>(), "the view sets' forward: forward instances only");
    return &trace_fwd_views_batch_kernel<MODE, SPEC, BVH>;
  } else if constexpr (KIND == KIND_VMAT) {
    static_assert(MODE == MODE_ADJ, "the views' adjoint is the bounded material adjoint");
    return &trace_mat_views_kernel<SPEC, BVH>;
  } else if constexpr (KIND == KIND_VFWD) {
    static_assert(is_fwd<MODE>(), "the views' forward: forward instances only");
    return &trace_fwd_views_kernel<MODE, SPEC, BVH>;
  } else if constexpr (KIND == KIND_MATG) {
    static_assert(MODE == MODE_ADJ || MODE == MODE_ADJU, "the material adjoint is MODE_ADJ or MODE_ADJU");
    if constexpr (MODE == MODE_ADJU) return &trace_matu_kernel<SPEC, BVH>;
    else return &trace_mat_kernel<SPEC, BVH>;
  } else if constexpr (KIND == KIND_FWDB) {
    static_assert(is_fwd<MODE>(), "the batch forward: forward instances only");
    return &trace_fwd_mat_kernel<MODE, SPEC, BVH>;
  } else {
    return &trace_kernel<MODE, SPEC, BVH>;
  }
}
// ... and its name, for the IPT_DEBUG_GRID prints.
constexpr const char *kernel_name(int mode, int kind) {
  return kind == KIND_SHADE  ? "trace_shade_kernel"
         : kind == KIND_TANG ? "trace_tan_kernel"
         : kind == KIND_VBFWD ? "trace_fwd_views_batch_kernel"
         : kind == KIND_VBMAT ? (mode == MODE_ADJU ? "trace_matu_views_batch_kernel" : "trace_mat_views_batch_kernel")
         : kind == KIND_VFWD ? "trace_fwd_views_kernel"
         : kind == KIND_VMAT ? "trace_mat_views_kernel"
         : kind == KIND_MATG ? (mode == MODE_ADJU ? "trace_matu_kernel" : "trace_mat_kernel")
         : kind == KIND_FWDB ? "trace_fwd_mat_kernel"
                             : "trace_kernel";
}
template <int MODE, bool SPEC, bool BVH, int KIND>
static int resident_grid(GpuScene *s, size_t lds_bytes, int *grid) {
  InstCache &c = s->inst[inst_slot(MODE, SPEC, BVH, KIND)];
  if (c.grid == 0 || c.grid_lds != lds_bytes) {
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_of<MODE, SPEC, BVH, KIND>(), kBlock, lds_bytes));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
    if (per_cu <= 0) {
      gpu_set_error("trace kernel cannot be resident (LDS request too large?)");
      return -1;
    }
    c.grid = per_cu * cus;
    c.grid_lds = lds_bytes;
    if (IPT_DEBUG_GRID)  // (make variant DEFS=-DIPT_DEBUG_GRID=1)
      std::fprintf(stderr, "[ipt] %s<%d,%d,%d>: %zu B LDS/block, %d blocks/CU x %d CUs\n", kernel_name(MODE, KIND), MODE,
                   (int)SPEC, (int)BVH, lds_bytes, per_cu, cus);
  }
  *grid = c.grid;
  return 0;
}

// camera_ray's origin M * (0,0,0,1) per row, with its own operations (fmaf is
// the IEEE fma on host and device), evaluated once: for the scene's camera
// (make_args) and for each entry of a views' table (gpu_views_create).
static void camera_origin(const float *cam, float *org) {
  for (int i = 0; i < 3; ++i) {
    const float *M = cam + 4 * i;
    org[i] = std::fmaf(M[3], 1.f, std::fmaf(M[2], 0.f, std::fmaf(M[1], 0.f, M[0] * 0.f)));
  }
}

static TraceArgs make_args(const GpuScene *s, const RenderParams &p);
static TraceArgs make_args_scene(const GpuScene *s) {
  RenderParams p;
  p.width = p.height = p.spp = 1;
  p.max_bounces = 0;
  p.seed = 0;
  p.row_begin = 0;
  p.row_end = 1;
  return make_args(s, p);
}
static TraceArgs make_args(const GpuScene *s, const RenderParams &p) {
  // Everything not written here is zero / nullptr: the BVH fields and
  // big_pomask (set together, bvh_lds), the gradient bins (adjoint_args),
  // mat_stride and kdpi_g (launch()), the chunk sizes, counters and ADJU ring
  // (launch_inst), the fused pixel mean's fields (render_impl).
  TraceArgs a = TraceArgs();
  a.W = p.width;
  a.H = p.height;
  a.spp = p.spp;
  a.max_bounces = p.max_bounces < 0 ? -1 : p.max_bounces;
  a.seed = p.seed;
  const int rows = band_rows(p);
  a.n_samples = (uint64_t)rows * p.width * p.spp;
  a.nT = s->host.nT;
  a.nE = s->host.nE;
  a.kd_tables = s->host.nT <= kMaxTableTris ? 1 : 0;
  a.small_pairs = s->host.nT <= 2 * kSmallPairs ? 1 : 0;  // (bit 1: shade_offer, in the entry points that can take the tables)
  a.npix = (uint64_t)rows * p.width;
  a.row0 = p.row_begin;
  a.row_step = p.row_step > 1 ? p.row_step : 1;
  const uint64_t total = (uint64_t)p.height * p.width * p.spp;
  a.idx32 = total <= 0xffffffffull ? 1 : 0;
  a.m_spp = p.spp > 1 ? ~0ull / (uint64_t)p.spp + 1 : 0;
  a.m_W = p.width > 1 ? ~0ull / (uint64_t)p.width + 1 : 0;
  a.m_npix = a.npix > 1 ? ~0ull / a.npix + 1 : 0;
  for (int k = 0; k < 6; ++k) a.root_box[k] = s->host.bvh_root_box[k];
  for (int k = 0; k < 4; ++k) a.tree_sphere[k] = s->host.bvh_sphere[k];
  a.src_cull = s->src_cull;
  std::memcpy(a.cam, s->host.cam, sizeof a.cam);
  a.emit_pmfr = s->emit_pmfr;
  camera_origin(a.cam, a.cam_org);  // camera_ray's pr[i], evaluated once
  a.rec_cap = p.max_bounces >= 0 ? p.max_bounces + 1 : 0;
  a.pboxes = s->pboxes;
  a.pomask = s->host.nE > 0 ? s->pomask : nullptr;
  a.nscenes = p.nscenes > 1 ? p.nscenes : 1;
  a.bps = 1;
  a.seed_stride = p.seed_stride;
  a.out_stride = a.n_samples * 3;
  a.adj_stride = (uint64_t)p.width * p.height * 3;
  a.rc_spp = (p.spp > 0 && p.spp <= (1 << 24) && (p.spp & (p.spp - 1)) == 0) ? 1.0f / (float)p.spp : 0.f;
  a.rc_W = (p.width > 0 && (p.width & (p.width - 1)) == 0) ? 1.0f / (float)p.width : 0.f;
  a.rc_H = (p.height > 0 && (p.height & (p.height - 1)) == 0) ? 1.0f / (float)p.height : 0.f;
  return a;
}

// Acceleration structure of a launch: the BVH when the scene has one and is
// past the brute-force size (or the caller forced it), else the pair loop.
static bool use_bvh(const GpuScene *s) {
  if (s->host.bvh_nodes.empty()) return false;
  if (s->accel == IPT_ACCEL_BVH) return true;
  if (s->accel == IPT_ACCEL_BRUTE) return false;
  return s->host.nT >= kBvhMinTris;
}

// trace_kernel's lane_ws: six words per lane (the BVH forwards, and MODE_ADJW)
constexpr size_t kLaneWsBytes = (size_t)6 * kBlock * sizeof(uint32_t);

// BVH LDS carve-out on top of `base` bytes; fills the args' BVH fields:
// [wide nodes if staged][large pairs' plane offsets][large pairs' copy if
// taken][emitter records][the wave's 8 group stacks].
static size_t bvh_lds(const GpuScene *s, TraceArgs &a, size_t base, bool stage = true, bool big_copy = true,
                      bool lane_words = false) {
  const size_t nw = s->host.bvh_wide.size();
  a.bvh_wide = s->wide;
  a.bvh_wtris = s->wtris;
  a.bvh_wide_lds = (stage && nw * kWideF4 * sizeof(float4) <= (size_t)kBvhLdsNodeBytes) ? (int)nw : 0;
  a.bvh_big_lds = big_copy ? 1 : 0;
  a.big_pomask = (s->host.nE > 0 && !s->host.bvh_big_idx.empty()) ? s->big_pomask : nullptr;
  a.coop_stride = 7 * s->host.bvh_wdepth + 8;
  a.bvh_nbig = (int)s->host.bvh_big_pairs.size();
  a.bvh_big = s->big_pairs;
  a.bvh_big_idx = s->big_idx;
  a.bvh_big_boxes = s->big_boxes;
  const size_t head = bvh_lds_offset(base) + (size_t)a.bvh_wide_lds * kWideF4 * sizeof(float4) +
                      (size_t)a.bvh_nbig * 6 * sizeof(float) + (a.bvh_big_lds ? big_lds_bytes(a.bvh_nbig) : 0) +
                      emit_lds_bytes(s->host.nE);
  return head + (size_t)(kBlock / 64) * 8 * a.coop_stride * sizeof(uint32_t) + (lane_words ? kLaneWsBytes : 0);
}

// The shading tables' bytes at the front of a workgroup's LDS (TraceArgs::small_pairs bit 1)
static size_t shade_bytes(const TraceArgs &a) {
  return (a.small_pairs & kSmallShade) ? (size_t)shade_table_words(a.nT, a.nE) * sizeof(uint32_t) : 0;
}
// Offered by the entry points whose launch can run a trace_shade_kernel
// instance (the forwards and the bounded adjoint of a brute-force scene), and
// by no other: every size and limit an entry point derives from table_bytes
// then counts the tables exactly where the launch may carry them.
static void shade_offer(const GpuScene *s, TraceArgs &a) {
  if ((a.small_pairs & 1) && !use_bvh(s) && shade_tables_fit(s->host.nT, s->host.nE))
    a.small_pairs |= kSmallShade;
}
// ... which must not cost a launch a resident workgroup: dropped (bit and
// bytes) when `lds` + `extra` with them fits fewer workgroups per CU than
// without, counting up to the `cap` that the instance's registers allow.
static bool shade_keeps_residency(const TraceArgs &a, size_t lds, size_t extra, size_t cap) {
  const size_t sh = shade_bytes(a), cu = 160 * 1024;
  return std::min(cap, cu / (lds + extra)) >= std::min(cap, cu / (lds + extra - sh));
}

static size_t table_bytes(const TraceArgs &a) {
  return (a.kd_tables ? (size_t)6 * a.nT * sizeof(float) : 0) +
         (a.small_pairs ? (size_t)kE3Floats * ((a.nT + 1) / 2) * sizeof(float) + 12 +
                              (size_t)((a.nT + 1) / 2) * sizeof(TriPair) +
                              (a.pomask ? (size_t)a.nT * a.nE * sizeof(uint32_t) : 0) +
                              shade_bytes(a)
                        : 0);
}

// Per-launch scratch (the fused render's sample buffer, kd/pi of large
// scenes) is allocated in stream order on the launch's own stream and freed
// behind it: launches on different streams never share a buffer, and the
// device's default pool (release threshold raised in gpu_upload) recycles
// the blocks without a device-wide synchronisation.
struct StreamScratch {
  void *p = nullptr;
  hipStream_t st = nullptr;
  int alloc(size_t bytes, hipStream_t stream) {
    st = stream;
    HIP_TRY(hipMallocAsync(&p, std::max<size_t>(bytes, 16), st));
    return 0;
  }
  ~StreamScratch() {
    if (p) (void)hipFreeAsync(p, st);
  }
};

// The chunk counters of launches on stream `st` with `words` grab words:
// one buffer per (scene, stream), allocated and zeroed (on `st`, in stream
// order) at the stream's first launch and replaced by a larger one when a
// launch needs more words (the old one is kept until gpu_free: another host
// thread may have taken it for a launch it has not enqueued yet -- launches
// already queued on it leave it zeroed and never touch the new one, so no
// synchronisation is needed).  Every launch leaves them zeroed
// (TraceArgs::chunk_ctr), so the host keeps no copy of device state: a launch
// that fails before or after enqueueing changes nothing the next one depends
// on, and any kind of launch (single set, regions, scene batch) may follow any
// other on the stream.  Launches on one stream run in order; other streams
// get their own buffers.  A launch captured into a graph gets a zeroed buffer
// of its own inside the graph (*scratch, freed behind it), so a replay never
// shares words with launches on the capturing stream.
static int stream_counters(GpuScene *s, hipStream_t st, int words, uint32_t **out, void **scratch) {
  const size_t bytes = (size_t)words * sizeof(uint32_t);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone) {
    HIP_TRY(hipMallocAsync(scratch, bytes, st));
    HIP_TRY(hipMemsetAsync(*scratch, 0, bytes, st));
    *out = (uint32_t *)*scratch;
    return 0;
  }
  std::lock_guard<std::mutex> lk(s->counters_mu);
  GpuScene::Counters *c = nullptr;
  for (auto &e : s->counters)
    if (e.stream == st) c = &e;
  if (c && c->words < words) {  // grow: a new buffer; the old one is retired, not freed
    s->counters_retired.push_back(c->dev);
    c->dev = nullptr;
    c->words = 0;
  }
  if (!c || c->dev == nullptr) {
    const int w = std::max(words, 16);
    uint32_t *dev = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev), (size_t)w * sizeof(uint32_t)));
    // zeroed ON the launch stream: a blocking hipMemset goes to the null
    // stream, which a non-blocking stream (every torch stream) does not wait
    // for (round 4's race)
    HIP_TRY(hipMemsetAsync(dev, 0, (size_t)w * sizeof(uint32_t), st));
    if (c) {
      c->dev = dev;
      c->words = w;
    } else {
      s->counters.push_back({st, w, dev});
      c = &s->counters.back();
    }
  }
  *out = c->dev;
  return 0;
}

// Guided chunk sizes (TraceArgs::chunk_big_n), BVH instances: a launch hands
// out its last ~IPT_GUIDED_TAIL small chunks per wave (64 work items) after
// the big ones, so the waves that take the last chunks finish close to the
// others -- a BVH loop iteration is ~2.4x a brute-force one, so a big chunk
// taken at the end kept its wave busy long after the rest of the grid ran
// dry.  North-star 1/8 share: forward 0.814 -> 0.727 ms, adjoint 0.933 ->
// 0.850 (4 per wave; 1 and 2 less).  The brute-force scenes lose with it
// (C2 1/8 share 0.278 -> 0.297 ms at 2 per wave: the fused render's 64-sample
// chunks outrun its two LDS slots, and each extra grab is an atomic round
// trip the wave waits for), so their instances keep fixed chunks
// (profiles/r03/envab_r03j.log).
#ifndef IPT_GUIDED_TAIL
#define IPT_GUIDED_TAIL 4
#endif

// Grabs of one counter word in a launch (a set's or a region's; units, big
// chunks and waves as chunk_range and the kernel's loop see them): chunks 0 ..
// rw-1 are the waves' own, each later chunk is taken by one successful grab,
// and every wave ends with exactly one failed grab -- the non-fused loop
// grabs when its range is used up and stops at the first chunk past the end;
// the fused loop grabs when its chunk is used up, or at once when its own
// chunk is past the end.  Guided instances (BVH) hand out nb chunks of c
// units and then chunks of `small`, the others only chunks of c.
static uint32_t launch_grabs(bool guided, uint64_t units, uint64_t c, uint64_t small, uint64_t nb, uint64_t rw) {
  const uint64_t chunks = guided ? nb + (units - nb * c + small - 1) / small : (units + c - 1) / c;
  return (uint32_t)((chunks > rw ? chunks - rw : 0) + rw);
}
#ifndef IPT_DYN_SMALL_CHUNK
#define IPT_DYN_SMALL_CHUNK 64
#endif

// What a launch reads and writes besides the scene, by name; whatever a kind
// of launch does not use stays null.
struct LaunchIO {
  const float *kd = nullptr;  // albedo (nullptr: the scene's own)
  float *out = nullptr;       // forwards: samples, or the HDR images of the fused render
  const float *adj = nullptr;  // adjoints: dL/dI ...
  double *grad = nullptr;      // ... and their gradient
  const uint8_t *target = nullptr;  // graph: target image ...
  double *edges = nullptr;          // ... and bins
  const TriMat *mat = nullptr;  // TriMat table (nullptr: the scene's own; the overrides pass what pack_mat_kernel wrote)
  const float *views = nullptr;  // KIND_VFWD / KIND_VMAT: the views' table
  int nviews = 0;                // KIND_VBFWD / KIND_VBMAT: its entries V (the launch has nscenes / V material sets)
  const float *tkd = nullptr, *tks = nullptr, *tke = nullptr;  // KIND_TANG: the tangents (nullptr: zero) ...
  int ntan = 0;                                                // ... and their count; `grad` is the tangent images
  hipStream_t stream = nullptr;
  size_t tail = 0;  // bytes per workgroup behind everything else (16-B aligned; the fused pixel mean's slots, TraceArgs::mean_off)
};

template <int MODE, bool SPEC, bool BVH, int KIND>
static int launch_inst(GpuScene *s, const TraceArgs &a, size_t lds, const LaunchIO &io) {
  const hipStream_t st = io.stream;
  int grid = 0;
  if (lds > 160 * 1024) {
    gpu_set_error("LDS footprint of the launch exceeds 160 KiB");
    return -1;
  }
  if (resident_grid<MODE, SPEC, BVH, KIND>(s, lds, &grid)) return -1;
  if (a.n_samples == 0) return 0;
  TraceArgs b = a;
  if (a.nscenes > 1) {  // scene batch: an equal share of the resident blocks per material set
    b.bps = std::max(1, grid / a.nscenes);
    grid = b.bps * a.nscenes;
  }
  b.chunk_ctr = nullptr;
  StreamScratch cap_ctr;  // only for a launch captured into a graph
  // ~IPT_DYN_CHUNKS_PER_WAVE chunks per wave, a multiple of 64 items, 64..4096
  const uint64_t waves = (uint64_t)(a.nscenes > 1 ? b.bps : grid) * (kBlock / 64);
  uint64_t c = (a.n_samples / (waves * IPT_DYN_CHUNKS_PER_WAVE) + 63) / 64 * 64;
  c = std::min<uint64_t>(std::max<uint64_t>(c, IPT_DYN_MIN_CHUNK), 4096);
  uint64_t units = a.n_samples, small = std::min<uint64_t>(c, IPT_DYN_SMALL_CHUNK);
  if (a.fused) {  // fused pixel mean: chunks of a.chunk pixels (all their samples), small ones of >= 64 samples
    // a launch with fewer chunks than waves (a thin band) halves them while
    // that gives the idle waves work and a chunk keeps >= 64 samples: C2's
    // 1/64 share 0.217 -> 0.10 ms (profiles/r03/launch_scaling_r03w.jsonl)
    c = a.chunk;
    while (c > 1 && (a.npix + c - 1) / c < waves && (c / 2) * (uint64_t)a.spp >= 64) c /= 2;
    b.group = std::min<uint32_t>(a.group, (uint32_t)c);
    small = std::min<uint64_t>(c, std::max<uint64_t>(1, 64 / (uint64_t)a.spp));
    units = a.npix;
  }
  // guided sizes: the last ~IPT_GUIDED_TAIL small chunks per wave end the launch
  // (non-guided instances: one size, chunk_small = chunk and no big-chunk count;
  // IPT_BF_BIG > 1: big chunks of IPT_BF_BIG x c, then IPT_BF_TAIL chunks of
  // c per wave -- fewer grabs for the same tail)
  if (!BVH) {
    small = c;
    c *= IPT_BF_BIG;
  }
  b.chunk = (uint32_t)c;
  b.chunk_small = (uint32_t)small;
  const uint64_t rw = waves;  // chunks 0 .. rw-1: the waves' own; every wave ends with one failed grab
  constexpr bool guided = kGuided<BVH>();
  const uint64_t tail = guided ? rw * (uint64_t)(BVH ? IPT_GUIDED_TAIL : IPT_BF_TAIL) * small : 0;
  const uint64_t nb = guided ? (units > tail ? (units - tail) / c : 0) : 0;
  b.chunk_big_n = (uint32_t)nb;
  b.grabs = launch_grabs(guided, units, c, small, nb, rw);
  cap_ctr.st = st;
  const int words = a.nscenes * kCtrStride;
  if (stream_counters(s, st, words, &b.chunk_ctr, &cap_ctr.p)) return -1;
  StreamScratch grec, mring;  // ADJU: the vertex-record ring (TraceArgs::grec), freed behind the launch
  if (MODE == MODE_ADJU) {  // the ring's global slots: one chunk pool per wave
    const size_t fields = SPEC ? kRecFieldsSpec : kRecFieldsDiffuse;
    const size_t waves = (size_t)grid * (kBlock / 64), chunk = (size_t)kPoolSlots * fields * sizeof(float);
    b.pool_chunks = (int)std::max<size_t>(16, std::min<size_t>(63, ((size_t)IPT_ADJU_POOL_MB << 20) / (waves * chunk)));
    if (g_adju_pool.load() > 0) b.pool_chunks = g_adju_pool.load();
    b.grec_stride = (uint64_t)b.pool_chunks * kPoolSlots * fields;  // floats per wave
    b.rec_cap = std::min(kAdjuRing, a.rec_lds + kPoolMaxChunks * kPoolSlots);
    if (grec.alloc(waves * b.grec_stride * sizeof(float), st)) return -1;
    b.grec = (float *)grec.p;
    if (kSub > 0) {  // the captured prefix throughputs of the sub-chunked sweep
      if (mring.alloc(waves * (size_t)kMrEnt * 64 * 3 * sizeof(float), st)) return -1;
      b.mring = (float *)mring.p;
    }
  }
  // (tests: a launch that fails after its counters and scratch are allocated)
  if (g_fail_launches.load() > 0 && g_fail_launches.fetch_sub(1) > 0) {
    gpu_set_error("launch failed on request (ipt_debug_fail_launches)");
    return -1;
  }
  if (IPT_DEBUG_GRID)  // every number of the launch the host decides (no pointers)
    std::fprintf(stderr,
                 "[ipt] launch %s<%d,%d,%d> grid=%d lds=%zu bps=%d chunk=%u chunk_small=%u chunk_big_n=%u grabs=%u group=%u "
                 "rec_cap=%d rec_lds=%d pool_chunks=%d grec_stride=%llu grad_slots=%d bvh_wide_lds=%d bvh_big_lds=%d "
                 "coop_stride=%d mean_off=%u mean_wstride=%u nslots=%d mat_stride=%u kd_tables=%d small_pairs=%d "
                 "sample_major=%d\n",
                 kernel_name(MODE, KIND), MODE, (int)SPEC, (int)BVH, grid, lds, b.bps, b.chunk, b.chunk_small,
                 b.chunk_big_n, b.grabs, b.group, b.rec_cap, b.rec_lds, b.pool_chunks, (unsigned long long)b.grec_stride,
                 b.grad_slots, b.bvh_wide_lds, b.bvh_big_lds, b.coop_stride, b.mean_off, b.mean_wstride, b.nslots,
                 b.mat_stride, b.kd_tables, b.small_pairs, b.sample_major);
  {  // ipt_debug_last_launch
    const int32_t rec[kLastLaunchFields] = {
        0, MODE, (int)SPEC, (int)BVH, KIND, b.kd_tables, b.small_pairs, b.grad_slots, b.bvh_wide_lds, b.rec_lds, b.lds_edges,
        (int32_t)lds, b.rec_cap, b.bvh_big_lds, BVH && emit_lds_bytes(b.nE) ? 1 : 0, grid, b.nT, b.nE};
    std::lock_guard<std::mutex> lk(g_last_launch_mu);
    const int32_t count = g_last_launch[0] + 1;
    std::memcpy(g_last_launch, rec, sizeof rec);
    g_last_launch[0] = count;
  }
  // the parameters every trace kernel takes, then its own trailing ones
  auto enqueue = [&](auto... trailing) {
    hipLaunchKernelGGL((kernel_of<MODE, SPEC, BVH, KIND>()), dim3(grid), dim3(kBlock), lds, st, b, s->isect, s->pairs,
                       s->geom, io.mat ? io.mat : s->mat, io.kd ? io.kd : s->kd, s->emit_tri, s->emit_cdf, s->emit_pmf,
                       io.out, io.adj, io.grad, io.target, io.edges, trailing...);
  };
  if constexpr (KIND == KIND_VBMAT) enqueue(s->tri_emit, io.views, io.nviews);
  else if constexpr (KIND == KIND_VBFWD) enqueue(io.views, io.nviews);
  else if constexpr (KIND == KIND_VMAT) enqueue(s->tri_emit, io.views);
  else if constexpr (KIND == KIND_VFWD) enqueue(io.views);
  else if constexpr (KIND == KIND_MATG) enqueue(s->tri_emit);
  else if constexpr (KIND == KIND_TANG) enqueue(s->tri_emit, io.tkd, io.tks, io.tke, io.ntan);
  else enqueue();
  HIP_TRY(hipGetLastError());
  return 0;
}

// The Phong paths (double-precision pow) are compiled only into the SPEC
// instance, used when some material has Ks != 0; the shipped scenes have
// none, and dropping the code lowers register pressure (occupancy).  The BVH
// instances carry the traversal (and its LDS) only for large scenes.
// kd / pi once per launch for scenes without LDS tables (the same IEEE
// division the per-vertex code would do three times per vertex)
__global__ __launch_bounds__(kBlock) void kdpi_kernel(const float *__restrict__ kd, int n, float *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = kd[i] / kPiF;
}

// BVH instances: the LDS extras (the wide nodes' stage, the large pairs' copy
// of the culled path pre-pass) are taken only as far as they cost no
// residency: of the four combinations, the first (most staged) with the most
// resident workgroups per CU.  North-star adjoint: the tree stage + records +
// bins sit just under 3 workgroups/CU, and the pair copy would tip it to 2
// (6.6 -> 7.9 ms).  Cached per scene and instance for the base LDS bytes.
template <int MODE, bool SPEC, int KIND>
static int launch_bvh_pick(GpuScene *s, TraceArgs &a, size_t *lds, size_t tail) {
  InstCache &c = s->inst[inst_slot(MODE, SPEC, false, KIND)];
  const bool opt[4][2] = {{true, true}, {true, false}, {false, true}, {false, false}};
  const size_t base = *lds;
  if (c.pick_opt < 0 || c.pick_base != base || c.pick_tail != tail) {
    int best = -1, best_per_cu = 0;
    for (int k = 0; k < 4; ++k) {
      TraceArgs b = a;
      const size_t l = bvh_lds_offset(bvh_lds(s, b, base, opt[k][0], opt[k][1], is_fwd<MODE>())) + tail;
      if (l > 160 * 1024) continue;
      int per_cu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_of<MODE, SPEC, true, KIND>(), kBlock, l));
      if (per_cu > best_per_cu) {
        best = k;
        best_per_cu = per_cu;
      }
    }
    if (best < 0) {
      gpu_set_error("BVH trace kernel cannot be resident (LDS request too large?)");
      return -1;
    }
    c.pick_opt = best;
    c.pick_base = base;
    c.pick_tail = tail;
  }
  const int k = c.pick_opt;
  *lds = bvh_lds(s, a, base, opt[k][0], opt[k][1], is_fwd<MODE>());
  return 0;
}

// One launch: `a` as the entry point filled it, `lds` its bytes before the
// BVH carve-out and the tail.  SPEC and BVH are chosen here, once.
template <int MODE, int KIND = KIND_TRACE>
static int launch(GpuScene *s, TraceArgs a, size_t lds, const LaunchIO &io) {
  const hipStream_t st = io.stream;
  // a batch's per-launch table holds one TriMat table per set (pack_materials);
  // its forward runs the instances that offset mat per set
  // (views: one table, one kd for every set; view sets: one of each per material set)
  const int msets = kind_views(KIND) ? 1 : kind_view_sets(KIND) ? a.nscenes / io.nviews : a.nscenes;
  a.mat_stride = (io.mat && msets > 1) ? (uint32_t)a.nT : 0u;
  if constexpr (is_fwd<MODE>() && KIND == KIND_TRACE) {
    if (a.mat_stride) return launch<MODE, KIND_FWDB>(s, a, lds, io);
  }
  StreamScratch kdpi;
  if (MODE != MODE_GRAPH && !a.kd_tables && a.n_samples > 0) {
    const int n = 3 * s->host.nT * msets;
    if (kdpi.alloc((size_t)n * sizeof(float), st)) return -1;
    hipLaunchKernelGGL(kdpi_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, io.kd ? io.kd : s->kd, n,
                       (float *)kdpi.p);
    HIP_TRY(hipGetLastError());
    a.kdpi_g = (const float *)kdpi.p;
  }
  // The shading tables (shade_offer sets the bit where the scene fits): a
  // forward or bounded adjoint of a brute-force scene that keeps its resident
  // workgroups with them runs its trace_shade_kernel instance; every other
  // launch drops the bit and the bytes.
  if (a.small_pairs & kSmallShade) {
    bool take = KIND == KIND_SHADE;
    if constexpr (KIND == KIND_TRACE && shade_mode(MODE))
      take = !use_bvh(s) && shade_keeps_residency(a, lds, io.tail ? io.tail + 15 : 0, MODE == MODE_ADJW ? 6 : 5);
    if (!take) {
      lds -= shade_bytes(a);
      a.small_pairs &= ~kSmallShade;
    }
    if constexpr (KIND == KIND_TRACE && shade_mode(MODE)) {
      if (take) return launch<MODE, KIND_SHADE>(s, a, lds, io);
    }
    if (KIND == KIND_SHADE && a.n_samples > 0) g_shade_launches.fetch_add(1);
  }
  auto run = [&](auto spec, auto bvh) {  // the instance: LDS extras of the BVH, then the tail, then the launch
    constexpr bool SPEC = decltype(spec)::value, BVH = decltype(bvh)::value;
    if constexpr (BVH) {
      if (launch_bvh_pick<MODE, SPEC, KIND>(s, a, &lds, io.tail)) return -1;
    }
    if (io.tail) {
      a.mean_off = (uint32_t)bvh_lds_offset(lds);
      lds = a.mean_off + io.tail;
    }
    return launch_inst<MODE, SPEC, BVH, KIND>(s, a, lds, io);
  };
  constexpr std::true_type yes;
  constexpr std::false_type no;
  if constexpr (MODE == MODE_ADJW) return run(no, no);  // (gpu_adjoint: brute-force diffuse scenes only)
  else if constexpr (KIND == KIND_SHADE) return s->has_ks ? run(yes, no) : run(no, no);
  else if (use_bvh(s)) return s->has_ks ? run(yes, yes) : run(no, yes);
  else return s->has_ks ? run(yes, no) : run(no, no);
}

int gpu_render_samples(GpuScene *s, const RenderParams &p, const float *kd_dev, float *samples_dev, void *stream) {
  if (check_params(s, p)) return -1;
  TraceArgs a = make_args(s, p);
  shade_offer(s, a);
  LaunchIO io;
  io.kd = kd_dev, io.out = samples_dev, io.stream = (hipStream_t)stream;
  return launch<MODE_FWD>(s, a, table_bytes(a), io);
}

int gpu_pixel_mean(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev, void *stream) {
  if (npix <= 0) return 0;
  const int blocks = (int)((npix + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(pixel_mean_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, samples_dev, npix, spp,
                     hdr_dev, ldr_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

template <int KIND = KIND_TRACE>
static int render_samples_sm(GpuScene *s, const RenderParams &p, const float *kd_dev, float *samples_dev,
                             void *stream, const TriMat *mat_dev, const float *views_dev = nullptr,
                             int nviews = 0) {
  if (check_params(s, p)) return -1;
  TraceArgs a = make_args(s, p);
  a.sample_major = 1;
  if (KIND == KIND_TRACE) shade_offer(s, a);
  LaunchIO io;
  io.kd = kd_dev, io.out = samples_dev, io.mat = mat_dev, io.views = views_dev, io.nviews = nviews;
  io.stream = (hipStream_t)stream;
  return launch<MODE_FWD, KIND>(s, a, table_bytes(a), io);
}
int gpu_render_samples_sm(GpuScene *s, const RenderParams &p, const float *kd_dev, float *samples_dev,
                          void *stream) {
  return render_samples_sm(s, p, kd_dev, samples_dev, stream, nullptr);
}

static int pixel_mean_sm_sets(const float *samples_dev, int64_t npix, int spp, int nsets, float *hdr_dev,
                              uint8_t *ldr_dev, void *stream) {
  if (npix <= 0 || nsets <= 0) return 0;
  const int blocks = (int)((npix + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(pixel_mean_sm_kernel, dim3(blocks, nsets), dim3(kBlock), 0, (hipStream_t)stream, samples_dev,
                     npix, spp, hdr_dev, ldr_dev);
  HIP_TRY(hipGetLastError());
  return 0;
}

int gpu_pixel_mean_sm(const float *samples_dev, int64_t npix, int spp, float *hdr_dev, uint8_t *ldr_dev,
                      void *stream) {
  return pixel_mean_sm_sets(samples_dev, npix, spp, 1, hdr_dev, ldr_dev, stream);
}

// Fused pixel mean: the ring of one-pixel slots per wave
// (nslots, <= 16, spp x 3 floats each, IPT_FUSED_WAVE_BYTES of LDS per wave)
// and the pixels per group (a power of two, group x spp <= 256 samples, >= 32),
// or {0, 0} when the launch renders through the sample
// buffer + pixel_mean_sm_kernel instead.  A pixel's slot stays busy until its
// last sample is in, so the ring holds at least two groups (bounded paths of
// <= 8 bounces) or four (longer or unbounded paths: a few long paths then
// still leave the next groups their slots -- simulated lane use >= 99% for
// the reference's Russian roulette).  The index math needs
// < 2^32 samples per frame.  (The unfused path stays reachable through
// ipt_render_samples_sm_dev + ipt_pixel_mean_sm_dev.)
#ifndef IPT_FUSED_GRAB_SAMPLES  // samples handed out per counter grab (at least)
#define IPT_FUSED_GRAB_SAMPLES 256
#endif
#ifndef IPT_FUSED_WAVE_BYTES
#define IPT_FUSED_WAVE_BYTES 6144
#endif
struct FusedShape {
  int slots, group, per_grab;  // per_grab: groups per chunk (counter grab)
};
// BVH scenes keep the two-kernel render unless the library is built with
// IPT_FUSED_BVH=1 (make variant, A/B timing): their LDS already holds the
// tree stage, and slots beyond IPT_FUSED_BVH_WAVE_BYTES per wave cost
// residency (north-star 3.82 -> 4.10 ms fused,
// profiles/r04/envab_fusedbvh_r04e.log).
#ifndef IPT_FUSED_BVH
#define IPT_FUSED_BVH 0
#endif
#ifndef IPT_FUSED_BVH_WAVE_BYTES
#define IPT_FUSED_BVH_WAVE_BYTES 3072
#endif
static FusedShape fused_shape(const RenderParams &p, bool bvh) {
  const FusedShape none = {0, 0, 0};
  if ((uint64_t)p.width * (uint64_t)p.height * (uint64_t)p.spp > 0xffffffffull || p.spp > 256) return none;
  int bytes = IPT_FUSED_WAVE_BYTES;
  if (bvh) {
    if (!IPT_FUSED_BVH) return none;
    bytes = IPT_FUSED_BVH_WAVE_BYTES;
  }
  const int slots = std::min(16, bytes / (12 * p.spp));
  const bool long_paths = p.max_bounces < 0 || p.max_bounces > 8;
  const int cap = slots / (long_paths ? 4 : 2);  // groups the ring holds at once
  if (cap < 1) return none;
  int g = 1;
  while (2 * g <= cap && 2 * g * p.spp <= 256) g *= 2;
  if (g * p.spp < 32) return none;  // (tiny spp: a grab per few samples; the two-kernel render wins)
  // a grab hands out >= 256 samples (small groups -- spp > 128, or long
  // paths -- would otherwise grab per pixel: the legacy 100-spp createImage
  // issued 250 000 counter atomics, 8 MB of memory-side writes per frame)
  const int per_grab = std::min(8, (IPT_FUSED_GRAB_SAMPLES + g * p.spp - 1) / (g * p.spp));
  return {slots, g, per_grab};
}

// mat_dev: the launch's TriMat table (nullptr: the scene's own)
// KIND_VFWD: the sets are the views of views_dev (gpu_render_views)
// KIND_VBFWD: the sets are (material set, view) pairs over its nviews entries (gpu_render_views_batch)
template <int KIND = KIND_TRACE>
static int render_impl(GpuScene *s, const RenderParams &p, const float *kd_dev, float *hdr_dev, uint8_t *ldr_dev,
                       void *stream, const TriMat *mat_dev, const float *views_dev = nullptr, int nviews = 0) {
  if (check_params(s, p)) return -1;
  const int64_t npix = (int64_t)band_rows(p) * p.width;
  const int sets = p.nscenes > 1 ? p.nscenes : 1;
  // (BVH scenes: two-kernel render by default, see fused_shape)
  const FusedShape fs = fused_shape(p, use_bvh(s));
  if (fs.group > 0) {
    TraceArgs a = make_args(s, p);
    if (KIND == KIND_TRACE) shade_offer(s, a);
    a.fused = 1;
    a.group = (uint32_t)fs.group;
    a.chunk = (uint32_t)(fs.group * fs.per_grab);  // pixels per grab; launch_inst may halve it for thin launches
    a.nslots = fs.slots;
    // floats per wave: slot table, the group's pixel entries (brute force), slots
    a.mean_wstride = (uint32_t)(((2 * fs.slots + 3) & ~3) + fused_entry_words((uint32_t)fs.group, use_bvh(s)) +
                                3 * fs.slots * p.spp + 3) & ~3u;
    a.ldr = ldr_dev;
    a.out_stride = (uint64_t)npix * 3;  // per material set: its own HDR (and LDR) image
    LaunchIO io;
    io.kd = kd_dev, io.out = hdr_dev, io.mat = mat_dev, io.views = views_dev, io.nviews = nviews;
    io.stream = (hipStream_t)stream;
    io.tail = (size_t)(kBlock / 64) * a.mean_wstride * sizeof(float);
    return launch<MODE_FWDM, KIND>(s, a, table_bytes(a), io);
  }
  StreamScratch ws;
  if (ws.alloc((size_t)sets * npix * p.spp * 3 * sizeof(float), (hipStream_t)stream)) return -1;
  if (render_samples_sm<KIND>(s, p, kd_dev, (float *)ws.p, stream, mat_dev, views_dev, nviews)) return -1;
  return pixel_mean_sm_sets((const float *)ws.p, npix, p.spp, sets, hdr_dev, ldr_dev, stream);
}
int gpu_render(GpuScene *s, const RenderParams &p, const float *kd_dev, float *hdr_dev, uint8_t *ldr_dev,
               void *stream) {
  return render_impl(s, p, kd_dev, hdr_dev, ldr_dev, stream, nullptr);
}

// ------------------------------------------------------------ material parameters (Kd, Ks, Ke)
// Structure is frozen at load: the emitter list and the lobe
// flags stay; these entry points change values only, and rows outside the
// masks are forced to 0.
int gpu_set_material_params(GpuScene *s, const float *kd, const float *ks, const float *ke) {
  HostScene &h = s->host;
  if (kd) std::memcpy(h.kd.data(), kd, h.kd.size() * sizeof(float));
  std::vector<char> em((size_t)h.nT, 0);
  for (int e : h.emit_tri) em[(size_t)e] = 1;
  for (int i = 0; i < h.nT; ++i) {
    TriMat &m = h.mat[(size_t)i];
    for (int c = 0; c < 3; ++c) {
      if (ks) m.ks[c] = (m.flags & MAT_HAS_KS) ? ks[3 * i + c] : 0.f;
      if (ke) m.ke[c] = em[(size_t)i] ? ke[3 * i + c] : 0.f;
    }
  }
  if (!s->on_device) return 0;
  if (kd) HIP_TRY(hipMemcpy(s->kd, h.kd.data(), h.kd.size() * sizeof(float), hipMemcpyHostToDevice));
  if (ks || ke) HIP_TRY(hipMemcpy(s->mat, h.mat.data(), h.mat.size() * sizeof(TriMat), hipMemcpyHostToDevice));
  return 0;
}

// The launch's TriMat tables for ks / ke overrides (device arrays, sets*nT*3
// each): one table per material set, written by one launch; *mat stays
// nullptr (the scene's own table, for every set) when both are null.
static int pack_materials(GpuScene *s, const float *ks_dev, const float *ke_dev, int sets, hipStream_t st,
                          StreamScratch &buf, const TriMat **mat) {
  *mat = nullptr;
  if (!ks_dev && !ke_dev) return 0;
  const int nT = s->host.nT;
  if (buf.alloc((size_t)sets * nT * sizeof(TriMat), st)) return -1;
  hipLaunchKernelGGL(pack_mat_kernel, dim3((nT + kBlock - 1) / kBlock, sets), dim3(kBlock), 0, st, s->mat, ks_dev,
                     ke_dev, s->tri_emit, nT, (TriMat *)buf.p);
  HIP_TRY(hipGetLastError());
  *mat = (const TriMat *)buf.p;
  return 0;
}

// A batch's kd: the caller's sets*nT*3 array, or the scene's own kd repeated
// for every set (stream scratch, on the launch's stream).
static int batch_kd(GpuScene *s, const float **kd_dev, int sets, hipStream_t st, StreamScratch &buf) {
  if (*kd_dev || sets <= 1) return 0;
  const int n = 3 * s->host.nT;
  const size_t total = (size_t)sets * n;
  if (buf.alloc(total * sizeof(float), st)) return -1;
  hipLaunchKernelGGL(replicate_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, s->kd, n,
                     total, (float *)buf.p);
  HIP_TRY(hipGetLastError());
  *kd_dev = (const float *)buf.p;
  return 0;
}

// What a material launch reads besides the scene: its kd (batch_kd) and its
// TriMat tables (pack_materials), enqueued on the launch's stream in that
// order; the scratch is freed behind the launch, in stream order.
struct LaunchMaterials {
  StreamScratch tab, kdrep;
  const TriMat *mat = nullptr;
  int fill(GpuScene *s, const float **kd_dev, const float *ks_dev, const float *ke_dev, int sets, void *stream) {
    if (batch_kd(s, kd_dev, sets, (hipStream_t)stream, kdrep)) return -1;
    return pack_materials(s, ks_dev, ke_dev, sets, (hipStream_t)stream, tab, &mat);
  }
};

// The batched material launches' limit on the number of sets, checked before
// anything is enqueued.
static int check_sets(int n_scenes) {
  if (n_scenes > 65535) {  // pack_mat_kernel's blockIdx.y
    gpu_set_error("material overrides: at most 65535 material sets per launch");
    return -1;
  }
  return 0;
}

static int render_mat_impl(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                           const float *ke_dev, float *hdr_dev, uint8_t *ldr_dev, void *stream) {
  const int sets = p.nscenes > 1 ? p.nscenes : 1;
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, sets, stream)) return -1;
  return render_impl(s, p, kd_dev, hdr_dev, ldr_dev, stream, m.mat);
}

int gpu_render_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                   float *hdr_dev, uint8_t *ldr_dev, void *stream) {
  if (check_params(s, p)) return -1;
  if (p.nscenes > 1) {
    gpu_set_error("material overrides do not support the scene batch (n_scenes > 1)");
    return -1;
  }
  return render_mat_impl(s, p, kd_dev, ks_dev, ke_dev, hdr_dev, ldr_dev, stream);
}

// The scene batch of gpu_render_mat: kd / ks / ke are n_scenes*nT*3 (nullptr:
// the scene's own values in every set), hdr_dev n_scenes images; set b is
// gpu_render_mat with its arrays and seed + b * seed_stride, bit for bit.
int gpu_render_mat_batch(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                         const float *ke_dev, float *hdr_dev, void *stream) {
  if (check_params(s, p) || check_sets(p.nscenes)) return -1;
  // the forward's own bounce limit is the adjoint's: one contract for the pair
  if (p.max_bounces < 0 || p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("material batch: give max_bounces in 0..62 (the unbounded estimator is not supported; one material set: ipt_adjoint_mat_unbounded_dev)");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("material batch supports at most 65535 triangles");
    return -1;
  }
  return render_mat_impl(s, p, kd_dev, ks_dev, ke_dev, hdr_dev, nullptr, stream);
}

// ------------------------------------------------------------ adjoints
// The args of every adjoint launch: make_args, the pixel-major work order
// (DESIGN.md §12.10), and the gradient bins (all triangles in LDS, or the
// hot set of gpu_upload's grad_map).
static TraceArgs adjoint_args(const GpuScene *s, const RenderParams &p) {
  TraceArgs a = make_args(s, p);
  a.sample_major = 0;
  if (s->grad_map) {
    a.grad_slots = kLdsGradBytes / (3 * (int)sizeof(double));
    a.grad_map = s->grad_map;
    a.slot_tri = s->slot_tri;
  } else {
    a.grad_slots = s->host.nT;
  }
  return a;
}

// TraceArgs::rec_lds of an unbounded adjoint (kernel_of<MODE_ADJU, .., KIND>)
// whose LDS is `base` bytes plus `per` bytes per ring slot: up to
// IPT_ADJU_LDS_SLOTS (brute force) or IPT_ADJU_LDS_SLOTS_BVH slots, as many
// as cost no resident workgroup (searched for the brute-force instances and
// cached per scene for this base in *cached_base / *cached_nl); the
// rest of the ring lives in global memory (launch_inst sizes that part).
// At least 1: a lane's first record never waits for a pool chunk -- with none
// left it could not start its ring -- so a scene whose base leaves no room
// for one slot at full residency runs with one workgroup less; the callers
// refuse one that leaves no room for one slot at all.
template <int KIND>
static int ring_lds_slots(GpuScene *s, size_t base, size_t per, bool bvh, size_t *cached_base, int *cached_nl,
                          int *rec_lds) {
  int nl = bvh ? IPT_ADJU_LDS_SLOTS_BVH : IPT_ADJU_LDS_SLOTS;
  if (!bvh) {
    if (*cached_base != base) {
      auto occ = [&](size_t bytes, int *o) {
        return s->has_ks ? hipOccupancyMaxActiveBlocksPerMultiprocessor(o, kernel_of<MODE_ADJU, true, false, KIND>(), kBlock, bytes)
                         : hipOccupancyMaxActiveBlocksPerMultiprocessor(o, kernel_of<MODE_ADJU, false, false, KIND>(), kBlock, bytes);
      };
      int occ0 = 0, best = 0;
      HIP_TRY(occ(base, &occ0));
      for (int k = nl; k > 0 && best == 0; --k) {
        int o = 0;
        HIP_TRY(occ(base + k * per, &o));
        if (o >= occ0 && base + k * per <= IPT_ADJU_LDS_CAP) best = k;
      }
      *cached_base = base;
      *cached_nl = best;
    }
    nl = *cached_nl;
  }
  if (g_adju_lds.load() > 0) nl = g_adju_lds.load();
  *rec_lds = std::max(1, std::min(nl, kAdjuRing - 1));
  return 0;
}

// LDS bytes of a bounded material adjoint's workgroup: bins (Kd, Ks with a
// lobe, Ke per emitter) + tables + owner markers + vertex records
static size_t mat_adjoint_lds(const GpuScene *s, const TraceArgs &a) {
  const size_t fields = (size_t)(s->has_ks ? kRecFieldsSpec : kRecFieldsDiffuse);
  return mat_lds_doubles(a.grad_slots, s->host.nE, s->has_ks) * sizeof(double) + table_bytes(a) +
         (size_t)kBlock * sizeof(uint32_t) + (size_t)a.rec_cap * fields * kBlock * sizeof(float);
}

// dL/dKd, dL/dKs, dL/dKe in one launch of trace_mat_kernel (the bounded
// adjoint only); grad_dev: 3 x nT x 3 doubles [Kd | Ks | Ke], accumulated.
static int adjoint_mat_impl(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                            const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream,
                            const float *views_dev = nullptr, int view_sets = 0);
int gpu_adjoint_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                    const float *adj_dev, double *grad_dev, void *stream) {
  if (check_params(s, p)) return -1;
  if (p.nscenes > 1 && p.max_bounces >= 0) {  // (the unbounded refusal comes first, as it always did)
    gpu_set_error("material adjoint: the scene batch (n_scenes > 1) is not supported");
    return -1;
  }
  return adjoint_mat_impl(s, p, kd_dev, ks_dev, ke_dev, adj_dev, grad_dev, stream);
}

// The scene batch of gpu_adjoint_mat: grad_dev is n_scenes x 3 x nT x 3
// doubles [set][Kd | Ks | Ke][tri][c], accumulated; a workgroup holds one
// set's bins and tables, so the LDS limit is the single-set one.
int gpu_adjoint_mat_batch(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                          const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream) {
  if (check_params(s, p) || check_sets(p.nscenes)) return -1;
  return adjoint_mat_impl(s, p, kd_dev, ks_dev, ke_dev, adj_dev, grad_dev, stream);
}

// views_dev: the sets are views over ONE material set and one gradient (gpu_adjoint_views),
// or with view_sets > 0 the (material set, view) pairs of view_sets material
// sets and as many gradients (gpu_adjoint_views_batch)
static int adjoint_mat_impl(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                            const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream,
                            const float *views_dev, int view_sets) {
  if (p.max_bounces < 0) {
    gpu_set_error("material adjoint: the unbounded estimator (max_bounces < 0) is not supported here; give max_bounces in 0..62, or call ipt_adjoint_mat_unbounded_dev (one material set)");
    return -1;
  }
  if (p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("adjoint requires max_bounces <= 62 (vertex records live in LDS); -1 = unbounded");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("adjoint supports at most 65535 triangles");
    return -1;
  }
  const TraceArgs a = adjoint_args(s, p);
  const size_t lds = mat_adjoint_lds(s, a);
  if (lds > 160 * 1024) {
    gpu_set_error("material adjoint: LDS footprint (Kd/Ks/Ke bins + tables + vertex records) exceeds 160 KiB; lower max_bounces");
    return -1;
  }
  const int sets = view_sets > 0 ? view_sets : (p.nscenes > 1 && !views_dev) ? p.nscenes : 1;
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, sets, stream)) return -1;
  LaunchIO io;
  io.kd = kd_dev, io.adj = adj_dev, io.grad = grad_dev, io.mat = m.mat, io.views = views_dev, io.stream = (hipStream_t)stream;
  if (view_sets > 0) {
    io.nviews = p.nscenes / view_sets;
    return launch<MODE_ADJ, KIND_VBMAT>(s, a, lds, io);
  }
  return views_dev ? launch<MODE_ADJ, KIND_VMAT>(s, a, lds, io) : launch<MODE_ADJ, KIND_MATG>(s, a, lds, io);
}

// The tangent launch: the bounded material adjoint's launch
// with the tangent tables in the bins' place (tan_lds_doubles) and
// trace_tan_kernel; tan_dev is n_tangents x band pixels x 3 doubles,
// accumulated.  Everything is checked before anything is enqueued.
static int tangent_checks(const GpuScene *s, const RenderParams &p, int n_tangents, bool any_tangent, TraceArgs *args,
                          size_t *lds_bytes) {
  // (the call's own arguments first, the frame and the LDS footprint next,
  // the scene's device last: a host-only scene meets every refusal too)
  if (n_tangents < 1 || n_tangents > kMaxTangents) {
    gpu_set_error("material tangents: n_tangents must be in 1..16");
    return -1;
  }
  if (!any_tangent) {
    gpu_set_error("material tangents: give at least one of the tangent arrays tkd, tks, tke");
    return -1;
  }
  if (p.max_bounces < 0 || p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("material tangents: give max_bounces in 0..62 (the unbounded estimator is not supported)");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("material tangents support at most 65535 triangles");
    return -1;
  }
  if (check_frame(s, p)) return -1;
  if (p.nscenes > 1) {
    gpu_set_error("material tangents: the scene batch (n_scenes > 1) is not supported");
    return -1;
  }
  bool has_ks = s->has_ks;  // (gpu_upload's; a host-only scene: from its materials)
  if (!s->on_device)
    for (const TriMat &m : s->host.mat) has_ks |= (m.flags & MAT_HAS_KS) != 0;
  TraceArgs a = adjoint_args(s, p);
  const size_t fields = (size_t)(has_ks ? kRecFieldsSpec : kRecFieldsDiffuse);
  // The launch's bytes before the BVH carve-out, and with the least the BVH
  // instance adds behind them (launch_bvh_pick's last option: nothing
  // staged), so that a launch accepted here is resident.
  size_t lds = 0;
  auto footprint = [&]() {
    lds = tan_lds_doubles(n_tangents, s->host.nT, s->host.nE, has_ks, a.kd_tables != 0) * sizeof(double) + table_bytes(a) +
          (size_t)kBlock * sizeof(uint32_t) + (size_t)a.rec_cap * fields * kBlock * sizeof(float);
    if (!use_bvh(s)) return lds;
    TraceArgs c = a;
    return bvh_lds_offset(bvh_lds(s, c, lds, false, false));
  };
  // The tangent tables go with the kd tables (trace_body.h).  Where both do
  // not fit beside the vertex records, the launch leaves them in global
  // memory -- the path every scene past kMaxTableTris takes -- so that a scene
  // is never refused a K that a larger one gets.  What is
  // left then does not depend on n_tangents.
  size_t all = footprint();
  if (all > 160 * 1024 && a.kd_tables) {
    a.kd_tables = 0;
    all = footprint();
  }
  if (all > 160 * 1024) {
    gpu_set_error("material tangents: LDS footprint (tables + vertex records) exceeds 160 KiB; lower max_bounces");
    return -1;
  }
  if (check_device(s)) return -1;
  *args = a;
  *lds_bytes = lds;
  return 0;
}

int gpu_tangent_mat(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev, const float *ke_dev,
                    int n_tangents, const float *tkd_dev, const float *tks_dev, const float *tke_dev, double *tan_dev,
                    void *stream) {
  TraceArgs a;
  size_t lds = 0;
  if (tangent_checks(s, p, n_tangents, tkd_dev || tks_dev || tke_dev, &a, &lds)) return -1;
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, 1, stream)) return -1;
  LaunchIO io;
  io.kd = kd_dev, io.grad = tan_dev, io.mat = m.mat, io.stream = (hipStream_t)stream;
  io.tkd = tkd_dev, io.tks = tks_dev, io.tke = tke_dev, io.ntan = n_tangents;
  return launch<MODE_ADJ, KIND_TANG>(s, a, lds, io);
}

// ------------------------------------------------------------ views
struct GpuViews {
  GpuScene *scene = nullptr;
  int n = 0;
  std::vector<float> tab;  // n x kViewFloats: matrix, origin, padding
  float *dev = nullptr;    // the same on the device (nullptr: host-only scene)
};

float gpu_camera_bound(const GpuScene *s) { return (float)(scene_coord_bound(s->host) - 1.0); }

// Validated once, here: the launches take the table as it is.  The origin
// bound is the one the acceptance boxes, the pair culls and the plane margin
// were built for (bvh.cpp scene_coord_bound): they are exact
// for ray origins with |coordinate| + 1 <= R only.
GpuViews *gpu_views_create(GpuScene *s, int n, const float *cams) {
  if (n < 1 || n > 65535) {
    gpu_set_error("ipt_views_create: n_views must be in 1..65535");
    return nullptr;
  }
  const double R = scene_coord_bound(s->host);
  GpuViews *v = new GpuViews;
  v->scene = s;
  v->n = n;
  v->tab.assign((size_t)n * kViewFloats, 0.f);
  for (int b = 0; b < n; ++b) {
    const float *M = cams + 16 * (size_t)b;
    float *e = v->tab.data() + (size_t)b * kViewFloats;
    std::string why;
    for (int i = 0; i < 12 && why.empty(); ++i)
      if (!std::isfinite(M[i])) why = "a non-finite entry in rows 0..2";
    if (why.empty()) {
      const double det = (double)M[0] * ((double)M[5] * M[10] - (double)M[6] * M[9]) -
                         (double)M[1] * ((double)M[4] * M[10] - (double)M[6] * M[8]) +
                         (double)M[2] * ((double)M[4] * M[9] - (double)M[5] * M[8]);
      if (!(det != 0.0) || !std::isfinite(det)) why = "a 3x3 part with zero determinant";
    }
    std::memcpy(e, M, 16 * sizeof(float));
    camera_origin(M, e + 16);
    for (int i = 0; i < 3 && why.empty(); ++i)
      if (!(std::fabs((double)e[16 + i]) + 1.0 <= R))
        why = "its origin lies outside the bound the acceleration structures were built for (|component| <= " +
              std::to_string(R - 1.0) + ", ipt_scene_camera_bound)";
    if (!why.empty()) {
      gpu_set_error("ipt_views_create: view " + std::to_string(b) + " has " + why);
      delete v;
      return nullptr;
    }
  }
  if (s->on_device) {
    const size_t bytes = v->tab.size() * sizeof(float);
    if (hipMalloc(reinterpret_cast<void **>(&v->dev), bytes) != hipSuccess ||
        hipMemcpy(v->dev, v->tab.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
      gpu_set_error("ipt_views_create: the views' table could not be uploaded");
      if (v->dev) (void)hipFree(v->dev);
      delete v;
      return nullptr;
    }
  }
  return v;
}
void gpu_views_free(GpuViews *v) {
  if (!v) return;
  if (v->dev) (void)hipFree(v->dev);
  delete v;
}
int gpu_views_count(const GpuViews *v) { return v->n; }

// p.seed_stride is the caller's; the views are the launch's sets.
static int views_params(GpuScene *s, const GpuViews *v, RenderParams &p) {
  if (v->scene != s) {
    gpu_set_error("views: the handle was created for another scene");
    return -1;
  }
  p.nscenes = v->n;
  return check_params(s, p);
}

// One launch renders every view with ONE material set (kd / ks / ke: nT*3
// device arrays, nullptr = the scene's own); hdr_dev: V images.  View b is
// gpu_render_mat of its camera at seed + b * seed_stride, bit for bit.
int gpu_render_views(GpuScene *s, const GpuViews *v, RenderParams p, const float *kd_dev, const float *ks_dev,
                     const float *ke_dev, float *hdr_dev, void *stream) {
  if (views_params(s, v, p)) return -1;
  if (p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("views: give max_bounces in 0..62, or -1 for the unbounded estimator");
    return -1;
  }
  LaunchMaterials m;  // (one set: the caller's kd or the scene's own, as it is)
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, 1, stream)) return -1;
  return render_impl<KIND_VFWD>(s, p, kd_dev, hdr_dev, nullptr, stream, m.mat, v->dev);
}

// d(sum over views of sum adj_b * I_b)/d(Kd, Ks, Ke): ONE gradient of 3 x nT x 3
// doubles, accumulated, every workgroup flushing into it; adj_dev: V full frames.
static int views_adjoint_bounces(const RenderParams &p) {  // (checked first: a host-only scene reports it too)
  if (p.max_bounces < 0 || p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("views adjoint: give max_bounces in 0..62 (the bounded estimator; the unbounded material adjoint keeps the scene's own camera)");
    return -1;
  }
  return 0;
}
int gpu_adjoint_views(GpuScene *s, const GpuViews *v, RenderParams p, const float *kd_dev, const float *ks_dev,
                      const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream) {
  if (views_adjoint_bounces(p) || views_params(s, v, p)) return -1;
  return adjoint_mat_impl(s, p, kd_dev, ks_dev, ke_dev, adj_dev, grad_dev, stream, v->dev);
}

// ------------------------------------------------------------ views x material sets
// What both entry points refuse before anything is enqueued -- the argument
// checks first, so a host-only scene reports them too; the forward's bounce
// limit is the adjoint's (one contract for the pair, like the material batch).
static int view_sets_params(GpuScene *s, const GpuViews *v, RenderParams &p, int n_sets) {
  if (n_sets < 1) {
    gpu_set_error("views batch: n_sets must be >= 1");
    return -1;
  }
  if ((int64_t)n_sets * v->n > 65535) {
    gpu_set_error("views batch: at most 65535 (material set, view) pairs per launch (n_sets * n_views)");
    return -1;
  }
  if (p.max_bounces < 0 || p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("views batch: give max_bounces in 0..62 (the unbounded estimator is not supported)");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("views batch supports at most 65535 triangles");
    return -1;
  }
  if (v->scene != s) {
    gpu_set_error("views: the handle was created for another scene");
    return -1;
  }
  p.nscenes = n_sets * v->n;
  return check_params(s, p);
}

// One launch renders n_sets material sets through every view: kd / ks / ke
// are n_sets*nT*3 device arrays (nullptr: the scene's own values in every
// set), hdr_dev [n_sets][V] images.  Pair (m, b) is gpu_render_views' view b
// of set m's arrays at seed + (m * V + b) * seed_stride, bit for bit.
int gpu_render_views_batch(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                           const float *ks_dev, const float *ke_dev, float *hdr_dev, void *stream) {
  if (view_sets_params(s, v, p, n_sets)) return -1;
  // (the adjoint's LDS limit holds for the pair: refuse here what it would refuse)
  if (mat_adjoint_lds(s, adjoint_args(s, p)) > 160 * 1024) {
    gpu_set_error("views batch: LDS footprint (Kd/Ks/Ke bins + tables + vertex records) exceeds 160 KiB; lower max_bounces");
    return -1;
  }
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, n_sets, stream)) return -1;
  return render_impl<KIND_VBFWD>(s, p, kd_dev, hdr_dev, nullptr, stream, m.mat, v->dev, v->n);
}

// grad_dev: n_sets x 3 x nT x 3 doubles [set][Kd | Ks | Ke][tri][c],
// accumulated: the V * bps workgroups of a material set flush into its slice.
// adj_dev: [n_sets][V] full frames.
int gpu_adjoint_views_batch(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                            const float *ks_dev, const float *ke_dev, const float *adj_dev, double *grad_dev,
                            void *stream) {
  if (view_sets_params(s, v, p, n_sets)) return -1;
  return adjoint_mat_impl(s, p, kd_dev, ks_dev, ke_dev, adj_dev, grad_dev, stream, v->dev, n_sets);
}

// The rays of view `view` for n global sample indices (host arrays).
int gpu_views_rays_host(GpuScene *s, const GpuViews *v, int view, RenderParams p, int64_t n, const int64_t *index,
                        float *org, float *dir) {
  RenderParams q = p;
  if (views_params(s, v, q)) return -1;
  if (view < 0 || view >= v->n) {
    gpu_set_error("ipt_views_rays_host: view outside [0, n_views)");
    return -1;
  }
  const uint64_t total = (uint64_t)p.width * (uint64_t)p.height * (uint64_t)p.spp;
  for (int64_t i = 0; i < n; ++i)
    if (index[i] < 0 || (uint64_t)index[i] >= total) {
      gpu_set_error("ipt_views_rays_host: a sample index outside [0, width*height*spp)");
      return -1;
    }
  if (n <= 0) return 0;
  const TraceArgs a = make_args(s, p);  // rc_W, rc_H as the trace kernels get them
  struct Buf {
    void *p = nullptr;
    ~Buf() {
      if (p) (void)hipFree(p);
    }
  } ix, o, d;
  const size_t n3 = (size_t)n * 3 * sizeof(float);
  HIP_TRY(hipMalloc(&ix.p, (size_t)n * sizeof(int64_t)));
  HIP_TRY(hipMalloc(&o.p, n3));
  HIP_TRY(hipMalloc(&d.p, n3));
  HIP_TRY(hipMemcpy(ix.p, index, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(view_rays_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, v->dev,
                     view, p.width, p.height, p.spp, a.rc_W, a.rc_H, p.seed, n, (const int64_t *)ix.p, (float *)o.p,
                     (float *)d.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(org, o.p, n3, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(dir, d.p, n3, hipMemcpyDeviceToHost));
  return 0;
}

// The unbounded material adjoint's LDS in front of its ring slots, in the view
// sets' launch too (a workgroup holds one pair's bins, tables and carried
// words): bins (Kd, Ks with a lobe, Ke per emitter) + tables + the owners'
// carried words + owner markers; *per = one ring slot per lane.
static size_t matu_lds_base(const GpuScene *s, const TraceArgs &a, size_t *per) {
  *per = (size_t)(s->has_ks ? kRecFieldsSpec : kRecFieldsDiffuse) * kBlock * sizeof(float);
  return mat_lds_doubles(a.grad_slots, s->host.nE, s->has_ks) * sizeof(double) + table_bytes(a) +
         mat_carry_bytes(use_bvh(s)) + (size_t)kBlock * sizeof(uint32_t);
}

// The ring of an unbounded material adjoint (KIND_MATG, KIND_VBMAT) and the
// launch's LDS bytes: the slots in LDS are chosen as gpu_adjoint chooses them
// but for THIS kernel's occupancy, in the caller's own cache pair; a forced or
// default count the base leaves no room for shrinks to what fits (>= 1: the
// callers have refused a base with no room for one slot per lane).
template <int KIND>
static int matu_ring(GpuScene *s, TraceArgs &a, size_t *cached_base, int *cached_nl, size_t *lds) {
  size_t per = 0;
  const size_t base = matu_lds_base(s, a, &per);
  a.rec_cap = kAdjuRing;
  if (ring_lds_slots<KIND>(s, base, per, use_bvh(s), cached_base, cached_nl, &a.rec_lds)) return -1;
  a.rec_lds = (int)std::min<size_t>((size_t)a.rec_lds, (160 * 1024 - base) / per);
  *lds = base + (size_t)a.rec_lds * per;
  return 0;
}

// dL/dKd, dL/dKs, dL/dKe of the reference's own estimator (no bounce cap) in
// one launch of trace_matu_kernel: gpu_adjoint's unbounded
// launch with the material adjoint's bins, overrides and tri_emit map.
// grad_dev as gpu_adjoint_mat's.  One material set.
static int check_unbounded(const RenderParams &p) {
  if (p.max_bounces >= 0) {
    gpu_set_error("unbounded material adjoint: max_bounces must be -1 (no bounce cap); ipt_adjoint_mat_dev takes max_bounces in 0..62");
    return -1;
  }
  return 0;
}
int gpu_adjoint_mat_unbounded(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *ks_dev,
                              const float *ke_dev, const float *adj_dev, double *grad_dev, void *stream) {
  if (check_unbounded(p) || check_params(s, p)) return -1;
  if (p.nscenes > 1) {
    gpu_set_error("unbounded material adjoint: the scene batch (n_scenes > 1) is not supported");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("adjoint supports at most 65535 triangles");
    return -1;
  }
  TraceArgs a = adjoint_args(s, p);
  size_t per = 0, lds = 0;
  if (matu_lds_base(s, a, &per) + per > 160 * 1024) {  // no room for one slot per lane
    gpu_set_error("unbounded material adjoint: the Kd/Ks/Ke bins and the scene's LDS tables plus one record slot per lane exceed 160 KiB");
    return -1;
  }
  // (its bins are larger than the Kd-only adjoint's, so its slot count and cache are its own)
  if (matu_ring<KIND_MATG>(s, a, &s->matu_base, &s->matu_nl, &lds)) return -1;
  LaunchMaterials m;  // (one set)
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, 1, stream)) return -1;
  LaunchIO io;
  io.kd = kd_dev, io.adj = adj_dev, io.grad = grad_dev, io.mat = m.mat, io.stream = (hipStream_t)stream;
  return launch<MODE_ADJU, KIND_MATG>(s, a, lds, io);
}

// ------------------------------------------------------------ views x material sets, unbounded
// What both entry points refuse before anything is enqueued -- the argument
// checks first, so a host-only scene reports them too and itself last; the
// forward refuses what its adjoint refuses (one contract for the pair).
static int view_sets_unbounded_params(GpuScene *s, const GpuViews *v, RenderParams &p, int n_sets) {
  if (p.max_bounces >= 0) {
    gpu_set_error("unbounded views batch: max_bounces must be -1 (no bounce cap); ipt_render_views_batch_dev and ipt_adjoint_views_batch_dev take max_bounces in 0..62");
    return -1;
  }
  if (n_sets < 1) {
    gpu_set_error("unbounded views batch: n_sets must be >= 1");
    return -1;
  }
  if ((int64_t)n_sets * v->n > 65535) {
    gpu_set_error("unbounded views batch: at most 65535 (material set, view) pairs per launch (n_sets * n_views)");
    return -1;
  }
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("unbounded views batch supports at most 65535 triangles");
    return -1;
  }
  if (v->scene != s) {
    gpu_set_error("views: the handle was created for another scene");
    return -1;
  }
  p.nscenes = n_sets * v->n;
  if (check_params(s, p)) return -1;
  size_t per = 0;
  const size_t base = matu_lds_base(s, adjoint_args(s, p), &per);
  if (base + per > 160 * 1024) {  // no room for one slot per lane
    gpu_set_error("unbounded views batch: the Kd/Ks/Ke bins and the scene's LDS tables plus one record slot per lane exceed 160 KiB");
    return -1;
  }
  return 0;
}

// gpu_render_views_batch at max_bounces = -1: the view sets' forward kernels
// render unbounded as they are (gpu_render_views accepts -1 too); pair (m, b)
// is gpu_render_views' view b of set m's arrays at seed + (m * V + b) *
// seed_stride and -1, bit for bit.
int gpu_render_views_batch_unbounded(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                                     const float *ks_dev, const float *ke_dev, float *hdr_dev, void *stream) {
  if (view_sets_unbounded_params(s, v, p, n_sets)) return -1;
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, n_sets, stream)) return -1;
  return render_impl<KIND_VBFWD>(s, p, kd_dev, hdr_dev, nullptr, stream, m.mat, v->dev, v->n);
}

// gpu_adjoint_mat_unbounded over n_sets material sets x V views in one launch
// of trace_matu_views_batch_kernel: grad_dev n_sets x 3 x nT x 3 doubles
// [set][Kd | Ks | Ke][tri][c], accumulated; adj_dev [n_sets][V] full frames.
int gpu_adjoint_views_batch_unbounded(GpuScene *s, const GpuViews *v, RenderParams p, int n_sets, const float *kd_dev,
                                      const float *ks_dev, const float *ke_dev, const float *adj_dev,
                                      double *grad_dev, void *stream) {
  if (view_sets_unbounded_params(s, v, p, n_sets)) return -1;
  TraceArgs a = adjoint_args(s, p);
  size_t lds = 0;
  if (matu_ring<KIND_VBMAT>(s, a, &s->vbmatu_base, &s->vbmatu_nl, &lds)) return -1;
  LaunchMaterials m;
  if (m.fill(s, &kd_dev, ks_dev, ke_dev, n_sets, stream)) return -1;
  LaunchIO io;
  io.kd = kd_dev, io.adj = adj_dev, io.grad = grad_dev, io.mat = m.mat, io.views = v->dev, io.nviews = v->n;
  io.stream = (hipStream_t)stream;
  return launch<MODE_ADJU, KIND_VBMAT>(s, a, lds, io);
}

// Bounded adjoint launches of at least this many samples (all material sets)
// use MODE_ADJW: C2 (16.8 M) gains 2.7%, a C2 1/8 share (2.1 M) loses 4%.
#ifndef IPT_ADJW_MIN_SAMPLES
#define IPT_ADJW_MIN_SAMPLES (8ull << 20)
#endif
int gpu_adjoint(GpuScene *s, const RenderParams &p, const float *kd_dev, const float *adj_dev, double *grad_dev,
                void *stream) {
  if (check_params(s, p)) return -1;
  if (p.max_bounces > kMaxAdjBounces) {
    gpu_set_error("adjoint requires max_bounces <= 62 (vertex records live in LDS); -1 = unbounded");
    return -1;
  }
  const bool unbounded = p.max_bounces < 0;
  if (s->host.nT > kMaxAdjTris) {
    gpu_set_error("adjoint supports at most 65535 triangles");
    return -1;
  }
  TraceArgs a = adjoint_args(s, p);
  const size_t fields = (size_t)(s->has_ks ? kRecFieldsSpec : kRecFieldsDiffuse);
  const size_t per = fields * kBlock * sizeof(float);  // one vertex record (ADJU: ring slot) per lane
  // (the bounded adjoint may take the shading tables -- unless its records then no longer fit the CU's LDS)
  if (!unbounded) {
    shade_offer(s, a);
    if ((size_t)a.grad_slots * 3 * sizeof(double) + table_bytes(a) + (size_t)kBlock * sizeof(uint32_t) + (size_t)a.rec_cap * per >
        160 * 1024)
      a.small_pairs &= ~kSmallShade;
  }
  const size_t base = (size_t)a.grad_slots * 3 * sizeof(double) + table_bytes(a) +
                      (size_t)kBlock * sizeof(uint32_t);  // + the sweep's owner markers
  if (unbounded) {
    a.rec_cap = kAdjuRing;
    if (ring_lds_slots<KIND_TRACE>(s, base, per, use_bvh(s), &s->adju_base, &s->adju_nl, &a.rec_lds)) return -1;
  }
  const size_t lds = base + (size_t)(unbounded ? a.rec_lds : a.rec_cap) * per;
  if (lds > 160 * 1024) {
    gpu_set_error(unbounded ? "unbounded adjoint: the scene's LDS tables plus one record slot per lane exceed 160 KiB"
                            : "adjoint LDS footprint exceeds 160 KiB; lower max_bounces");
    return -1;
  }
  LaunchIO io;
  io.kd = kd_dev, io.adj = adj_dev, io.grad = grad_dev, io.stream = (hipStream_t)stream;
  if (unbounded) return launch<MODE_ADJU>(s, a, lds, io);
  // the 6-wave instance for full-size launches whose LDS leaves room for a
  // sixth workgroup per CU (IPT_ADJW=0/1 in the environment forces the choice)
  const size_t lane_words = kLaneWsBytes;  // MODE_ADJW's work item and Le in LDS (trace_kernel's lane_ws)
  bool wide = !use_bvh(s) && !s->has_ks && 6 * (lds + lane_words) <= 160 * 1024 &&
              (uint64_t)a.n_samples * (uint64_t)std::max(1, a.nscenes) >= IPT_ADJW_MIN_SAMPLES;
  if (const char *e = std::getenv("IPT_ADJW")) wide = std::atoi(e) != 0 && !use_bvh(s) && !s->has_ks;
  // (a sixth workgroup that only fits without the shading tables: launch<> then drops them)
  if (!wide && !std::getenv("IPT_ADJW") && !use_bvh(s) && !s->has_ks && 6 * (lds - shade_bytes(a) + lane_words) <= 160 * 1024 &&
      (uint64_t)a.n_samples * (uint64_t)std::max(1, a.nscenes) >= IPT_ADJW_MIN_SAMPLES)
    wide = true;
  if (wide) return launch<MODE_ADJW>(s, a, lds + lane_words, io);
  return launch<MODE_ADJ>(s, a, lds, io);
}

int gpu_graph(GpuScene *s, const RenderParams &p, const uint8_t *target_dev, double *acc_dev, void *stream) {
  if (check_params(s, p)) return -1;
  TraceArgs a = make_args(s, p);
  const size_t bins = graph_lds_doubles(s->host.nT, s->host.nE) * sizeof(double);
  a.lds_edges = bins <= (size_t)IPT_GRAPH_LDS_KB * 1024 ? 1 : 0;
  a.kd_tables = 0;  // the graph integrator never reads albedo
  a.sample_major = 0;  // pixel-major, as the adjoints (adjoint_args)
  LaunchIO io;
  io.target = target_dev, io.edges = acc_dev, io.stream = (hipStream_t)stream;
  return launch<MODE_GRAPH>(s, a, (a.lds_edges ? bins : 0) + table_bytes(a), io);
}

// ------------------------------------------------------------ math self-test
// Diagnostic for the exactness claims behind the in-range cores: each core is
// compared bitwise with the IEEE operation hipcc emits, over random operands
// drawn across the whole range the core is used in (and the guard boundaries
// of unit()).  counts[k] = mismatches of test k:
//   0 sqrt_core vs sqrtf          x in [2^-96, 2^127]
//   1 dsqrt_core vs sqrt (f64)    x in [2^-767, 2^1000]
//   2 div_inrange vs a/b          |a| in [2^-100, 2^60], |b| in [2^-60, 2^60], |a/b| in [2^-120, 2^120]
//   3 div_inrange, hit-test range |a| <= 2^20, |b| in [kMinDotUp, 1]
//   4 div3_core vs v/s            unit()'s fast-path operands
//   5 unit vs unit_ieee           vectors with zero / tiny / huge components (guard both ways)
//   6 fast-path hits of test 5    (not a mismatch: shows both paths were exercised)
//   7 camera division range       (2(c+u0))/W, c in [0, 2^16), W in [1, 2^16]
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float rand_exp_float(uint64_t r, int emin, int emax) {  // sign random
  const int e = emin + (int)((r >> 23) % (uint64_t)(emax - emin + 1));
  const uint32_t m = (uint32_t)r & 0x7fffffu;
  const uint32_t sgn = (uint32_t)(r >> 63) << 31;
  return __uint_as_float(sgn | ((uint32_t)(e + 127) << 23) | m);
}
__global__ __launch_bounds__(kBlock) void math_selftest_kernel(uint64_t n, uint64_t seed,
                                                               unsigned long long *counts) {
  unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint64_t r0 = mix64(seed ^ (i * 8 + 0)), r1 = mix64(seed ^ (i * 8 + 1)), r2 = mix64(seed ^ (i * 8 + 2));
    const uint64_t r3 = mix64(seed ^ (i * 8 + 3)), r4 = mix64(seed ^ (i * 8 + 4));
    {  // 0
      const float x = fabsf(rand_exp_float(r0, -96, 127));
      c[0] += __float_as_uint(sqrt_core(x)) != __float_as_uint(sqrtf(x));
    }
    {  // 1
      const int e = -767 + (int)((r1 >> 52) % 1768u);
      const double x = __longlong_as_double((long long)(((uint64_t)(e + 1023) << 52) | (r1 & 0xfffffffffffffull)));
      c[1] += __double_as_longlong(dsqrt_core(x)) != __double_as_longlong(sqrt(x));
    }
    {  // 2
      const float a = rand_exp_float(r2, -100, 60);  // nonzero: see div_inrange on zeros
      const float b = rand_exp_float(r3, -60, 60);
      const float q = a / b;
      if (fabsf(q) >= 0x1p-120f && fabsf(q) <= 0x1p120f)
        c[2] += __float_as_uint(div_inrange(a, b)) != __float_as_uint(q);
    }
    {  // 3
      const float a = rand_exp_float(r4, -40, 20);
      const float b = (r0 & 1 ? 1.f : -1.f) * (kMinDotUp + (1.f - kMinDotUp) * (float)(r3 >> 40) * 0x1p-24f);
      c[3] += __float_as_uint(div_inrange(a, b)) != __float_as_uint(a / b);
    }
    {  // 4, 5, 6
      V3 v;
      float comp[3];
      for (int k = 0; k < 3; ++k) {
        const uint64_t rk = mix64(r4 ^ (uint64_t)(k + 11));
        const int kind = (int)(rk & 15);
        if (kind == 0) comp[k] = 0.f;
        else if (kind == 1) comp[k] = (rk & 16) ? -0.f : 0.f;
        else if (kind == 2) comp[k] = rand_exp_float(rk, -149 + 23, -85);   // tiny: around the 2^-90 guard
        else if (kind == 3) comp[k] = rand_exp_float(rk, 25, 35);           // huge: around the 2^60 guard
        else if (kind == 4) comp[k] = rand_exp_float(rk, -6, -2);           // small: around the 2^-6 guard
        else comp[k] = rand_exp_float(rk, -30, 3);
      }
      v = mk(comp[0], comp[1], comp[2]);
      const V3 u = unit(v), w = unit_ieee(v);
      c[5] += (__float_as_uint(u.x) != __float_as_uint(w.x)) || (__float_as_uint(u.y) != __float_as_uint(w.y)) ||
              (__float_as_uint(u.z) != __float_as_uint(w.z));
      const float n2 = dot3(v, v);
      const uint32_t m = min(min((__float_as_uint(v.x) << 1) - 1u, (__float_as_uint(v.y) << 1) - 1u),
                             (__float_as_uint(v.z) << 1) - 1u);
      const bool fast = n2 >= 0x1p-6f && n2 <= 0x1p60f && m >= ((0x25u << 24) - 1u);
      c[6] += fast;
      if (fast) {
        const float sq = sqrtf(n2);
        const V3 q = div3_core(v, sq);
        c[4] += (__float_as_uint(q.x) != __float_as_uint(v.x / sq)) || (__float_as_uint(q.y) != __float_as_uint(v.y / sq)) ||
                (__float_as_uint(q.z) != __float_as_uint(v.z / sq));
      }
    }
    {  // 7
      const int W = 1 + (int)(r0 % 65536u), cc = (int)(r1 % (uint64_t)W);
      const float u0 = (float)(uint32_t)r2 * 2.3283064e-10f + 1.1641532e-10f;
      const float a = 2.f * ((float)cc + u0);
      c[7] += __float_as_uint(div_inrange(a, (float)W)) != __float_as_uint(a / (float)W);
    }
  }
  for (int k = 0; k < 8; ++k)
    if (c[k]) atomicAdd(&counts[k], c[k]);
}

int gpu_selftest_math(uint64_t n, uint64_t seed, uint64_t *counts_host) {
  unsigned long long *d = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), 8 * sizeof(unsigned long long)));
  int rc = 0;
  if (hipMemset(d, 0, 8 * sizeof(unsigned long long)) != hipSuccess) rc = -1;
  if (!rc) {
    hipLaunchKernelGGL(math_selftest_kernel, dim3(2048), dim3(kBlock), 0, 0, n, seed, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -1;
  }
  if (!rc && hipMemcpy(counts_host, d, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
  (void)hipFree(d);
  if (rc) gpu_set_error("math self-test failed to run");
  return rc;
}

// ------------------------------------------------------------ closest-hit probe
// The cast() of the megakernel on caller-supplied rays: one ray per thread,
// the same LDS staging (small-scene plane offsets, BVH nodes + stack).
// targets[i] >= 0 makes ray i a shadow ray towards that emitter triangle
// (the BVH and the small scenes' culled shadow cast then answer only "is the
// closest hit the target, and at which t"); targets[i] < 0 runs the
// megakernel's path cast (the culled one in small scenes); without targets
// the brute-force loop returns the full closest hit.  Used by the exactness tests of the
// BVH and of the shadow cull against the brute-force loop.
// Potential-occluder mask of a shadow ray from a vertex on triangle `src`
// towards emitter triangle `target` (all pairs when unknown: src outside
// [0, nT), or target not an emitter).
__device__ __forceinline__ uint32_t probe_allow(const uint32_t *masks, const int *emit_tri, int nE, int nT, int src,
                                                int target) {
  if (!masks || src < 0 || src >= nT) return 0xffffffffu;
  for (int e = 0; e < nE; ++e)
    if (emit_tri[e] == target) return masks[src * nE + e];
  return 0xffffffffu;
}

template <bool BVH>
__global__ __launch_bounds__(kBlock) void closest_hit_kernel(const TriIsect *__restrict__ isect,
                                                             const TriPair *__restrict__ pairs, const TraceArgs a,
                                                             int small, int64_t n, const float *__restrict__ org,
                                                             const float *__restrict__ dir,
                                                             const int *__restrict__ targets,
                                                             const int *__restrict__ sources,
                                                             const int *__restrict__ emit_tri, float *__restrict__ t_out,
                                                             int *__restrict__ i_out) {
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  const int nT = a.nT;
  const int nP = (nT + 1) >> 1;
  float *lds_e3 = reinterpret_cast<float *>(lds);
  const f2 *e3 = nullptr;
  if (small) {
    for (int i = tid; i < kE3Floats * nP; i += kBlock) lds_e3[i] = small_table_entry(pairs, i);
    e3 = reinterpret_cast<const f2 *>(lds_e3);
  }
  float *lds_pr = lds_e3 + kE3Floats * nP;  // the culled path cast's TriPair copy (!BVH, small), 16-B aligned
  lds_pr += (4 - (int)((lds_pr - lds_e3) & 3)) & 3;
  if (!BVH && small) {
    const float *gp = reinterpret_cast<const float *>(pairs);
    for (int i = tid; i < 36 * nP; i += kBlock) lds_pr[i] = gp[i];
  }
  BvhView bv;
  bv.isect = isect;
  bv.big = nullptr;
  bv.big_idx = nullptr;
  bv.big_e3 = nullptr;
  bv.nbig = 0;
  bv.big_boxes = nullptr;
  bv.big_lds = nullptr;
  bv.emit_is = nullptr;
  CoopView cv;
  cv.wn = a.bvh_wide;
  cv.wn_lds = false;
  cv.wt = a.bvh_wtris;
  cv.stk = nullptr;
  cv.stride = a.coop_stride;
  for (int k = 0; k < 6; ++k) cv.root[k] = a.root_box[k];
  for (int k = 0; k < 4; ++k) cv.sphere[k] = a.tree_sphere[k];
  if (BVH) {
    char *base = reinterpret_cast<char *>(lds);
    float4 *lw = reinterpret_cast<float4 *>(base + bvh_lds_offset((size_t)(small ? kE3Floats * nP : 0) * sizeof(float)));
    if (a.bvh_wide_lds > 0) {
      for (int i = tid; i < kWideF4 * a.bvh_wide_lds; i += kBlock) lw[i] = a.bvh_wide[i];
      cv.wn = lw;
      cv.wn_lds = true;
    }
    float *be3 = reinterpret_cast<float *>(lw + kWideF4 * a.bvh_wide_lds);
    for (int i = tid; i < 6 * a.bvh_nbig; i += kBlock) {
      const int j = i / 6, kf = (i % 6) >> 1, h = i & 1;
      be3[i] = a.bvh_big[j].f[9 + 4 * kf][h];
    }
    bv.big = a.bvh_big;
    bv.big_idx = a.bvh_big_idx;
    bv.big_boxes = a.bvh_big_boxes;
    bv.big_e3 = reinterpret_cast<const f2 *>(be3);
    bv.nbig = a.bvh_nbig;
    uint32_t *after = reinterpret_cast<uint32_t *>(
        big_lds_copy(a, be3 + 6 * a.bvh_nbig, reinterpret_cast<float *>(lds), tid, kBlock, bv));
    cv.stk = after + (tid >> 6) * 8 * a.coop_stride;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kBlock + tid;
  const bool valid = i < n;  // no early return: the cooperative cast needs the whole wave
  V3 p = mk(0.f, 0.f, 0.f), d = mk(0.f, 0.f, 1.f);
  int target = -1, src = -1;
  if (valid) {
    p = mk(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
    d = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    target = targets ? targets[i] : -1;
    src = sources ? sources[i] : -1;
    src = src < nT ? src : -1;
  }
  float t = 0.f;
  int h = -1;
  if (BVH) {
    bool qn = false;
    if (valid) {
      // the tree-entry culls (sphere, source plane) hold for the megakernel's
      // unit directions; a caller's ray of another length takes the box test
      // only, so the BVH answers the brute-force loop for any direction
      const bool unit = fabsf(dot3(d, d) - 1.f) <= 0x1p-20f;
      if (target >= 0) {
        const uint32_t allow = probe_allow(a.big_pomask, emit_tri, a.nE, nT, src, target);
        if (bvh_prepass<true>(bv, p, d, t, h, target, allow))
          qn = coop_root_test(cv, p, d, t, unit) && !tree_skip(a.src_cull, src, d, unit);
      } else {  // (a path ray with a source: the megakernel's bounce ray leaving that triangle)
        bvh_prepass<false>(bv, p, d, t, h, -1);
        qn = coop_root_test(cv, p, d, t, unit) && !tree_skip(a.src_cull, src, d, unit);
      }
    }
    coop_cast<false>(cv, qn && target < 0, p, d, t, h);
    coop_cast<true>(cv, qn && target >= 0, p, d, t, h);
  } else if (valid) {
    if (small && target >= 0) {  // the megakernel's shadow cast of small scenes
      h = shadow_hit_pairs_small((const lds_f32 *)lds_pr, pairs, a.pboxes, e3, nT, p, d,
                                 target, t, [&]() {
                                   return probe_allow(a.pomask, emit_tri, a.nE, nT, src, target);
                                 });
    } else if (small && targets && target < 0) {  // ... and its path cast
      h = closest_hit_pairs_culled((const lds_f32 *)lds_pr, a.pboxes, nT, p, d, t);
    } else {  // the full closest hit (brute-force pair loop)
      h = cast_bf(pairs, e3, nT, p, d, t);
    }
  }
  if (valid) {
    t_out[i] = t;
    i_out[i] = h;
  }
}

int gpu_set_accel(GpuScene *s, int mode) {
  if (mode != IPT_ACCEL_AUTO && mode != IPT_ACCEL_BRUTE && mode != IPT_ACCEL_BVH) {
    gpu_set_error("unknown acceleration mode");
    return -1;
  }
  if (mode == IPT_ACCEL_BVH && s->host.bvh_nodes.empty()) {
    gpu_set_error("scene has no BVH: " + s->host.bvh_status);
    return -1;
  }
  s->accel = mode;
  return 0;
}
int gpu_accel_in_use(const GpuScene *s) { return use_bvh(s) ? IPT_ACCEL_BVH : IPT_ACCEL_BRUTE; }

int gpu_closest_hit(GpuScene *s, int64_t n, const float *org_dev, const float *dir_dev, const int *targets_dev,
                    const int *sources_dev, float *t_dev, int *idx_dev, void *stream) {
  if (!s->on_device) {
    gpu_set_error("scene was loaded host-only (ipt_load_scene_host); it cannot be traced");
    return -1;
  }
  if (n <= 0) return 0;
  TraceArgs a = make_args_scene(s);
  const int small = s->host.nT <= 2 * kSmallPairs ? 1 : 0;
  const size_t base = small ? (size_t)kE3Floats * ((s->host.nT + 1) / 2) * sizeof(float) : 0;
  const int blocks = (int)((n + kBlock - 1) / kBlock);
  if (use_bvh(s)) {
    const size_t lds = bvh_lds(s, a, base);
    hipLaunchKernelGGL(closest_hit_kernel<true>, dim3(blocks), dim3(kBlock), lds, (hipStream_t)stream, s->isect,
                       s->pairs, a, small, n, org_dev, dir_dev, targets_dev, sources_dev, s->emit_tri, t_dev, idx_dev);
  } else {
    const size_t lds = base + (small ? 12 + (size_t)((s->host.nT + 1) / 2) * sizeof(TriPair) : 0);
    hipLaunchKernelGGL(closest_hit_kernel<false>, dim3(blocks), dim3(kBlock), lds, (hipStream_t)stream, s->isect,
                       s->pairs, a, small, n, org_dev, dir_dev, targets_dev, sources_dev, s->emit_tri, t_dev, idx_dev);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------ host wrappers
namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// The round trip of the adjoint and graph wrappers: `in` (n_in elements)
// uploaded, an accumulator of n_acc doubles zeroed, run(in_dev, acc_dev), the
// accumulator downloaded.
template <typename T, typename F>
int accumulate_host(const T *in, size_t n_in, double *acc, size_t n_acc, F run) {
  DevBuf i, a;
  HIP_TRY(hipMalloc(&i.p, n_in * sizeof(T)));
  HIP_TRY(hipMalloc(&a.p, n_acc * sizeof(double)));
  HIP_TRY(hipMemcpy(i.p, in, n_in * sizeof(T), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(a.p, 0, n_acc * sizeof(double)));
  if (run((const T *)i.p, (double *)a.p)) return -1;
  HIP_TRY(hipMemcpy(acc, a.p, n_acc * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
}  // namespace

int gpu_render_samples_host(GpuScene *s, const RenderParams &p, float *samples) {
  if (check_params(s, p)) return -1;
  const size_t n = (size_t)band_rows(p) * p.width * p.spp * 3;
  DevBuf b;
  HIP_TRY(hipMalloc(&b.p, std::max<size_t>(n, 1) * sizeof(float)));
  if (gpu_render_samples(s, p, nullptr, (float *)b.p, nullptr)) return -1;
  HIP_TRY(hipMemcpy(samples, b.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int gpu_render_host(GpuScene *s, const RenderParams &p, float *hdr, uint8_t *ldr) {
  if (check_params(s, p)) return -1;
  const size_t npix = (size_t)band_rows(p) * p.width;
  DevBuf h, l;
  HIP_TRY(hipMalloc(&h.p, std::max<size_t>(npix, 1) * 3 * sizeof(float)));
  if (ldr) HIP_TRY(hipMalloc(&l.p, std::max<size_t>(npix, 1) * 3));
  if (gpu_render(s, p, nullptr, (float *)h.p, (uint8_t *)l.p, nullptr)) return -1;
  HIP_TRY(hipMemcpy(hdr, h.p, npix * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (ldr) HIP_TRY(hipMemcpy(ldr, l.p, npix * 3, hipMemcpyDeviceToHost));
  return 0;
}

int gpu_adjoint_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad) {
  if (check_params(s, p)) return -1;
  const size_t na = (size_t)p.width * p.height * 3, ng = (size_t)s->host.nT * 3;
  return accumulate_host(adj, na, grad, ng, [&](const float *a, double *g) {
    return gpu_adjoint(s, p, nullptr, a, g, nullptr);
  });
}

int gpu_adjoint_mat_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad) {
  if (check_params(s, p)) return -1;
  const size_t na = (size_t)p.width * p.height * 3, ng = (size_t)s->host.nT * 9;
  return accumulate_host(adj, na, grad, ng, [&](const float *a, double *g) {
    return gpu_adjoint_mat(s, p, nullptr, nullptr, nullptr, a, g, nullptr);
  });
}

int gpu_tangent_mat_host(GpuScene *s, const RenderParams &p, int n_tangents, const float *tkd, const float *tks,
                         const float *tke, double *tan) {
  TraceArgs a;
  size_t lds = 0;
  if (tangent_checks(s, p, n_tangents, tkd || tks || tke, &a, &lds)) return -1;  // (before anything is allocated)
  const size_t nt = (size_t)n_tangents * s->host.nT * 3, nout = (size_t)n_tangents * band_rows(p) * p.width * 3;
  const float *host[3] = {tkd, tks, tke};
  DevBuf dev[3];
  for (int i = 0; i < 3; ++i) {
    if (!host[i]) continue;
    HIP_TRY(hipMalloc(&dev[i].p, nt * sizeof(float)));
    HIP_TRY(hipMemcpy(dev[i].p, host[i], nt * sizeof(float), hipMemcpyHostToDevice));
  }
  DevBuf out;
  HIP_TRY(hipMalloc(&out.p, std::max<size_t>(nout, 1) * sizeof(double)));
  HIP_TRY(hipMemset(out.p, 0, std::max<size_t>(nout, 1) * sizeof(double)));
  if (gpu_tangent_mat(s, p, nullptr, nullptr, nullptr, n_tangents, (const float *)dev[0].p, (const float *)dev[1].p,
                      (const float *)dev[2].p, (double *)out.p, nullptr))
    return -1;
  HIP_TRY(hipMemcpy(tan, out.p, nout * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int gpu_adjoint_mat_unbounded_host(GpuScene *s, const RenderParams &p, const float *adj, double *grad) {
  if (check_unbounded(p) || check_params(s, p)) return -1;
  const size_t na = (size_t)p.width * p.height * 3, ng = (size_t)s->host.nT * 9;
  return accumulate_host(adj, na, grad, ng, [&](const float *a, double *g) {
    return gpu_adjoint_mat_unbounded(s, p, nullptr, nullptr, nullptr, a, g, nullptr);
  });
}

int gpu_render_views_host(GpuScene *s, const GpuViews *v, const RenderParams &p, float *hdr) {
  RenderParams q = p;
  if (views_params(s, v, q)) return -1;
  const size_t n = (size_t)v->n * band_rows(p) * p.width * 3;
  DevBuf h;
  HIP_TRY(hipMalloc(&h.p, std::max<size_t>(n, 1) * sizeof(float)));
  if (gpu_render_views(s, v, p, nullptr, nullptr, nullptr, (float *)h.p, nullptr)) return -1;
  HIP_TRY(hipMemcpy(hdr, h.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int gpu_adjoint_views_host(GpuScene *s, const GpuViews *v, const RenderParams &p, const float *adj, double *grad) {
  RenderParams q = p;
  if (views_adjoint_bounces(p) || views_params(s, v, q)) return -1;
  const size_t na = (size_t)v->n * p.width * p.height * 3, ng = (size_t)s->host.nT * 9;
  return accumulate_host(adj, na, grad, ng, [&](const float *a, double *g) {
    return gpu_adjoint_views(s, v, p, nullptr, nullptr, nullptr, a, g, nullptr);
  });
}

int gpu_closest_hit_host(GpuScene *s, int64_t n, const float *org, const float *dir, const int *targets,
                         const int *sources, float *t, int *idx) {
  if (n <= 0) return 0;
  DevBuf o, d, g, sr, tt, ii;
  const size_t n3 = (size_t)n * 3 * sizeof(float);
  HIP_TRY(hipMalloc(&o.p, n3));
  HIP_TRY(hipMalloc(&d.p, n3));
  HIP_TRY(hipMalloc(&tt.p, (size_t)n * sizeof(float)));
  HIP_TRY(hipMalloc(&ii.p, (size_t)n * sizeof(int)));
  HIP_TRY(hipMemcpy(o.p, org, n3, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.p, dir, n3, hipMemcpyHostToDevice));
  if (targets) {
    HIP_TRY(hipMalloc(&g.p, (size_t)n * sizeof(int)));
    HIP_TRY(hipMemcpy(g.p, targets, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  }
  if (sources) {
    HIP_TRY(hipMalloc(&sr.p, (size_t)n * sizeof(int)));
    HIP_TRY(hipMemcpy(sr.p, sources, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  }
  if (gpu_closest_hit(s, n, (const float *)o.p, (const float *)d.p, (const int *)g.p, (const int *)sr.p,
                      (float *)tt.p, (int *)ii.p, nullptr))
    return -1;
  HIP_TRY(hipMemcpy(t, tt.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(idx, ii.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int gpu_graph_host(GpuScene *s, const RenderParams &p, const uint8_t *target, double *acc) {
  if (check_params(s, p)) return -1;
  const size_t nt = (size_t)p.width * p.height * 3;
  const size_t nb = (size_t)(s->host.nT + 1) * s->host.nT * kEdgeW;
  return accumulate_host(target, nt, acc, nb, [&](const uint8_t *t, double *e) { return gpu_graph(s, p, t, e, nullptr); });
}

}  // namespace ipt
