// trace_body.h -- the body shared by every trace kernel of ipt_hip.hip,
// included INSIDE each __global__ entry point (no include guard: it is
// included once per kernel).  Text inclusion, not a device function: a
// force-inlined function template taking the launch arguments changed the
// register allocation and scratch of the BVH instances of trace_kernel.
// The including kernel provides, as template parameters or constexpr locals,
// MODE, SPEC, BVH and MATG (the material adjoint: an adjoint -- bounded,
// DESIGN.md §13, or unbounded, §16 -- whose sweep also emits dL/dKs and
// dL/dKe) and MATB (a forward whose
// scene batch has one TriMat table per set), the parameters of
// TraceKernArgs under their names, and tri_emit (MATG: triangle -> emitter
// index or -1; nullptr otherwise), and VIEWS (the sets of the grid split are
// cameras over one material set, DESIGN.md §18: the view kernels' trailing
// parameter is the views' table, read by its kernarg offset), and VSETS (with
// VIEWS: the sets are (material set, view) pairs, DESIGN.md §20 -- the view
// count V follows the table as one more trailing parameter), and SHADE (the
// small scenes' shading tables in LDS, DESIGN.md §23: trace_shade_kernel),
// and TANG (with MATG at MODE_ADJ: the sweep's terms go, times the tangents'
// entries of their bins, into per-pixel tangent images instead of the
// gradient bins, DESIGN.md §24 -- trace_tan_kernel, whose trailing parameters
// after tri_emit are the three tangent arrays and their count).
  extern __shared__ double lds[];
  const int tid = threadIdx.x;
  // scene batch: this workgroup's material set and its place among the set's blocks
  const int set = a.nscenes > 1 ? (int)(blockIdx.x % (uint32_t)a.nscenes) : 0;
  const uint32_t sblock = a.nscenes > 1 ? blockIdx.x / (uint32_t)a.nscenes : blockIdx.x;
  const uint32_t sgrid = a.nscenes > 1 ? (uint32_t)a.bps : gridDim.x;
  const uint64_t seed = a.seed + (uint64_t)set * a.seed_stride;
  // VSETS: launch set `set` of S * V is material set set / V seen through view
  // set % V (wave-uniform, once per workgroup).  Seed, image, adjoint image,
  // grab counter and bps stay keyed by `set`; kd, mat, kd/pi and the gradient
  // go by mset, the camera by view.
  int mset = 0, view = set;
  if (VSETS) {
    const int nviews = karg<int>(sizeof(TraceKernArgs) + (MATG ? sizeof(void *) : 0) + sizeof(const float *));
    mset = set / nviews;
    view = set - mset * nviews;
  }
  if (a.nscenes > 1) {
    // (VIEWS: the sets are views of ONE material set -- kd, mat, kd/pi and the
    // gradient carry no per-set offset)
    if (!VIEWS) kd += (size_t)set * 3 * a.nT;
    else if (VSETS) kd += (size_t)mset * 3 * a.nT;
    // per-set TriMat tables (0: one table for every set): the material
    // adjoint, and the forward instances of the material overrides' batch
    if (!VIEWS && (MATG || MATB)) mat += (size_t)set * a.mat_stride;
    else if (VSETS) mat += (size_t)mset * a.mat_stride;
    if (is_fwd<MODE>()) out_samples += (size_t)set * a.out_stride;
    // (adj, grad: karg() at their uses, offset there; a set's gradient is
    // 3 nT doubles, or with MATG its [Kd | Ks | Ke] slice of 9 nT)
  }
  const float *kdpi_g = a.kdpi_g ? a.kdpi_g + (VIEWS ? (VSETS ? (size_t)mset * 3 * a.nT : (size_t)0) : (size_t)set * 3 * a.nT) : nullptr;
  constexpr int nthr = kBlock;
  const int nT = a.nT, nE = a.nE;
  const int vmax = a.rec_cap;  // ADJ record capacity per lane (ADJU: ring slots)
  // SHADE (trace_shade_kernel; small scenes with <= kShadeMaxEmit emitters):
  // the shading tables (scene_layout.h) -- the emitters' CDF, a
  // TriShade record per triangle and for the camera, an EmitShade record per
  // emitter -- at the front of the workgroup's LDS, so that their addresses
  // are constants plus the record's offset and no base is held through the
  // trace loop.  The host launches a SHADE instance exactly when it has set
  // TraceArgs::small_pairs bit 1 and added the bytes (launch<>, table_bytes).
  // the emitter's triangle: taken with its vertices and held to the shadow
  // cast, or (the six-wave adjoint and the Phong per-sample forward, which it
  // would push to 16 B of scratch per lane) read again from the record in
  // front of the cast
  constexpr bool kEtEarly = !(MODE == MODE_ADJW || (MODE == MODE_FWD && SPEC));
  float *lds_sh = reinterpret_cast<float *>(lds);
  // LDS: [shading tables][fp64 accumulators][kd table][kd/pi table][ADJ vertex records]
  double *lds_acc = lds;               // ADJ: nT*3 grad; GRAPH: (nT+1)*nT*kEdgeW bins
  if (SHADE) lds_acc += shade_table_words(nT, nE) / 2;
  int n_acc = 0;
  if (is_adj<MODE>()) {
    n_acc = a.grad_slots * 3;
    // material adjoint: [Kd slots][Ks slots (SPEC)][Ke by emitter index] (mat_lds_doubles)
    if (MATG) n_acc = (int)mat_lds_doubles(a.grad_slots, nE, SPEC);
    // the tangent launch has no bins: its tangent tables take their place
    if (TANG) n_acc = (int)tan_lds_doubles(karg<int>(sizeof(TraceKernArgs) + 4 * sizeof(void *)), nT, nE, SPEC, a.kd_tables != 0);
  } else if (MODE == MODE_GRAPH && a.lds_edges) {
    n_acc = (int)graph_lds_doubles(nT, nE);
  }
  // Per-triangle kd and kd/pi (the latter is BSDF's indirect `diffuse /=
  // M_PI`, path_trace.cu:15-17): computed once per workgroup with the same
  // IEEE division the per-vertex code would do, instead of three divisions
  // per vertex.  Falls back to global memory for large scenes.
  float *tab = reinterpret_cast<float *>((SHADE ? lds_acc : lds) + n_acc);
  if (a.kd_tables) {
    for (int i = tid; i < 3 * nT; i += nthr) {
      const float v = kd[i];
      tab[i] = v;
      tab[3 * nT + i] = v / kPiF;
    }
  }
  // kd and kd/pi of triangle t, from the tables or from global memory by a
  // wave-uniform branch (a pointer that may point at either compiles to flat
  // loads: vector-memory latency and a vmcnt+lgkmcnt wait for LDS data)
  const lds_f32 *tab_l = (const lds_f32 *)tab;
  const gbl_f32 *kd_g = (const gbl_f32 *)kd;
  auto kd3 = [&](int t) -> V3 {
    if (a.kd_tables) return mk(tab_l[3 * t], tab_l[3 * t + 1], tab_l[3 * t + 2]);
    return mk(kd_g[3 * t], kd_g[3 * t + 1], kd_g[3 * t + 2]);
  };
  auto kdpi3 = [&](int t) -> V3 {
    if (a.kd_tables) return mk(tab_l[3 * nT + 3 * t], tab_l[3 * nT + 3 * t + 1], tab_l[3 * nT + 3 * t + 2]);
    const gbl_f32 *q = (const gbl_f32 *)kdpi_g + 3 * t;
    return mk(q[0], q[1], q[2]);
  };
  // edge-plane offsets of each triangle pair for the unrolled small-scene
  // closest-hit loop (ipt_device.h::closest_hit_pairs_small)
  const f2 *e3 = nullptr;
  float *lds_e3 = tab + (a.kd_tables ? 6 * nT : 0);
  const int nP = (nT + 1) >> 1;
  if (a.small_pairs) {
    for (int i = tid; i < kE3Floats * nP; i += nthr) lds_e3[i] = small_table_entry(pairs, i);
    e3 = reinterpret_cast<const f2 *>(lds_e3);
  }
  // small scenes, culled path cast: a copy of the TriPair records (16-B
  // aligned), gathered per lane
  float *const e3_end = lds_e3 + (a.small_pairs ? kE3Floats * nP : 0);
  float *lds_pr = e3_end + ((4 - (int)((e3_end - reinterpret_cast<float *>(lds)) & 3)) & 3);
  if (a.small_pairs) {
    const float *g = reinterpret_cast<const float *>(pairs);
    for (int i = tid; i < 36 * nP; i += nthr) lds_pr[i] = g[i];
  }
  // ... and the shadow casts' potential-occluder masks
  uint32_t *lds_po = reinterpret_cast<uint32_t *>(lds_pr + (a.small_pairs ? 36 * nP : 0));
  const bool po = a.small_pairs && a.pomask;
  if (po)
    for (int i = tid; i < nT * nE; i += nthr) lds_po[i] = a.pomask[i];
  if (SHADE) {  // the shading tables' fill
    uint32_t *w = reinterpret_cast<uint32_t *>(lds_sh);
    const uint32_t *gw = reinterpret_cast<const uint32_t *>(geom), *mw = reinterpret_cast<const uint32_t *>(mat);
    constexpr int GW = sizeof(TriGeom) / 4, MW = sizeof(TriMat) / 4;
    for (int i = tid; i < kShadeCdfWords; i += nthr) w[i] = i < nE ? __float_as_uint(emit_cdf[i]) : 0x7fc00000u;
    w += kShadeCdfWords;
    for (int i = tid; i < (nT + 1) * kTriShadeWords; i += nthr) {
      const int t = i / kTriShadeWords, f = i % kTriShadeWords;
      w[t * kTriShadeStride + f] = tri_shade_word(gw + (size_t)t * GW, t < nT ? mw + (size_t)t * MW : nullptr, f);
    }
    w += (nT + 1) * kTriShadeStride;
    for (int i = tid; i < nE * kEmitShadeWords; i += nthr) {
      const int e = i / kEmitShadeWords, f = i % kEmitShadeWords, t = emit_tri[e];
      w[e * kEmitShadeStride + f] = emit_shade_word(gw + (size_t)t * GW, mw + (size_t)t * MW, t, emit_pmf[e], a.emit_pmfr[e], f);
    }
  }
  const lds_f32 *cdf_l = (const lds_f32 *)lds_sh;
  const lds_f32 *tsh = cdf_l + kShadeCdfWords;                    // TriShade of triangle t at tsh + t * kTriShadeStride
  const lds_f32 *esh = tsh + (nT + 1) * kTriShadeStride;          // EmitShade of emitter e at esh + e * kEmitShadeStride
  float *lds_rec = a.small_pairs ? reinterpret_cast<float *>(lds_po) + (po ? nT * nE : 0) : lds_e3;
  auto ke3 = [&](int t) -> V3 {  // TriMat::ke
    if (SHADE) {
      const lds_f32 *r = tsh + t * kTriShadeStride + TS_KE;
      return mk(r[0], r[1], r[2]);
    }
    const gbl_f32 *q = (const gbl_f32 *)mat + (size_t)t * (sizeof(TriMat) / sizeof(float)) + offsetof(TriMat, ke) / sizeof(float);
    return mk(q[0], q[1], q[2]);
  };
  // the unbounded material adjoint, brute force (96 VGPRs): the owner lane's
  // carried state -- Scar, Mlo, the path's first triangle and the work item,
  // each touched once per chunk -- in kCarryWords LDS words per lane instead of registers
  // (mat_carry_bytes on the host side)
  constexpr bool kCarryLds = MATG && MODE == MODE_ADJU && !BVH;
  lds_u32 *carry_ws = nullptr;
  if (kCarryLds) {
    carry_ws = (lds_u32 *)lds_rec;
    lds_rec += kCarryWords * kBlock;
  }
  // MODE_ADJ: one word per lane (the sweep's owner markers) in front of the
  // vertex records
  if (is_adj<MODE>()) lds_rec += kBlock;
  BvhView bv;
  bv.isect = isect;
  bv.big = nullptr;
  bv.big_idx = nullptr;
  bv.big_e3 = nullptr;
  bv.nbig = 0;
  bv.big_boxes = nullptr;
  bv.big_lds = nullptr;
  bv.emit_is = nullptr;
  // BVH forward (5 waves/SIMD, 96 VGPRs): the lane's work item, the triangle
  // its path ray leaves and its first emission Le live in LDS ([6][kBlock]
  // words: item lo, hi, source, Le xyz) instead of registers -- each is
  // touched a few times per path, and in registers the allocator spilled them
  // (and more) to scratch inside the loop
  // The 6-wave adjoint (MODE_ADJW, 80 VGPRs) likewise keeps its work item
  // and Le there (its path source is not needed): in registers they pushed
  // the culled path cast past 80 VGPRs and a ray-direction pair was reloaded
  // from scratch in every pair block (16 B/lane of scratch)
  constexpr bool kLaneLds = (BVH && is_fwd<MODE>()) || (!BVH && MODE == MODE_ADJW);
  lds_u32 *lane_ws = nullptr;
  if (!BVH && kLaneLds)  // after the vertex records ([6][kBlock] words, as the BVH forward's)
    lane_ws = (lds_u32 *)(lds_rec + (size_t)vmax * kRecFieldsDiffuse * kBlock);
  CoopView cv;
  cv.wn = nullptr;
  cv.wn_lds = false;
  cv.wt = a.bvh_wtris;
  cv.stk = nullptr;
  cv.stride = a.coop_stride;
  for (int k = 0; k < 6; ++k) cv.root[k] = a.root_box[k];
  for (int k = 0; k < 4; ++k) cv.sphere[k] = a.tree_sphere[k];
  if (BVH) {
    const size_t rec_words = is_badj<MODE>()    ? (size_t)vmax * (SPEC ? kRecFieldsSpec : kRecFieldsDiffuse) * kBlock
                             : MODE == MODE_ADJU ? (size_t)a.rec_lds * (SPEC ? kRecFieldsSpec : kRecFieldsDiffuse) * kBlock
                                                 : 0;
    char *base = reinterpret_cast<char *>(lds);
    const size_t off = bvh_lds_offset((size_t)(reinterpret_cast<char *>(lds_rec + rec_words) - base));
    float4 *lw = reinterpret_cast<float4 *>(base + off);
    cv.wn = a.bvh_wide;
    if (a.bvh_wide_lds > 0) {
      for (int i = tid; i < kWideF4 * a.bvh_wide_lds; i += nthr) lw[i] = a.bvh_wide[i];
      cv.wn = lw;
      cv.wn_lds = true;
    }
    float *be3 = reinterpret_cast<float *>(lw + kWideF4 * a.bvh_wide_lds);
    for (int i = tid; i < 6 * a.bvh_nbig; i += nthr) {
      const int j = i / 6, kf = (i % 6) >> 1, h = i & 1;
      be3[i] = a.bvh_big[j].f[9 + 4 * kf][h];
    }
    bv.big = a.bvh_big;
    bv.big_idx = a.bvh_big_idx;
    bv.big_boxes = a.bvh_big_boxes;
    bv.big_e3 = reinterpret_cast<const f2 *>(be3);
    bv.nbig = a.bvh_nbig;
    float *after = big_lds_copy(a, be3 + 6 * a.bvh_nbig, reinterpret_cast<float *>(lds), tid, nthr, bv);
    if (emit_lds_bytes(nE)) {
      for (int i = tid; i < 20 * nE; i += nthr) after[i] = reinterpret_cast<const float *>(isect)[20 * emit_tri[i / 20] + i % 20];
      bv.emit_is = after;
      after += 20 * nE;
    }
    cv.stk = reinterpret_cast<uint32_t *>(after) + (tid >> 6) * 8 * a.coop_stride;
    if (kLaneLds) lane_ws = (lds_u32 *)(reinterpret_cast<uint32_t *>(after) + (kBlock / 64) * 8 * a.coop_stride);
  }
  if (!TANG)
    for (int i = tid; i < n_acc; i += nthr) lds_acc[i] = 0.0;
  // TANG: the tangents (trailing parameters: tkd, tks, tke, each ntan x nT x 3
  // floats or nullptr = zero; then ntan).  Small scenes stage them here as
  // [k][tri] Kd rows, (SPEC) [k][tri] Ks rows -- zero off the lobe mask, whose
  // rows are never read -- and [k][emitter] Ke rows (only emitters' rows are read)
  const int ntan = TANG ? karg<int>(sizeof(TraceKernArgs) + 4 * sizeof(void *)) : 0;
  if (TANG && a.kd_tables) {
    const float *tkd_p = karg<const float *>(sizeof(TraceKernArgs) + sizeof(void *));
    const float *tks_p = karg<const float *>(sizeof(TraceKernArgs) + 2 * sizeof(void *));
    const float *tke_p = karg<const float *>(sizeof(TraceKernArgs) + 3 * sizeof(void *));
    float *tt = reinterpret_cast<float *>(lds_acc);
    const int nk = ntan * nT * 3;
    for (int i = tid; i < nk; i += nthr) tt[i] = tkd_p ? tkd_p[i] : 0.f;
    if (SPEC)
      for (int i = tid; i < nk; i += nthr)
        tt[nk + i] = (tks_p && (mat[(i / 3) % nT].flags & MAT_HAS_KS)) ? tks_p[i] : 0.f;
    float *te = tt + (SPEC ? 2 : 1) * nk;
    for (int i = tid; i < ntan * nE * 3; i += nthr) {
      const int kq = i / (3 * nE), r = i - kq * 3 * nE;
      te[i] = tke_p ? tke_p[((size_t)kq * nT + emit_tri[r / 3]) * 3 + r % 3] : 0.f;
    }
  }
  __syncthreads();
  // fp64 bin updates go to LDS (ds_add_f64) or to global memory by a
  // wave-uniform (GRAPH) or per-lane (ADJ hot set) branch -- never through
  // one pointer that may be either: that compiles to flat atomics, which take
  // the vector-memory path even when the address is in LDS.
  // The pointers carry their address space in the type so that LLVM cannot
  // merge the two branches' atomics back into one through a selected pointer.
  auto bins_add = [&](bool in_lds, double *glob, size_t off, int n, const double *v) {
    if (in_lds) {
      lds_f64 *b = (lds_f64 *)lds_acc + off;
      for (int i = 0; i < n; ++i) __hip_atomic_fetch_add(b + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      gbl_f64 *b = (gbl_f64 *)glob + off;
      for (int i = 0; i < n; ++i) __hip_atomic_fetch_add(b + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };

  // MODE_ADJU: the ring's global slots (TraceArgs::grec): this wave's pool of
  // pool_chunks chunks, [chunk][slot][field], a record's fields contiguous --
  // one 12-B store per vertex, and a sweep round reads an owner's consecutive
  // records as contiguous runs.  Round 4's first form, [field][slot][lane],
  // stored 4 B per field at a different place per lane: three write requests
  // per vertex, 767 MB written per C3 launch, profiles/r04/unbounded_pmc_r04l.txt)
  gbl_f32 *upool = nullptr;  // this wave's chunk pool ([chunk][slot][field])
  if (MODE == MODE_ADJU)
    upool = (gbl_f32 *)a.grec + ((size_t)blockIdx.x * (kBlock / 64) + (tid >> 6)) * a.grec_stride;
  gbl_f32 *umr = nullptr;  // this lane's captured prefix throughputs (IPT_ADJU_SUB), entry e at umr + e * 192
  if (MODE == MODE_ADJU && kSub > 0)
    umr = (gbl_f32 *)a.mring + ((size_t)blockIdx.x * (kBlock / 64) + (tid >> 6)) * (kMrEnt * 64 * 3) + (tid & 63) * 3;
  {  // the wave's persistent loop
  // wave-uniform sample range (static partition, regenerated per lane)
  const uint32_t wave = __builtin_amdgcn_readfirstlane((sblock * kBlock + tid) >> 6);
  const uint32_t nwaves = (sgrid * kBlock) >> 6;
  const TraceArgs &ar = a;
  // Work items w in [0, n_samples) of this launch (item_split): pixel-major
  // w = lp * spp + s, or sample-major w = s * npix + lp over the launch's
  // pixels lp.  Either way the sample's seed is seed + its global index g:
  // results do not depend on the enumeration or on the row partition.
  // Which wave traces which items only changes WHO computes a sample, never
  // its value.  Static ranges leave the launch's tail to the waves whose
  // pixels hold the longest paths; chunks taken from a per-launch counter
  // keep every wave busy to the end.
  const bool dyn = a.chunk != 0;
  uint64_t next, end;
  if (dyn) {
    chunk_range<kGuided<BVH>()>(ar, wave, ar.n_samples, next, end);
  } else {
    next = (ar.n_samples * wave) / nwaves;
    end = (ar.n_samples * (wave + 1)) / nwaves;
  }
  bool exhausted = !dyn;
  // fused pixel mean (MODE_FWDM), wave-uniform: the current group's first
  // launch-local pixel glp, pixel count gnp and slots gslots (4 bits per
  // pixel), fj = its samples issued so far (item j = sample j / gnp of pixel
  // glp + j % gnp: sample-major inside the group); sfree / sdone = the ring's
  // free slots / slots whose samples are all in but not yet summed.  A slot
  // is held by ONE pixel, so a long path keeps one pixel's slot, not a whole
  // chunk's: the ring also serves unbounded paths.
  uint32_t glp = 0, gnp = 0, gslots = 0, fj = 0, sdone = 0;
  uint64_t pl0 = 0, pl1 = 0;  // the grabbed chunk's pixels not yet in a group
  uint32_t sfree = MODE == MODE_FWDM ? (a.nslots >= 32 ? ~0u : (1u << a.nslots) - 1u) : 0u;
  bool started = false;

  bool active = false;
  Rng st;
  V3 p = mk(0.f, 0.f, 0.f), d = p;
  V3 L = p, Le_r = p, Ld = p, M = mk(1.f, 1.f, 1.f);
  // Le: the path's first emission (kLaneLds: in LDS words 3..5 of lane_ws)
  auto set_le = [&](V3 v) {
    if (kLaneLds) {
      ((lds_f32 *)lane_ws)[3 * kBlock + tid] = v.x;
      ((lds_f32 *)lane_ws)[4 * kBlock + tid] = v.y;
      ((lds_f32 *)lane_ws)[5 * kBlock + tid] = v.z;
    } else {
      Le_r = v;
    }
  };
  auto le = [&]() -> V3 {
    if (kLaneLds)
      return mk(((lds_f32 *)lane_ws)[3 * kBlock + tid], ((lds_f32 *)lane_ws)[4 * kBlock + tid],
                ((lds_f32 *)lane_ws)[5 * kBlock + tid]);
    return Le_r;
  };
  // ADJU (unbounded adjoint): suffix carried from the chunk after, replay
  // target (0 = first pass), next ring slot
  // and the prefix throughput at the chunk's first vertex (1 for a chunk
  // starting at vertex 0; captured while a replay passes its start)
  V3 Scar = mk(0.f, 0.f, 0.f), Mlo = mk(1.f, 1.f, 1.f);
  int rhi = 0, rslot = 0;
  // the unbounded material adjoint: the path's first triangle, kept by its
  // owner lane across the replays (every replay passes vertex 0 again and
  // captures the same triangle) -- a replay chunk does not start at vertex 0,
  // so the sweep cannot read it from the chunk's first task
  constexpr bool kTri0Carry = MATG && MODE == MODE_ADJU;
  static_assert(!kTri0Carry || kSub == 0, "the unbounded material adjoint has no sub-chunked sweep (IPT_ADJU_SUB)");
  int tri0_r = 0;
  // carried state in LDS (kCarryLds): word f of lane l at carry_ws[f * kBlock + l];
  // 0-2 Scar, 3-5 Mlo, 6 tri_0, 7-8 the work item.  Written by the owner lane,
  // read by its task lanes (same wave: LDS operations of a wave complete in
  // order).  The lane index is opaque at each use, so that the addresses are
  // formed there and not kept in registers through the trace loop.
  auto carry_at = [&](int f, int l) -> lds_u32 * {
    asm volatile("" : "+v"(l));
    return carry_ws + f * kBlock + l;
  };
  auto carry_put3 = [&](int f, V3 v) {
    lds_f32 *w = (lds_f32 *)carry_at(f, tid);
    w[0] = v.x;
    w[kBlock] = v.y;
    w[2 * kBlock] = v.z;
  };
  auto carry_get3 = [&](int f, int l) -> V3 {  // of lane l of this wave
    const lds_f32 *w = (const lds_f32 *)carry_at(f, (tid & ~63) + l);
    return mk(w[0], w[kBlock], w[2 * kBlock]);
  };
  // IPT_ADJU_SUB: the end of the sub-chunk this lane sweeps next (0: none);
  // such a lane is neither traced nor refilled until its chunk is swept
  int usub = 0;
  auto pending = [&]() { return MODE == MODE_ADJU && kSub > 0 && usub > 0; };
  // ADJU: the pool chunks this path holds and its ring size, in one word --
  // bits 6j..6j+5: the id of its chunk j (63: none), 24-29: the ring size
  // (a.rec_cap unless the pool ran dry) -- and the wave's free chunks
  constexpr uint32_t kNoChunks = 0x00ffffffu;
  uint32_t ctab = kNoChunks | ((uint32_t)vmax << 24);
  uint64_t pfree = MODE == MODE_ADJU ? (a.pool_chunks >= 64 ? ~0ull : (1ull << a.pool_chunks) - 1ull) : 0ull;
  auto vcap_of = [&]() { return (int)(ctab >> 24); };
  float weight = 1.f;  // GRAPH path weight
  V3 pix = p;          // GRAPH target pixel
  int k = 0, dst = 0;
  int ptri_r = -1;       // BVH: the triangle the path ray leaves (tree_skip), -1 = camera ray
  uint64_t witem_r = 0;  // this lane's work item (output slot / pixel source)
  auto set_item = [&](uint64_t w) {
    if (kLaneLds) {
      lane_ws[tid] = (uint32_t)w;
      lane_ws[kBlock + tid] = (uint32_t)(w >> 32);
    } else if (kCarryLds) {
      lds_u32 *q = carry_at(7, tid);
      q[0] = (uint32_t)w;
      q[kBlock] = (uint32_t)(w >> 32);
    } else {
      witem_r = w;
    }
  };
  auto witem = [&]() -> uint64_t {
    if (kLaneLds) return (uint64_t)lane_ws[tid] | ((uint64_t)lane_ws[kBlock + tid] << 32);
    if (kCarryLds) {
      const lds_u32 *q = carry_at(7, tid);
      return (uint64_t)q[0] | ((uint64_t)q[kBlock] << 32);
    }
    return witem_r;
  };
  auto set_ptri = [&](int t) {  // (read by the BVH instances' tree_skip only)
    if (!BVH) return;
    if (kLaneLds) lane_ws[2 * kBlock + tid] = (uint32_t)t;
    else ptri_r = t;
  };
  auto ptri = [&]() -> int { return kLaneLds ? (int)lane_ws[2 * kBlock + tid] : ptri_r; };
  // One iteration = one path vertex for the whole wave, in two
  // wave-synchronous phases: (1) every active lane casts its path ray and,
  // on a hit, shades the vertex and draws ALL of the vertex's random numbers
  // in the reference's order (NEE: emitter, r1, r2; then RR; then phi,
  // theta); (2) the lanes that need one cast their next-event shadow ray;
  // then every vertex lane finalises (L, M, records, next ray).  Each shading
  // block thus runs once per vertex with most lanes on, instead of path and
  // shadow lanes serialising each other's code every iteration.
#ifdef IPT_PHASE_TIMING
  uint64_t tacc[kPhaseWords] = {};
  uint64_t tp_ = __builtin_amdgcn_s_memtime();
#endif
  const int lane = tid & 63;
  // MODE_FWDM: this wave's slot table ([nslots] unfinished counts, [nslots]
  // pixels, padded to 16 B) and slots ([channel][sample] floats each)
  // kInph (the in-phase refill): between the two, the current
  // group's pixel entries (kEntryWords each, 16-B aligned, by place q in the group)
  constexpr bool kInph = kInphase<MODE, BVH>();
  // (VIEWS: the merged block rotates camera rays by record nT of geom, the
  // SCENE's camera -- the view instances keep the entries and refill at the
  // loop top from the view's own matrix; same frames, §17.2)
  constexpr bool kInphM = kInph && !VIEWS;
  // kInphP: the sample taken in phase waits above the old path's item in the
  // one item word; else in a register of its own.  The SPEC instances spill
  // 16 B per lane with the register, the diffuse ones are 0.5% slower packed.
  constexpr bool kInphP = kInphM && SPEC;
  auto fused_tab = [&](const TraceArgs &A) -> lds_u32 * {
    return (lds_u32 *)(reinterpret_cast<char *>(lds) + A.mean_off) + (size_t)(tid >> 6) * A.mean_wstride;
  };
  auto fused_entries = [&](const TraceArgs &A) -> lds_u32 * { return fused_tab(A) + ((2 * A.nslots + 3) & ~3); };
  auto fused_slots = [&](const TraceArgs &A) -> lds_f32 * {
    return (lds_f32 *)(fused_tab(A) + ((2 * A.nslots + 3) & ~3) + (kInph ? kEntryWords * A.group : 0u));
  };
  // the sample s of the group's pixel q: seed, column and row from the pixel's
  // entry -- item_ray_ls's values without its per-sample index arithmetic
  auto entry_sample = [&](const TraceArgs &A, uint32_t q, uint32_t s, float &cf, float &rf) -> uint64_t {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) v4u lds_v4u;
    const v4u e = *(const lds_v4u *)(fused_entries(A) + kEntryWords * q);
    cf = __uint_as_float(e.z);
    rf = __uint_as_float(e.w);
    return (((uint64_t)e.y << 32) | (uint64_t)e.x) + (uint64_t)s;
  };
  // Sum the slots of `mask` (wave-uniform, <= 16 of them): lanes 3i + c take
  // the i-th slot's channel c and add v_s / spp over s = 0 .. spp-1 in sample
  // order -- toneMap's operations (path_trace.cu:186-198), i.e.
  // pixel_mean_sm_kernel's -- then write the HDR (and 8-bit) pixel.
  auto fused_sum = [&](const TraceArgs &A, uint32_t mask) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the slots' sample writes before the sums
    __builtin_amdgcn_wave_barrier();
    const int m = __popc(mask);
    const int kq = (lane * 43) >> 7;  // lane / 3 for lane < 64
    int ch = lane - 3 * kq;
    // opaque per sum: left alone, the compiler forms the lane's output
    // pointer (out_samples + ch) once before the trace loop and holds the two
    // VGPRs through it for this one store per pixel
    asm volatile("" : "+v"(ch));
    int slot = 0;
    uint32_t mm = mask;
    for (int i = 0; i < m; ++i) {  // wave-uniform: this lane's slot = the kq-th set bit
      const int b = __builtin_ctz(mm);
      mm &= mm - 1u;
      slot = kq == i ? b : slot;
    }
    if (lane < 3 * m) {
      const int spp = A.spp;
      const lds_f32 *v = fused_slots(A) + (size_t)(3 * slot + ch) * spp;
      float acc = 0.f;
      if (A.rc_spp != 0.f && (spp & 3) == 0) {  // x * (1/spp) == x / spp (power of two); 16-B reads
        const float rc = A.rc_spp;
        for (int s = 0; s < spp; s += 4) {
          const v4f w4 = *(const lds_v4 *)(v + s);
          acc += w4.x * rc;
          acc += w4.y * rc;
          acc += w4.z * rc;
          acc += w4.w * rc;
        }
      } else {
        const float fs = (float)spp;
        for (int s = 0; s < spp; ++s) acc += v[s] / fs;
      }
      const uint64_t px = fused_tab(A)[A.nslots + slot];
      out_samples[px * 3 + ch] = acc;
      if (A.ldr) A.ldr[(size_t)set * A.out_stride + px * 3 + ch] = (uint8_t)(255.f * acc / (1 + acc));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the sums' reads before the slots are refilled
    __builtin_amdgcn_wave_barrier();
  };
  for (;;) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass has no AS4 copy)
    // The launch arguments, re-read from the kernarg segment every iteration
    // through a pointer the compiler cannot see through: left alone it keeps
    // the loop-invariant fields (camera, divisors, pointers) in SGPRs for
    // the whole loop, runs out of them and spills them to VGPR lanes, paying
    // a v_readlane (a VALU instruction) at every use.  Scalar loads hit the
    // constant cache.  This `a` shadows the parameter inside the loop.
    typedef __attribute__((address_space(4))) const TraceArgs cst_args;
    const cst_args *apc = (const cst_args *)__builtin_amdgcn_kernarg_segment_ptr();  // first parameter: offset 0
    asm volatile("" : "+s"(apc));
    TraceArgs a = *apc;
    if (VIEWS) {
      // The view's camera and origin (19 floats of the views' table, the
      // kernel's trailing parameter) in place of the scene's: wave-uniform,
      // read through the constant address space like the kernarg copy above
      // -- scalar loads from the scalar cache, taken again every iteration
      // instead of 19 SGPRs held through the loop.
      const cst_f32 *vq = (const cst_f32 *)karg<const float *>(sizeof(TraceKernArgs) + (MATG ? sizeof(void *) : 0)) +
                          (size_t)view * kViewFloats;
      asm volatile("" : "+s"(vq));
#pragma unroll
      for (int i = 0; i < 16; ++i) a.cam[i] = vq[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) a.cam_org[i] = vq[16 + i];
    }
#else
    TraceArgs a = ar;
#endif
    if (MODE == MODE_FWDM) {
      const uint32_t G = a.group;  // pixels per group (a chunk's last group may hold fewer)
      const bool issued = fj >= gnp * (uint32_t)a.spp;
      // sum the finished slots when a group's worth is waiting, when the next
      // group lacks free slots, or -- once the launch's work is handed out --
      // right away (lazily: one pass sums up to 16 pixels, 3 lanes each)
      if (sdone && ((uint32_t)__popc(sdone) >= G || exhausted || (issued && (uint32_t)__popc(sfree) < G))) {
        fused_sum(a, sdone);
        sfree |= sdone;
        sdone = 0;
      }
      // the next group of pixels (from the chunk in hand, else the wave's own
      // chunk, then the counter's) once the current one is fully issued and
      // G slots are free
      if (issued && !exhausted && (uint32_t)__popc(sfree) >= G) {
        if (pl0 >= pl1) {
          bool own = false;
          if (!started) {
            started = true;
            chunk_range<kGuided<BVH>()>(a, wave, a.npix, pl0, pl1);
            own = pl0 < a.npix;
          }
          if (!own) {
            uint32_t c = 0;
            if (lane == 0) c = atomicAdd(a.chunk_ctr + (size_t)set * kCtrStride, 1u);
            c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);  // lane 0 (full exec here)
            chunk_range<kGuided<BVH>()>(a, nwaves + c, a.npix, pl0, pl1);
            if (pl0 >= a.npix && lane == 0) grab_failed(a.chunk_ctr + (size_t)set * kCtrStride, c, a.grabs);
          }
        }
        if (pl0 < a.npix) {
          glp = (uint32_t)pl0;
          gnp = (uint32_t)(pl1 - pl0 < G ? pl1 - pl0 : G);
          pl0 += gnp;
          fj = 0;
          gslots = 0;
          uint32_t mm = sfree;
          for (uint32_t q = 0; q < gnp; ++q) {  // the lowest free slots, 4 bits per pixel
            gslots |= (uint32_t)__builtin_ctz(mm) << (4 * q);
            mm &= mm - 1u;
          }
          sfree = mm;
          if ((uint32_t)lane < gnp) {  // slot table: unfinished samples, pixel
            lds_u32 *tab = fused_tab(a);
            const uint32_t sl = (gslots >> (4 * lane)) & 15u;
            tab[sl] = (uint32_t)a.spp;
            tab[a.nslots + sl] = glp + (uint32_t)lane;
            if (kInph) {  // the pixel's entry, read by every sample of it that a lane takes
              uint32_t e[kEntryWords];
              pixel_entry(a, seed, glp + (uint32_t)lane, e);
              lds_u32 *w = fused_entries(a) + kEntryWords * lane;
#pragma unroll
              for (int i = 0; i < kEntryWords; ++i) w[i] = e[i];
            }
          }
          if (kInph) {  // the entries before the refills' reads (other lanes')
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
        } else {
          exhausted = true;
        }
      }
    } else if (next >= end && !exhausted) {  // wave-uniform: the next chunk (full exec here)
      // One counter, grabbed when needed.  Measured against alternatives
      // (profiles/r02_variants_chunk_*.log): 8 counters on separate lines
      // with stealing and a grab prefetched one chunk ahead were both slower
      // (and round 6's XCD bands).
      uint32_t c = 0;
      if (lane == 0) c = atomicAdd(a.chunk_ctr + (size_t)set * kCtrStride, 1u);
      c = (uint32_t)__shfl((int)c, 0);
      uint64_t start, stop;
      chunk_range<kGuided<BVH>()>(a, nwaves + c, a.n_samples, start, stop);
      if (start < a.n_samples) {
        next = start;
        end = stop;
      } else {
        exhausted = true;
        if (lane == 0) grab_failed(a.chunk_ctr + (size_t)set * kCtrStride, c, a.grabs);
      }
    }
    // ---- refill finished lanes from the wave's range (ballot + mbcnt)
    const bool wants = !active && !pending();
    const uint64_t need = __ballot(wants);
#ifdef IPT_PHASE_TIMING
    const uint64_t act0_ = ~need;
#endif
    if (MODE == MODE_FWDM) {
      const uint32_t fn = gnp * (uint32_t)a.spp;
      if (need && fj < fn) {
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
        if (!active && fj + rank < fn) {
          const uint32_t j = fj + rank;
          const uint32_t s = (gnp & (gnp - 1u)) == 0u ? j >> __builtin_ctz(gnp) : j / gnp;
          const uint32_t q = j - s * gnp;
          if (kInph) {
            float cf, rf;
            rng_init(st, entry_sample(a, q, s, cf, rf));
            camera_ray_f(a.cam, a.cam_org, st, rf, cf, a.W, a.H, a.rc_W, a.rc_H, p, d);
          } else {
            int r, c;
            item_ray_ls(a, seed, glp + q, s, st, p, d, r, c);
          }
          // the sample's LDS place: its pixel's slot, sample s
          if (kInph) set_item((uint64_t)(((gslots >> (4 * q)) & 15u) | (s << 4)));  // (one 32-bit value: s < 2^28)
          else set_item((uint64_t)((gslots >> (4 * q)) & 15u) | ((uint64_t)s << 4));
          L = mk(0.f, 0.f, 0.f);
          set_le(L);
          Ld = L;
          M = mk(1.f, 1.f, 1.f);
          k = 0;
          set_ptri(-1);
          active = true;
        }
        fj += (uint32_t)__popcll(need);
        fj = fj < fn ? fj : fn;
      }
    } else if (need) {
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      if (wants) {
        const uint64_t w = next + rank;
        if (w < end) {
          set_item(w);
          int r, c;
          item_ray(a, seed, w, st, p, d, r, c);
          L = mk(0.f, 0.f, 0.f);
          set_le(L);
          Ld = L;
          M = mk(1.f, 1.f, 1.f);
          k = 0;
          set_ptri(-1);
          if (MODE == MODE_ADJU) {
            rhi = 0;
            rslot = 0;
            if (!kSub) Mlo = mk(1.f, 1.f, 1.f);
            ctab = kNoChunks | ((uint32_t)vmax << 24);
          }
          if (MODE == MODE_GRAPH) {
            weight = 1.f;
            dst = nT;
            const uint8_t *px = target + ((size_t)r * a.W + c) * 3;
            pix = mk((float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f);
          }
          active = true;
        }
      }
      next += (uint64_t)__popcll(need);
    }
    PHASE(0)
    PHASE_LANES(10, active && !((act0_ >> (tid & 63)) & 1ull))
    // (MODE_FWDM: the last finished slots are summed at the loop top first)
    if (__ballot(active || pending()) == 0 &&
        (MODE != MODE_FWDM || (exhausted && sdone == 0 && fj >= gnp * (uint32_t)a.spp)))
      break;
#ifdef IPT_PHASE_TIMING
    tacc[6] += 1;
    tacc[7] += __popcll(__ballot(active));
#endif

    // ================= phase 1: path ray (radiance, path_trace.cu:111-144)
    float t = 0.f;
    int hit = -1;
    if (BVH) {  // pre-pass per lane, the tree part by 8-lane groups
      bool qn = false;
      if (active) {
        bvh_prepass<false>(bv, p, d, t, hit, -1);
        qn = coop_root_test(cv, p, d, t) && !tree_skip(a.src_cull, ptri(), d);
      }
      SUBPHASE_BEGIN
      coop_cast<false>(cv, qn, p, d, t, hit);
      SUBPHASE_END(8)
    } else if (active) {
      if (e3)
        hit = closest_hit_pairs_culled((const lds_f32 *)lds_pr, a.pboxes, nT, p, d, t);
      else
        hit = cast_bf(pairs, e3, nT, p, d, t);
    }
    PHASE(1)
    const bool vertex = active && hit >= 0;
    bool finished = false, escaped = false;
    if (active && hit < 0) {  // miss: the stale L_e/L_d are re-added (F4)
      finished = true;
      escaped = (k > 0);
      if (MODE != MODE_GRAPH) {
        const V3 Le = le();
        L = mk(fmaf(M.x, Le.x + Ld.x, L.x), fmaf(M.y, Le.y + Ld.y, L.y), fmaf(M.z, Le.z + Ld.z, L.z));
      }
    }
    const int tri = hit;
    V3 nh = p, din = d, sd = d, nd = d;
    bool shadow = false, cont = false;
    // kInphM: the vertex passed Russian roulette; this lane's path ends here
    // and it has taken its next sample, the item nitem (slot | s << 4)
    bool wantc = false, refill = false;
    uint32_t nitem = 0;
    int emitter = 0, et_sh = 0;
    float ct = 0.f, coeff = 0.f, speci = 0.f, specd = 0.f;
    if (vertex) {
      const V3 q = along(p, d, t);
      if (MODE == MODE_GRAPH) {
        (void)uniform(st);  // isSpecular = u < P_SPEC(0), inv_path_trace.cu:117
        const float wf = weight * 1.f;  // Edge::update, inv_scene.h:26-36
        const double v[5] = {(double)weight, (double)wf, (double)(wf * pix.x), (double)(wf * pix.y),
                             (double)(wf * pix.z)};
        const size_t bin = (size_t)dst * nT + tri;
        bins_add(a.lds_edges != 0, edges, a.lds_edges ? bin * kEdgeL : bin * kEdgeW, 5, v);
      } else if (k == 0) {
        set_le(ke3(tri));
        if (kTri0Carry) {
          if (kCarryLds) *carry_at(6, tid) = (uint32_t)tri;
          else tri0_r = tri;
        }
      }
      if (SHADE) {  // the flat normal from the triangle's record; a wave without other triangles pays nothing more
        const lds_f32 *r = tsh + tri * kTriShadeStride;
        const bool flat = (__float_as_uint(r[TS_FLAGS]) & GEOM_AXIS_FLAT) != 0u;
        nh = mk(r[TS_VN], r[TS_VN + 1], r[TS_VN + 2]);
        if (__ballot(!flat)) {
          if (!flat) nh = shading_normal(geom[tri], q);
        }
      } else {
        nh = shading_normal(geom[tri], q);
      }
      p = q;
      Ld = mk(0.f, 0.f, 0.f);
      if (nE > 0) {  // directLighting up to the shadow ray, path_trace.cu:30-71
        const float u = uniform(st);
        int ie = 0;
        if (SHADE) {
          // the CDF is the same for every lane: a wave-uniform walk over its LDS
          // copy, 16 B per read (broadcast), the first i with cdf[i] >= u kept
          // per lane -- the loop below without its per-lane loads (the NaN
          // padding behind entry nE-1 is never >= u; no monotone CDF assumed)
          ie = nE - 1;
          bool found = false;
          for (int i = 0; i < nE; i += 4) {
            const v4f c = *(const lds_v4 *)(cdf_l + i);
            const bool h0 = !found && c.x >= u;
            ie = h0 ? i : ie;
            found = found || h0;
            const bool h1 = !found && c.y >= u;
            ie = h1 ? i + 1 : ie;
            found = found || h1;
            const bool h2 = !found && c.z >= u;
            ie = h2 ? i + 2 : ie;
            found = found || h2;
            const bool h3 = !found && c.w >= u;
            ie = h3 ? i + 3 : ie;
            found = found || h3;
          }
        } else {
          while (ie < nE && !(emit_cdf[ie] >= u)) ++ie;
          ie = ie < nE ? ie : nE - 1;
        }
        const float r1 = uniform(st), r2 = uniform(st);
        const double sq = dsqrt_core((double)r1);  // r1 >= 2^-33: sqrt's identity range
        const float ca = (float)(1.0 - sq);
        const float cb = (float)(sq * (double)(1.f - r2));
        const float cc = (float)((double)r2 * sq);
        V3 pt;
        if (SHADE) {  // the emitter's vertices (and its triangle) from its record
          const lds_f32 *er = esh + ie * kEmitShadeStride;
          if (kEtEarly) et_sh = (int)__float_as_uint(er[ES_TRI]);
          const lds_f32 *ev = er + ES_V;
          pt = mk(fmaf(cc, ev[6], fmaf(cb, ev[3], ca * ev[0])), fmaf(cc, ev[7], fmaf(cb, ev[4], ca * ev[1])),
                  fmaf(cc, ev[8], fmaf(cb, ev[5], ca * ev[2])));
        } else {
          const TriGeom &ge = geom[emit_tri[ie]];
          pt = mk(fmaf(cc, ge.v[2][0], fmaf(cb, ge.v[1][0], ca * ge.v[0][0])),
                  fmaf(cc, ge.v[2][1], fmaf(cb, ge.v[1][1], ca * ge.v[0][1])),
                  fmaf(cc, ge.v[2][2], fmaf(cb, ge.v[1][2], ca * ge.v[0][2])));
        }
        sd = unit(sub(pt, q));
        ct = dot3(nh, sd);
        emitter = ie;
        shadow = !(ct < 0.f);
      }
      if (!(a.max_bounces >= 0 && k == a.max_bounces)) {
        const float pr = uniform(st);  // Russian roulette, path_trace.cu:130-131
        if (kInphM) {                   // (the direction: below, merged with the refilling lanes' camera rays)
          wantc = pr < kPRR;
        } else if (pr < kPRR) {         // sampleNextDir, path_trace.cu:91-109
          const TriMat &m = mat[tri];
          // (SHADE: TriMat::flags from the record's flags word)
          const uint32_t sflags = SPEC && SHADE ? __float_as_uint(tsh[tri * kTriShadeStride + TS_FLAGS]) >> 8 : 0u;
          const bool spec = SPEC && (MODE != MODE_GRAPH) && ((SHADE ? sflags : m.flags) & MAT_SPECULAR);
          const float uphi = uniform(st);
          const float phi = (float)(2.0 * kPi * (double)uphi);
          const float ut = uniform(st);
          float cth, sth, psamp;
          if (!spec) {
            cth = sqrt_core(ut);  // == (float)sqrt((double)ut) (innocuous double rounding); ut >= 2^-33
            // sin(theta) = sqrt(1 - u) from the float 1 - u (rounds 1-6: from the
            // exact double 1 - u, 0.6% slower)
            const float omu = 1.0f - ut;  // 0 or >= 2^-24
            sth = omu > 0.f ? sqrt_core(omu) : 0.f;
            psamp = kInvPiF;
          } else {
            const double cd = pow_d((double)ut, 1.0 / ((double)m.shininess + 1.0));
            cth = (float)cd;
            sth = (float)sqrt(1.0 - cd * cd);
            psamp = pow_f((m.shininess + 1.f) * cth, m.shininess);
          }
          float sp, cp;
          sincos_f(phi, sp, cp);
          const V3 h = mk(sth * cp, sth * sp, cth);
          if (SHADE) {
            const lds_f32 *R = tsh + tri * kTriShadeStride + TS_R;
            nd = unit(mk(fmaf(R[2], h.z, fmaf(R[1], h.y, R[0] * h.x)), fmaf(R[5], h.z, fmaf(R[4], h.y, R[3] * h.x)),
                         fmaf(R[8], h.z, fmaf(R[7], h.y, R[6] * h.x))));
          } else {
            const TriGeom &g = geom[tri];
            nd = unit(mk(fmaf(g.R[0][2], h.z, fmaf(g.R[0][1], h.y, g.R[0][0] * h.x)),
                         fmaf(g.R[1][2], h.z, fmaf(g.R[1][1], h.y, g.R[1][0] * h.x)),
                         fmaf(g.R[2][2], h.z, fmaf(g.R[2][1], h.y, g.R[2][0] * h.x))));
          }
          if (MODE != MODE_GRAPH) {
            if (SPEC && ((SHADE ? sflags : m.flags) & MAT_HAS_KS)) speci = phong(m.shininess, nh, din, nd);
            coeff = spec ? (dot3(nd, nh) / psamp) / kPRR : div_const<1>(div_const<0>(dot3(nd, nh)));  // psamp = kInvPiF
          }
          cont = true;
        }
      }
    }
    if (kInphM) {
      // In-phase refill.  A lane whose path ends in this
      // iteration -- it missed, or its vertex does not continue -- takes the
      // group's next sample here, handed out as at the loop top, and builds
      // its camera ray in the block that samples the continuing lanes' next
      // direction: two draws from the lane's state, a local vector under each
      // group's own mask, then one rotation (the camera's is record nT of
      // geom) and one unit() for both.  The old path's RNG state is dead by
      // now: every draw of a vertex precedes this point.  L, Le, Ld, M, k and
      // the work item still serve the old path to the end of the iteration;
      // the lane is reset after its output write.
      const bool ends = active && !wantc;
      const uint64_t ask = __ballot(ends);
      const uint32_t fn = gnp * (uint32_t)a.spp;
      float ecf = 0.f, erf = 0.f;
      if (ask && fj < fn) {  // wave-uniform
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(ask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ask, 0u));
        if (ends && fj + rank < fn) {
          const uint32_t j = fj + rank;
          const uint32_t s = (gnp & (gnp - 1u)) == 0u ? j >> __builtin_ctz(gnp) : j / gnp;
          const uint32_t q = j - s * gnp;
          rng_init(st, entry_sample(a, q, s, ecf, erf));
          nitem = ((gslots >> (4 * q)) & 15u) | (s << 4);
          // kInphP: it waits (12 bits: slot, s < 256) above the old path's item, under a marker bit
          if (kInphP) set_item(witem() | (uint64_t)((nitem | 0x1000u) << 16));
          refill = true;
        }
        fj += (uint32_t)__popcll(ask);
        fj = fj < fn ? fj : fn;
      }
      if (wantc || refill) {
        const float ua = uniform(st);  // cont: phi's draw; refill: the camera's u0
        const float ub = uniform(st);  // cont: theta's;    refill: u1
        const TriMat &m = mat[refill ? 0 : tri];
        // (SHADE: TriMat::flags from the record's flags word)
        const uint32_t sflags = SPEC && SHADE ? __float_as_uint(tsh[(refill ? 0 : tri) * kTriShadeStride + TS_FLAGS]) >> 8 : 0u;
        const bool spec = SPEC && !refill && ((SHADE ? sflags : m.flags) & MAT_SPECULAR);
        float psamp = kInvPiF;
        V3 h;
        if (refill) {
          h = camera_local(ua, ub, ecf, erf, a.W, a.H, a.rc_W, a.rc_H);
        } else {  // sampleNextDir, path_trace.cu:91-109
          const float phi = (float)(2.0 * kPi * (double)ua);
          float cth, sth;
          if (!spec) {
            cth = sqrt_core(ub);  // == (float)sqrt((double)ut) (innocuous double rounding); ut >= 2^-33
            const float omu = 1.0f - ub;  // 0 or >= 2^-24
            sth = omu > 0.f ? sqrt_core(omu) : 0.f;
          } else {
            const double cd = pow_d((double)ub, 1.0 / ((double)m.shininess + 1.0));
            cth = (float)cd;
            sth = (float)sqrt(1.0 - cd * cd);
            psamp = pow_f((m.shininess + 1.f) * cth, m.shininess);
          }
          float sp, cp;
          sincos_f(phi, sp, cp);
          h = mk(sth * cp, sth * sp, cth);
        }
        V3 v;
        if (SHADE) {  // (the camera's rotation is record nT of the table, as of geom)
          const lds_f32 *R = tsh + (refill ? nT : tri) * kTriShadeStride + TS_R;
          v = mk(fmaf(R[2], h.z, fmaf(R[1], h.y, R[0] * h.x)), fmaf(R[5], h.z, fmaf(R[4], h.y, R[3] * h.x)),
                 fmaf(R[8], h.z, fmaf(R[7], h.y, R[6] * h.x)));  // rotate3's chain
        } else {
          const TriGeom &g = geom[refill ? nT : tri];
          v = rotate3(g.R[0], g.R[1], g.R[2], h);
        }
        if (refill) v = camera_w0(a.cam, v);  // Ray::transform's w term: these lanes only
        nd = unit(v);
        if (wantc) {
          if (SPEC && ((SHADE ? sflags : m.flags) & MAT_HAS_KS)) speci = phong(m.shininess, nh, din, nd);
          coeff = spec ? (dot3(nd, nh) / psamp) / kPRR : div_const<1>(div_const<0>(dot3(nd, nh)));  // psamp = kInvPiF
          cont = true;
        }
      }
    }

    // ================= phase 2: next-event shadow ray (path_trace.cu:73-88)
    PHASE(2)
    PHASE_LANES(12, vertex)
    V3 lo = mk(0.f, 0.f, 0.f);
    float emit_s = 0.f;  // ADJ record: lo = Ke[emit_et] * emit_s
    int emit_et = 0;
    float ts = 0.f;
    int hs = -1;
    const int et = !shadow ? -1
                   : !SHADE   ? emit_tri[emitter]
                   : kEtEarly ? et_sh
                              : (int)__float_as_uint(esh[emitter * kEmitShadeStride + ES_TRI]);
    if (__ballot(shadow)) {
      PHASE_LANES(14, shadow)
      if (BVH) {
        bool qn = false;
        if (shadow && bvh_prepass<true>(bv, p, sd, ts, hs, et,
                                        a.big_pomask ? a.big_pomask[tri * nE + emitter] : 0xffffffffu, emitter))
          qn = coop_root_test(cv, p, sd, ts) && !tree_skip(a.src_cull, tri, sd);
        SUBPHASE_BEGIN
        coop_cast<true>(cv, qn, p, sd, ts, hs);
        SUBPHASE_END(9)
      } else if (shadow) {
        if (e3)
          hs = shadow_hit_pairs_small((const lds_f32 *)lds_pr, pairs, a.pboxes, e3, nT, p, sd, et, ts,
                                      [&]() { return po ? ((const lds_u32c *)lds_po)[tri * nE + emitter] : 0xffffffffu; });
        else
          hs = cast_bf(pairs, e3, nT, p, sd, ts);
      }
      PHASE(3)
      if (shadow && hs == et) {  // must hit the sampled emitter itself
        // SHADE: the emitter's record -- normal and flags, then, on the lanes that
        // face it, Ke, pmf and its reciprocal (asked for with the normal they
        // cost the fused forward three registers it does not have)
        V3 ne;
        if (SHADE) {
          const lds_f32 *er = esh + emitter * kEmitShadeStride;
          const bool flat = (__float_as_uint(er[ES_FLAGS]) & GEOM_AXIS_FLAT) != 0u;
          ne = mk(er[ES_VN], er[ES_VN + 1], er[ES_VN + 2]);
          if (__ballot(!flat)) {
            if (!flat) ne = shading_normal(geom[et], along(p, sd, ts));
          }
        } else {
          ne = shading_normal(geom[et], along(p, sd, ts));
        }
        const float ctp = -dot3(ne, sd);
        if (!(ctp < 0.f)) {
          const double td = (double)ts;
          V3 kee_s = mk(0.f, 0.f, 0.f);
          double pr_s = 0.0;
          float pmf_s = 0.f;
          if (SHADE) {
            const lds_f32 *er = esh + emitter * kEmitShadeStride;
            kee_s = mk(er[ES_KE], er[ES_KE + 1], er[ES_KE + 2]);
            pmf_s = er[ES_PMF];
            pr_s = __hiloint2double((int)__float_as_uint(er[ES_PMFR + 1]), (int)__float_as_uint(er[ES_PMFR]));
          }
          if (MODE == MODE_GRAPH) {
            const TriMat &me = mat[et];
            const double q = (double)((weight * ct) * ctp) / (td * td), pr = SHADE ? pr_s : a.emit_pmfr[emitter];
            double w2d;
            if (pr != 0.0)
              w2d = q * pr;
            else
              w2d = q / (double)(SHADE ? pmf_s : emit_pmf[emitter]);
            const float w2 = (float)w2d;
            const float wf = w2 * kInvPiF;  // BSDF(direct) factor 1/pi, inv_path_trace.cu:8
            const double v[8] = {(double)w2, (double)wf, (double)(wf * pix.x), (double)(wf * pix.y),
                                 (double)(wf * pix.z), (double)(wf * me.ke[0]), (double)(wf * me.ke[1]),
                                 (double)(wf * me.ke[2])};
            const size_t bin = (size_t)tri * nT + et;
            if (a.lds_edges) {
              bins_add(true, edges, bin * kEdgeL, 5, v);
              bins_add(true, edges, (size_t)(nT + 1) * nT * kEdgeL + ((size_t)tri * nE + emitter) * 3, 3, v + 5);
            } else {
              bins_add(false, edges, bin * kEdgeW, 8, v);
            }
          } else {
            const double q = (double)(ct * ctp) / (td * td), pr = SHADE ? pr_s : a.emit_pmfr[emitter];
            double s64;
            if (pr != 0.0)
              s64 = q * pr;
            else
              s64 = q / (double)(SHADE ? pmf_s : emit_pmf[emitter]);
            const float s = (float)s64;
            const V3 kee = SHADE ? kee_s : ke3(et);
            lo = mk(kee.x * s, kee.y * s, kee.z * s);
            emit_s = s;
            emit_et = et;
            const TriMat &m = mat[tri];
            if (SPEC && (m.flags & MAT_HAS_KS)) specd = phong(m.shininess, nh, din, sd);
            const V3 kt = kd3(tri);
            if (SPEC)
              Ld = mk((kt.x + m.ks[0] * specd) * lo.x, (kt.y + m.ks[1] * specd) * lo.y,
                      (kt.z + m.ks[2] * specd) * lo.z);
            else  // Ks = 0: kd + 0*0 == kd
              Ld = mk(kt.x * lo.x, kt.y * lo.y, kt.z * lo.z);
          }
        }
      }
    }

    PHASE(4)
    PHASE_LANES(16, shadow && hs == et)
    if (MODE == MODE_ADJU) {
      // a lane about to write the first slot of a pool chunk it does not hold
      // takes one (wave-uniform hand-out in lane order); none left: the ring
      // ends here for this path (rslot = k, no wrap yet, so the path's chunks
      // [j vcap, (j+1) vcap) stay aligned) and this record goes to slot 0
      const int gs = rslot - a.rec_lds;
      const int sh = 6 * (gs / kPoolSlots);
      const bool needc = vertex && gs >= 0 && (gs % kPoolSlots) == 0 && ((ctab >> sh) & 63u) == 63u;
      uint64_t want = __ballot(needc);
      if (want) {
        int got = -1;
        do {
          const int l = (int)__builtin_ctzll(want);
          want &= want - 1;
          const int c = pfree ? (int)__builtin_ctzll(pfree) : -1;
          pfree &= pfree - 1ull;
          if (lane == l) got = c;
        } while (want);
        if (needc) {
          if (got >= 0) {
            ctab = (ctab & ~(63u << sh)) | ((uint32_t)got << sh);
          } else {
            ctab = (ctab & 0x00ffffffu) | ((uint32_t)rslot << 24);
            rslot = 0;
          }
        }
      }
    }
    // ================= finalise the vertex
    PHASE_LANES(18, vertex)
    if (vertex) {
      if (is_badj<MODE>()) {  // vertex record k (layout [field][vertex][lane])
        float *rec = lds_rec + (size_t)k * kBlock + tid;
        const size_t fs = (size_t)vmax * kBlock;
        rec[0] = __uint_as_float((uint32_t)tri | ((uint32_t)emit_et << 16));
        rec[fs] = emit_s;
        rec[2 * fs] = coeff;
        if (SPEC) {
          rec[kRecSD * fs] = specd;
          rec[(kRecSD + 1) * fs] = speci;
        }
      }
      if (MODE == MODE_ADJU) {  // ring slot rslot = k % rec_cap: LDS or global (TraceArgs::rec_lds)
        constexpr int NF = SPEC ? kRecFieldsSpec : kRecFieldsDiffuse;
        float v[NF];
        v[0] = __uint_as_float((uint32_t)tri | ((uint32_t)emit_et << 16));
        v[1] = emit_s;
        v[2] = coeff;
        if (SPEC) {
          v[kRecSD] = specd;
          v[kRecSD + 1] = speci;
        }
        const int nl = a.rec_lds;
        if (rslot < nl) {  // LDS slot
          float *rec = lds_rec + (size_t)rslot * kBlock + tid;
          const size_t fs = (size_t)nl * kBlock;
#pragma unroll
          for (int f = 0; f < NF; ++f) rec[f * fs] = v[f];
        } else {  // global slot: pool chunk (rslot - nl) / kPoolSlots of this lane
          const int gs = rslot - nl;
          const uint32_t c = (ctab >> (6 * (gs / kPoolSlots))) & 63u;
          gbl_f32 *rec = upool + ((size_t)c * kPoolSlots + (size_t)(gs % kPoolSlots)) * NF;
#pragma unroll
          for (int f = 0; f < NF; ++f) rec[f] = v[f];
        }
        // a chunk starts at ring slot 0 (vertex j * ring size): the forward's M
        // before the update of its first vertex is the chunk's Mlo
        if (kSub > 0) {  // (vertex 0's M is 1: not stored)
          if (rslot % kSub == 0 && k > 0) {
            gbl_f32 *m = umr + (size_t)(rslot / kSub) * 192;
            m[0] = M.x;
            m[1] = M.y;
            m[2] = M.z;
          }
        } else if (rslot == 0) {
          // (kCarryLds: vertex 0 is at slot 0 and stores M = 1, so the resets of Mlo are not mirrored)
          if (kCarryLds) carry_put3(3, M);
          else Mlo = M;
        }
        rslot = (rslot + 1 == vcap_of()) ? 0 : rslot + 1;
      }
      if (MODE == MODE_GRAPH) {
        if (cont) {
          weight *= dot3(nd, nh);  // inv_path_trace.cu:144-145
          weight = (float)((double)weight * (((1.0 / (double)kInvPiF) / (double)kPRR) / 1.0));
          dst = tri;
        }
      } else {
        const V3 Le = le();
        L = mk(fmaf(M.x, Le.x + Ld.x, L.x), fmaf(M.y, Le.y + Ld.y, L.y), fmaf(M.z, Le.z + Ld.z, L.z));
        if (cont) {
          const V3 tp = kdpi3(tri);
          const float t0 = tp.x, t1 = tp.y, t2 = tp.z;
          if (SPEC) {
            const TriMat &m = mat[tri];
            M = mk((M.x * (t0 + m.ks[0] * speci)) * coeff, (M.y * (t1 + m.ks[1] * speci)) * coeff,
                   (M.z * (t2 + m.ks[2] * speci)) * coeff);
          } else {  // Ks = 0: kd/pi + 0*0 == kd/pi
            M = mk((M.x * t0) * coeff, (M.y * t1) * coeff, (M.z * t2) * coeff);
          }
        }
      }
      ++k;  // vertices so far
      if (BVH) set_ptri(tri);
      if (cont) d = nd;
      else finished = true;
      if (MODE == MODE_ADJU && rhi > 0 && k == rhi) finished = true;  // replay reached its target
    }

    // ADJU: the chunk [ulo, uhi) to sweep; uend = it ends the path (its escape
    // terms apply, uesc = the path escaped); urep = replay target (0: none)
    int uhi = 0, ulo = 0, urep = 0;
    bool uend = false, uesc = false;
    const bool upend = pending();  // a lane with sub-chunks of its chunk left (IPT_ADJU_SUB)
    if (upend) {  // the chunk of its last sweep: k, rslot, rhi and ctab are untouched since
      uhi = usub;
      ulo = rhi == 0 ? k - (rslot == 0 ? vcap_of() : rslot) : rhi - vcap_of();
      if (ulo > 0) urep = ulo;
    }
    if (finished) {
      active = false;
      if (MODE == MODE_FWDM) {  // slot [channel][sample]
        const uint64_t wi = witem();
        // (kInphP: the item is slot | s << 4 in 12 bits, the waiting one above it)
        lds_f32 *o = fused_slots(a) + (uint32_t)(wi & 15u) * 3u * (uint32_t)a.spp +
                     (kInphP ? ((uint32_t)wi >> 4) & 0xffu : (uint32_t)(wi >> 4));
        o[0] = L.x;
        o[a.spp] = L.y;
        o[2 * a.spp] = L.z;
      } else if (MODE == MODE_FWD) {
        float *o = out_samples + witem() * 3;
        o[0] = L.x;
        o[1] = L.y;
        o[2] = L.z;
      } else if (MODE == MODE_ADJU) {
        // The first pass sweeps the path's last chunk [b, K), b = the last
        // multiple of rec_cap below K (its records are the ring's slots 0 ..
        // K - b - 1, its Mlo was captured at vertex b).  A replay to vertex b
        // (same seed, same draws, same floats) re-records [b - rec_cap, b) in
        // slots 0 .. rec_cap - 1 and captures that chunk's Mlo; it is swept with
        // the suffix carried from the chunk after (Scar), and so on to vertex 0.
        if (rhi == 0) {
          uhi = k;
          ulo = k > 0 ? k - (rslot == 0 ? vcap_of() : rslot) : 0;  // (rslot = K % ring size)
          uend = true;
          uesc = escaped;
        } else {
          uhi = rhi;
          ulo = rhi - vcap_of();
        }
        if (ulo > 0) urep = ulo;
      }
    }
    // IPT_ADJU_SUB: this iteration sweeps the chunk's last unswept sub-chunk
    // [uslo, uhi) (sub-chunks aligned to the chunk's start)
    const int uslo = (MODE == MODE_ADJU && kSub > 0 && uhi > ulo) ? ulo + kSub * ((uhi - 1 - ulo) / kSub) : ulo;
    if (MODE == MODE_FWDM && __ballot(finished)) {
      // fused pixel mean: each finished lane counts its sample off its slot's
      // table entry (LDS atomic, after the wave's sample writes: a wave's LDS
      // operations complete in order); the lane that takes a count to zero
      // marks the slot done.  Slots are summed lazily at the loop top.
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      uint32_t left = 0;
      if (finished)
        left = __hip_atomic_fetch_sub(fused_tab(a) + (uint32_t)(witem() & 15u), 1u, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_WORKGROUP);
      uint64_t comp = __ballot(finished && left == 1u);
      while (comp) {  // wave-uniform: usually 0 or 1 slot per iteration
        const int l = (int)__builtin_ctzll(comp);
        comp &= comp - 1ull;
        sdone |= 1u << (__builtin_amdgcn_readlane((int)(witem() & 15u), l) & 31);
      }
    }
    // the old path is written and counted: a lane that took a sample in phase starts it
    if (kInphM && (kInphP ? ((uint32_t)witem() >> 16) != 0u : refill)) {
      L = mk(0.f, 0.f, 0.f);
      set_le(L);
      Ld = L;
      M = mk(1.f, 1.f, 1.f);
      k = 0;
      p = mk(a.cam_org[0], a.cam_org[1], a.cam_org[2]);
      d = nd;
      set_item(kInphP ? (uint64_t)(((uint32_t)witem() >> 16) & 0xfffu) : (uint64_t)nitem);
      active = true;
    }
    if (is_adj<MODE>()) {
      // Wave-parallel backward sweep (oracle adjoint_sample).  The vertices of
      // the paths that finished in this iteration become tasks (path, vertex
      // kk), packed into rounds of <= 64 consecutive lanes without splitting a
      // path (K <= rec_cap <= 63).  Each task lane reads ITS vertex's record
      // once; the prefix throughputs M_kk then pass left to right and the
      // suffixes S_kk+1 right to left between neighbouring lanes (wave shifts),
      // every step with the forward's / the per-path sweep's own operations,
      // so each M_kk and S_kk+1 is the same float as in the oracle's single
      // sweep (only the order of the fp64 gradient atomics changes).  Round 2
      // recomputed both chains per task from the owner's LDS column (O(K^2)
      // record reads, loops as long as the wave's longest chain).
      // MODE_ADJU sweeps the chunk [ulo, uhi) of each finished lane the same
      // way, from its ring slots (LDS, then global): the prefix chain starts
      // from the chunk's captured Mlo, the last task's suffix is the chunk
      // after's (Scar) unless the chunk ends the path, and the suffix at ulo
      // goes back to the owner for its replay.
      const int Kf = is_badj<MODE>() ? ((finished && k > 0) ? k : 0) : (uhi > 0 ? uhi - uslo : 0);
      if (__ballot(Kf > 0)) {
        const int lane = tid & 63;
        const int inc = wave_scan_add(Kf);  // inclusive scan of the task counts over the wave
        const int T = __builtin_amdgcn_readlane(inc, 63);
        // per-wave LDS word per lane: the round's owner markers
        uint32_t *swl = reinterpret_cast<uint32_t *>(lds_rec) - kBlock + (tid & ~63);
        float wx = 0.f, wy = 0.f, wz = 0.f;  // the owner's adjoint weights dL/dI / spp
        uint32_t tlp_lo = 0u, tlp_hi = 0u;   // TANG: the owner's launch-local pixel
        if (TANG) {  // no adjoint image: dL/dI = 1 at the owner's own pixel
          if (Kf > 0) {
            wx = wy = wz = a.rc_spp != 0.f ? a.rc_spp : 1.0f / (float)a.spp;
            uint64_t lp, sj;
            item_split(a, witem(), lp, sj);
            tlp_lo = (uint32_t)lp;
            tlp_hi = (uint32_t)(lp >> 32);
          }
        } else if (Kf > 0) {
          const float *adj = karg<const float *>(offsetof(TraceKernArgs, adj)) +
                             (a.nscenes > 1 ? (size_t)set * a.adj_stride : 0);
          const uint64_t pixel = item_pixel(a, witem());
          if (a.rc_spp != 0.f) {
            wx = adj[pixel * 3 + 0] * a.rc_spp;
            wy = adj[pixel * 3 + 1] * a.rc_spp;
            wz = adj[pixel * 3 + 2] * a.rc_spp;
          } else {
            wx = adj[pixel * 3 + 0] / (float)a.spp;
            wy = adj[pixel * 3 + 1] / (float)a.spp;
            wz = adj[pixel * 3 + 2] / (float)a.spp;
          }
        }
        const size_t fs = (size_t)vmax * kBlock;  // ADJ record field stride (ADJU: per slot kind, below)
        int base = 0;
        while (base < T) {  // wave-uniform
          // this round: the whole paths whose tasks end by base + 64
          const uint64_t fit = __ballot(Kf > 0 && inc <= base + 64);
          const int next = __builtin_amdgcn_readlane(inc, 63 - (int)__builtin_clzll(fit));
          const int t = base + lane;
          const bool valid = t < next;
          PHASE_LANES(20, valid)
          // owners of this round mark their first task's lane with (start,
          // first pass, escaped, K, owner lane) + 1 -- start in the top bits,
          // so an inclusive max-scan leaves every task lane the marker of the
          // last owner starting at or before it: its own path
          swl[lane] = 0u;
          const int st0 = inc - Kf - base;
          const bool owns = Kf > 0 && inc <= next && st0 >= 0;
          const bool oend = is_badj<MODE>() || uend, oesc = is_badj<MODE>() ? escaped : uesc;
          // (ADJU: the sub-chunk's first ring slot, uslo - ulo, in bits 15-20)
          if (owns)
            swl[st0] = (((uint32_t)st0 << 21) | ((uint32_t)(MODE == MODE_ADJU ? uslo - ulo : 0) << 15) |
                        (oend ? 1u << 14 : 0u) | (oesc ? 1u << 13 : 0u) | ((uint32_t)Kf << 6) | (uint32_t)lane) + 1u;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const uint32_t mk_ = wave_scan_max(swl[lane]) - 1u;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // read before the next round's marks
          __builtin_amdgcn_wave_barrier();
          const int ow = valid ? (int)(mk_ & 63u) : lane;
          const int KL = valid ? (int)((mk_ >> 6) & 127u) : 0;
          const int kk = valid ? lane - (int)(mk_ >> 21) : 0;  // task index inside the path's (sub-)chunk
          const bool esc = valid && ((mk_ >> 13) & 1u);
          const bool fst_o = is_badj<MODE>() || (valid && ((mk_ >> 14) & 1u));  // the chunk ends the path
          const int rr = valid ? KL - 1 - kk : 0;  // vertices after this one
          const V3 Lev = le();
          V3 LeL = mk(__shfl(Lev.x, ow), __shfl(Lev.y, ow), __shfl(Lev.z, ow));
          // the unbounded material adjoint: the owner's first triangle instead, and Le = Ke[tri_0]
          // re-read through it (the same floats; the owner's three Le registers die in the trace loop)
          if (kCarryLds) {  // the owners' carried words, written in this or an earlier iteration
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
          }
          // (taken only by the round's task lanes, whose owner has passed its vertex 0; a lane outside the
          // round may never have written its word -- carry_ws is not initialised -- and the load below is
          // unconditional; clamped as unsigned, like tk below, so nothing reaches global memory out of bounds)
          int tri0c = 0;
          if (kCarryLds) {
            if (valid) tri0c = (int)min(*carry_at(6, (tid & ~63) + ow), (uint32_t)(nT - 1));
          } else if (kTri0Carry) {
            tri0c = (int)min((uint32_t)__shfl(tri0_r, ow), (uint32_t)(nT - 1));
          }
          if (kTri0Carry) LeL = ke3(tri0c);
          // this task's record (lanes past the round read vertex 0 of a valid column)
          uint32_t f0;
          float es, ck, sdv = 0.f, si = 0.f;
          // the prefix throughput: the chunk's Mlo on its first task, passed
          // right by the chain below (ADJ: every chunk starts at vertex 0)
          V3 Mk = mk(1.f, 1.f, 1.f);
          V3 Sc = mk(0.f, 0.f, 0.f);  // ADJU: the owner's suffix from the chunk after
          if (is_badj<MODE>()) {
            const float *r = lds_rec + (tid & ~63) + (valid ? ow : lane) + (size_t)kk * kBlock;
            f0 = valid ? __float_as_uint(r[0]) : 0u;
            es = r[fs];
            ck = r[2 * fs];
            if (SPEC) {
              sdv = r[kRecSD * fs];
              si = r[(kRecSD + 1) * fs];
            }
          } else {
            // the vertex's ring slot (chunks start at slot 0; a sub-chunk at uslo - ulo)
            const int sl = kk + (valid ? (int)((mk_ >> 15) & 63u) : 0), nl = a.rec_lds;
            constexpr int NF = SPEC ? kRecFieldsSpec : kRecFieldsDiffuse;
            float rv[NF];
            uint32_t cto = 0;  // the owner's pool chunks (uniform branch: its ds_bpermute sees every lane)
            if (__ballot(sl >= nl)) cto = (uint32_t)__shfl((int)ctab, ow);
            if (sl < nl) {  // LDS slot (typed: ds_read, see bins_add)
              const lds_f32 *r = (const lds_f32 *)lds_rec + (tid & ~63) + (valid ? ow : lane) + (size_t)sl * kBlock;
              const size_t fl = (size_t)nl * kBlock;
#pragma unroll
              for (int f = 0; f < NF; ++f) rv[f] = r[f * fl];
            } else {  // global slot
              const int gs = sl - nl;
              const uint32_t c = (cto >> (6 * (gs / kPoolSlots))) & 63u;
              const gbl_f32 *r = upool + ((size_t)c * kPoolSlots + (size_t)(gs % kPoolSlots)) * NF;
#pragma unroll
              for (int f = 0; f < NF; ++f) rv[f] = r[f];
            }
            f0 = valid ? __float_as_uint(rv[0]) : 0u;
            es = rv[1];
            ck = rv[2];
            if (SPEC) {
              sdv = rv[kRecSD];
              si = rv[kRecSD + 1];
            }
            // (wave-uniform skips: a chunk from vertex 0 has Mlo = 1, and only
            // replay chunks, which paths longer than the ring make, read Scar)
            if (kSub > 0) {  // the sub-chunk's first M: captured by the forward (1 at vertex 0)
              if (__ballot(owns && uslo > 0)) {
                V3 m0 = mk(1.f, 1.f, 1.f);
                if (owns && uslo > 0) {
                  const gbl_f32 *m = umr + (size_t)((uslo - ulo) / kSub) * 192;
                  m0 = mk(m[0], m[1], m[2]);
                }
                Mk = mk(__shfl(m0.x, ow), __shfl(m0.y, ow), __shfl(m0.z, ow));
              }
            } else if (__ballot(owns && ulo > 0)) {
              if (kCarryLds) Mk = carry_get3(3, ow);
              else Mk = mk(__shfl(Mlo.x, ow), __shfl(Mlo.y, ow), __shfl(Mlo.z, ow));
            }
            if (__ballot(owns && !uend)) {
              if (kCarryLds) Sc = carry_get3(0, ow);
              else Sc = mk(__shfl(Scar.x, ow), __shfl(Scar.y, ow), __shfl(Scar.z, ow));
            }
          }
          // (the min()s keep a mis-indexed record from reaching global memory out of bounds)
          const int tk = min((int)(f0 & 0xffffu), nT - 1);
          const int etk = min((int)(f0 >> 16), nT - 1);
          const V3 kee = ke3(etk);
          const V3 lk = mk(kee.x * es, kee.y * es, kee.z * es);  // the forward's lo, same products
          V3 dj = kd3(tk), tv = kdpi3(tk);  // D = kd (+ Ks*specd), T = kd/pi (+ Ks*speci)
          if (SPEC) {
            const TriMat &mj = mat[tk];
            dj = mk(dj.x + mj.ks[0] * sdv, dj.y + mj.ks[1] * sdv, dj.z + mj.ks[2] * sdv);
            tv = mk(tv.x + mj.ks[0] * si, tv.y + mj.ks[1] * si, tv.z + mj.ks[2] * si);
          }
          // prefix (ADJ): M_0 = 1, M_s = (M_{s-1} * T_{s-1}) * c_{s-1} from the left neighbour
          // suffix: S_K = escaped ? Le + D_{K-1} lo_{K-1} : 0 (ADJU replay chunks: Scar),
          // S_j = (Le + D_j lo_j) + (T_j c_j) S_{j+1}
          const V3 A = mk(LeL.x + dj.x * lk.x, LeL.y + dj.y * lk.y, LeL.z + dj.z * lk.z);
          const V3 B = mk(tv.x * ck, tv.y * ck, tv.z * ck);
          V3 S = (esc && rr == 0) ? A : mk(0.f, 0.f, 0.f);
          if (MODE == MODE_ADJU && !fst_o && rr == 0) S = Sc;
          const int kkp = kk;  // prefix chain: task kk takes its left neighbour's M_kk-1 T c
          // both chains in one loop (max(K) - 1 steps instead of up to twice
          // that; two independent dependency chains per step: -0.2..0.6%,
          // profiles/r03/variants_merged_r03o.log)
          const int steps = valid ? max(kkp, rr) : 0;  // this lane's chain steps
          if (__ballot(steps > 0)) {
            // Every lane steps every round: lane i takes lane i-1's (M T) c and
            // lane i+1's A + B S, computed here from the neighbours' operands
            // (shifted once per round; the same float operations as in the
            // neighbour), except a path's first task keeps its M (Mlo / 1) and
            // its last keeps its S.  A lane's value is final after kk (M) / rr
            // (S) steps -- its neighbour's is by then -- and stays so.  (Round 3:
            // a select of the shifted product at step kk only; this form has no
            // per-step compares and one shift fewer per channel.)
            float mx = Mk.x, my = Mk.y, mz = Mk.z, sx = S.x, sy = S.y, sz = S.z;
            int s = 1;
            if (is_badj<MODE>()) {
              const V3 tvl = mk(wave_shr1(tv.x), wave_shr1(tv.y), wave_shr1(tv.z));
              const float ckl = wave_shr1(ck);
              const V3 Al = mk(wave_shl1(A.x), wave_shl1(A.y), wave_shl1(A.z));
              const V3 Bl = mk(wave_shl1(B.x), wave_shl1(B.y), wave_shl1(B.z));
              const bool keepM = kkp == 0, keepS = rr == 0;
              const uint64_t kM = __ballot(keepM), kS = __ballot(keepS);
              do {
                chain_step_shifted(mx, my, mz, sx, sy, sz, tvl, ckl, Al, Bl, kM, kS);
              } while (__ballot(steps > s++));
            } else {  // ADJU (register pressure: no pre-shifted operands; a lane takes its neighbour's value at step kk / rr)
              do {
                chain_step_select(mx, my, mz, sx, sy, sz, tv, ck, A, B, kkp, rr, s);
              } while (__ballot(steps > s++));
            }
            Mk = mk(mx, my, mz);
            S = mk(sx, sy, sz);
#ifdef IPT_PHASE_TIMING
            tacc[22] += (uint64_t)(s - 1);  // chain steps of this round (s: one past the last)
            tacc[23] += 1;
            tacc[24] += (uint64_t)__builtin_amdgcn_readlane(wave_scan_add(steps), 63);
#endif
          }
          // (the owner's adjoint weights are taken only here: their global
          // loads, issued as the sweep starts, finish under the chain)
          const float ax = __shfl(wx, ow), ay = __shfl(wy, ow), az = __shfl(wz, ow);
          // material adjoint: the path's first triangle (the stale Le is Ke[tri_0]),
          // from the lane of the path's task 0 (ADJ: every chunk starts at vertex 0);
          // ADJU: from the owner lane, which carries it like Le (replay chunks start later)
          const int tri0 = kTri0Carry ? tri0c : (MATG ? __shfl(tk, lane - kk) : 0);
          // TANG: this task's fp32 terms a * g (the adjoint's own products) for
          // Kd[tk], Ks[tk], Ke[et_k], Ke[tri_0]; t_ks / t_ek / t_e0: the term exists
          float tg[12];
#pragma unroll
          for (int i = 0; i < 12; ++i) tg[i] = 0.f;
          bool t_ks = false;
          int t_ek = -1, t_e0 = -1;
          if (valid) {
            V3 dLd = Mk;
            if (esc && rr == 0) {  // the escape's stale re-add weights Ld by M_K = (M_K-1 T_K-1) c_K-1
              const V3 ML = mk((Mk.x * tv.x) * ck, (Mk.y * tv.y) * ck, (Mk.z * tv.z) * ck);
              dLd = mk(dLd.x + ML.x, dLd.y + ML.y, dLd.z + ML.z);
            }
            V3 gk = mk(dLd.x * lk.x, dLd.y * lk.y, dLd.z * lk.z);
            if (rr > 0 || esc || !fst_o) {
              const float cpi = div_const<2>(ck);  // ck / kPiF
              gk = mk(gk.x + (cpi * Mk.x) * S.x, gk.y + (cpi * Mk.y) * S.y, gk.z + (cpi * Mk.z) * S.z);
            }
            if (TANG) {
              tg[0] = ax * gk.x, tg[1] = ay * gk.y, tg[2] = az * gk.z;
              if (SPEC && (mat[tk].flags & MAT_HAS_KS)) {
                V3 gs = mk((dLd.x * lk.x) * sdv, (dLd.y * lk.y) * sdv, (dLd.z * lk.z) * sdv);
                if (rr > 0 || esc || !fst_o) {
                  const float cs = ck * si;
                  gs = mk(gs.x + (cs * Mk.x) * S.x, gs.y + (cs * Mk.y) * S.y, gs.z + (cs * Mk.z) * S.z);
                }
                tg[3] = ax * gs.x, tg[4] = ay * gs.y, tg[5] = az * gs.z;
                t_ks = true;
              }
              t_ek = es != 0.f ? tri_emit[etk] : -1;
              if (t_ek >= 0) tg[6] = ax * ((dLd.x * dj.x) * es), tg[7] = ay * ((dLd.y * dj.y) * es), tg[8] = az * ((dLd.z * dj.z) * es);
              t_e0 = tri_emit[min(tri0, nT - 1)];
              if (t_e0 >= 0) tg[9] = ax * dLd.x, tg[10] = ay * dLd.y, tg[11] = az * dLd.z;
            } else {
            const int sl = a.grad_map ? a.grad_map[tk] : tk;
            const double v[3] = {(double)(ax * gk.x), (double)(ay * gk.y), (double)(az * gk.z)};
            double *grad = karg<double *>(offsetof(TraceKernArgs, grad)) + (VSETS ? (size_t)mset * 9 * a.nT : !VIEWS && a.nscenes > 1 ? (size_t)set * (MATG ? 9 : 3) * a.nT : 0);
            bins_add(sl >= 0, grad, sl >= 0 ? (size_t)sl * 3 : (size_t)tk * 3, 3, v);
            if (MATG) {  // dL/dKs[tk], dL/dKe[et_k], dL/dKe[tri_0] (global layout [Kd | Ks | Ke], nT*3 each)
              const size_t gs3 = (size_t)a.grad_slots * 3;
              if (SPEC && (mat[tk].flags & MAT_HAS_KS)) {
                // (dLd lo) specd + ((c speci) M_k) S_k+1, the second term as for Kd
                V3 gs = mk((dLd.x * lk.x) * sdv, (dLd.y * lk.y) * sdv, (dLd.z * lk.z) * sdv);
                if (rr > 0 || esc || !fst_o) {
                  const float cs = ck * si;
                  gs = mk(gs.x + (cs * Mk.x) * S.x, gs.y + (cs * Mk.y) * S.y, gs.z + (cs * Mk.z) * S.z);
                }
                const double vs[3] = {(double)(ax * gs.x), (double)(ay * gs.y), (double)(az * gs.z)};
                bins_add(sl >= 0, grad, sl >= 0 ? gs3 + (size_t)sl * 3 : (size_t)(nT + tk) * 3, 3, vs);
              }
              // Ke bins by emitter index, always in LDS
              const size_t ke0 = gs3 * (SPEC ? 2 : 1);
              const int ek = es != 0.f ? tri_emit[etk] : -1;  // s = 0: the shadow ray did not find its emitter
              if (ek >= 0) {  // (dLd D_k) s_k
                const double ve[3] = {(double)(ax * ((dLd.x * dj.x) * es)), (double)(ay * ((dLd.y * dj.y) * es)),
                                      (double)(az * ((dLd.z * dj.z) * es))};
                bins_add(true, grad, ke0 + (size_t)ek * 3, 3, ve);
              }
              const int e0 = tri_emit[min(tri0, nT - 1)];
              if (e0 >= 0) {  // the stale Le, re-added at every vertex: dLd
                const double v0[3] = {(double)(ax * dLd.x), (double)(ay * dLd.y), (double)(az * dLd.z)};
                bins_add(true, grad, ke0 + (size_t)e0 * 3, 3, v0);
              }
            }
            }
          }
          if (TANG) {
            // Per tangent k and channel: the task's terms, widened, times the
            // tangents' entries (fp64), summed over the consecutive task lanes of
            // ONE PATH by a segmented inclusive scan; the path's last task lane
            // adds the total to its pixel's entry (one fp64 atomic per path, k and
            // channel instead of one per task).  Paths that share a pixel are not
            // combined before the atomics.
            const uint32_t plo = (uint32_t)__shfl((int)tlp_lo, ow), phi = (uint32_t)__shfl((int)tlp_hi, ow);
            const bool head = !valid || kk == 0;
            const int soff = lane - ((int)wave_scan_max(head ? (uint32_t)lane + 1u : 0u) - 1);  // lanes since the segment's first
            const uint64_t hb = __ballot(head);
            const bool tail = valid && (lane == 63 || ((hb >> (lane + 1)) & 1ull));
            uint64_t lp = ((uint64_t)phi << 32) | plo;
            lp = lp < a.npix ? lp : a.npix - 1;  // (nothing reaches global memory out of bounds)
            const int nk = ntan * nT * 3;
            const int tri0t = min(tri0, nT - 1);
            const gbl_f32 *gkd = nullptr, *gks = nullptr, *gke = nullptr;
            if (!a.kd_tables) {  // large scenes: the tangents by triangle, from global memory
              gkd = (const gbl_f32 *)karg<const float *>(sizeof(TraceKernArgs) + sizeof(void *));
              gks = (const gbl_f32 *)karg<const float *>(sizeof(TraceKernArgs) + 2 * sizeof(void *));
              gke = (const gbl_f32 *)karg<const float *>(sizeof(TraceKernArgs) + 3 * sizeof(void *));
            }
            gbl_f64 *tout = (gbl_f64 *)karg<double *>(offsetof(TraceKernArgs, grad)) + lp * 3;
            for (int kq = 0; kq < ntan; ++kq) {  // wave-uniform
              double c[3] = {0.0, 0.0, 0.0};
              if (valid) {
                if (a.kd_tables) {
                  const lds_f32 *tt = (const lds_f32 *)lds_acc;
                  const lds_f32 *q = tt + ((size_t)kq * nT + tk) * 3;
#pragma unroll
                  for (int i = 0; i < 3; ++i) c[i] = (double)tg[i] * (double)q[i];
                  if (SPEC && t_ks) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[3 + i] * (double)q[nk + i];
                  }
                  const lds_f32 *te = tt + (SPEC ? 2 : 1) * nk + (size_t)kq * nE * 3;
                  if (t_ek >= 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[6 + i] * (double)te[t_ek * 3 + i];
                  }
                  if (t_e0 >= 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[9 + i] * (double)te[t_e0 * 3 + i];
                  }
                } else {
                  const size_t r = ((size_t)kq * nT + tk) * 3;
                  if (gkd) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] = (double)tg[i] * (double)gkd[r + i];
                  }
                  if (SPEC && gks && t_ks) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[3 + i] * (double)gks[r + i];
                  }
                  if (gke && t_ek >= 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[6 + i] * (double)gke[((size_t)kq * nT + etk) * 3 + i];
                  }
                  if (gke && t_e0 >= 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) c[i] += (double)tg[9 + i] * (double)gke[((size_t)kq * nT + tri0t) * 3 + i];
                  }
                }
              }
              for (int d = 1; __ballot(soff >= d); d <<= 1) {  // (soff <= 63: at most six steps)
                const double u0 = __shfl_up(c[0], d), u1 = __shfl_up(c[1], d), u2 = __shfl_up(c[2], d);
                if (soff >= d) c[0] += u0, c[1] += u1, c[2] += u2;
              }
              if (tail) {
                gbl_f64 *o = tout + (size_t)kq * a.npix * 3;
#pragma unroll
                for (int i = 0; i < 3; ++i)
                  if (c[i] != 0.0) __hip_atomic_fetch_add(o + i, c[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
            }
          }
          if (MODE == MODE_ADJU && __ballot(owns && (urep > 0 || uslo > ulo))) {  // the suffix at the chunk's first vertex, S_lo = A + B S, back to its owner (for its replay)
            const V3 H = mk(A.x + B.x * S.x, A.y + B.y * S.y, A.z + B.z * S.z);
            const int sa = (owns ? st0 : lane) << 2;
            const V3 Hs = mk(bperm_f(sa, H.x), bperm_f(sa, H.y), bperm_f(sa, H.z));
            if (owns) {
              if (kCarryLds) carry_put3(0, Hs);
              else Scar = Hs;
            }
          }
          base = next;
        }
      }
      // IPT_ADJU_SUB: a lane whose chunk has sub-chunks left sweeps the next
      // one in the next iteration (neither traced nor refilled meanwhile)
      const bool umore = MODE == MODE_ADJU && kSub > 0 && (finished || upend) && uslo > ulo;
      if (MODE == MODE_ADJU && kSub > 0) usub = umore ? uslo : 0;
      if (MODE == MODE_ADJU) {  // a path swept to its first vertex gives its pool chunks back
        const bool rel = (finished || upend) && !umore && urep == 0 && (ctab & kNoChunks) != kNoChunks;
        uint64_t rm = __ballot(rel);
        if (rm) {
          uint64_t mine = 0;
#pragma unroll
          for (int j = 0; j < kPoolMaxChunks; ++j) {
            const uint32_t c = (ctab >> (6 * j)) & 63u;
            if (c != 63u) mine |= 1ull << c;
          }
          do {
            const int l = (int)__builtin_ctzll(rm);
            rm &= rm - 1;
            pfree |= (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, l) |
                     ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), l) << 32);
          } while (rm);
          if (rel) ctab |= kNoChunks;
        }
      }
      if (MODE == MODE_ADJU && urep > 0 && !umore) {  // replay the path from its camera ray (see the chunk choice)
        int r, c;
        item_ray(a, seed, witem(), st, p, d, r, c);
        L = mk(0.f, 0.f, 0.f);
        set_le(L);
        Ld = L;
        M = mk(1.f, 1.f, 1.f);
        Mlo = M;
        k = 0;
        set_ptri(-1);
        rslot = 0;
        rhi = urep;
        active = true;
      }
    }
    PHASE(5)
  }
#ifdef IPT_PHASE_TIMING
  if ((tid & 63) == 0)
    for (int i = 0; i < kPhaseWords; ++i) atomicAdd(&g_phase_cycles[i], (unsigned long long)tacc[i]);
#endif
  }

  if (!is_fwd<MODE>()) {
    __syncthreads();
    if (!TANG && n_acc > 0) {
      double *dstp = is_adj<MODE>() ? karg<double *>(offsetof(TraceKernArgs, grad)) + (VSETS ? (size_t)mset * 9 * a.nT : !VIEWS && a.nscenes > 1 ? (size_t)set * (MATG ? 9 : 3) * a.nT : 0)
                                    : edges;
      const int nb5 = (nT + 1) * nT * kEdgeL;
      for (int i = tid; i < n_acc; i += nthr) {
        const double v = lds_acc[i];
        int j = (!MATG && is_adj<MODE>() && a.slot_tri) ? a.slot_tri[i / 3] * 3 + i % 3 : i;
        if (MATG) {  // [Kd slots][Ks slots (SPEC)][Ke by emitter] -> [Kd | Ks | Ke] by triangle
          const int gs3 = a.grad_slots * 3, ke0 = gs3 * (SPEC ? 2 : 1);
          const int blk = i >= ke0 ? 2 : (i >= gs3 ? 1 : 0);      // Ke, Ks, Kd
          const int q = i - (blk == 2 ? ke0 : blk * gs3);         // index inside the block's bins
          const int t = blk == 2 ? emit_tri[q / 3] : (a.slot_tri ? a.slot_tri[q / 3] : q / 3);
          j = (blk * nT + t) * 3 + q % 3;
        }
        if (MODE == MODE_GRAPH) {  // LDS form -> kEdgeW-wide global bins
          if (i < nb5) {
            j = (i / kEdgeL) * kEdgeW + i % kEdgeL;
          } else {
            const int q = i - nb5, dst = q / (3 * nE), ie = (q / 3) % nE;
            j = (dst * nT + emit_tri[ie]) * kEdgeW + kEdgeL + q % 3;
          }
        }
        if (v != 0.0) atomicAdd(dstp + j, v);
      }
    }
  }
