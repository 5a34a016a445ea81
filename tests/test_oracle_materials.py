"""The oracle's material adjoint (oro_adjoint_mat, oro_set_material_params): CPU only.

tests/test_gpu_materials_oracle.py compares every entry of the kernels' Kd, Ks
and Ke blocks with OracleScene.adjoint_materials, so that code is pinned here
first, by the identities the GPU suites were written around and on the frames
their bars were calibrated on (scene A / scene B of test_gpu_materials.py,
32x32x8, seed 11, pos_adj):
  * the Kd block is oro_adjoint's, bit for bit at equal thread count;
  * Ke, every emitter entry: F(Ke) - F(Ke with the entry zeroed) through the
    oracle's forward equals Ke[e, c] * gKe[e, c] (the radiance is linear in Ke);
  * Ks, every lobe entry: the five-point stencil through the oracle's forward;
  * the setter's masks, the frozen structure, a round trip;
  * on every frame of the GPU file: the fp64 summation-order noise between 1
    and 16 threads (at most 1e-11, a hundredth of the GPU bar) and the
    coverage conditions the GPU tests rely on, from the oracle's own counters.

This module also owns what the GPU file shares with it: the frames, the
material values and the coverage checks (imported there, not copied).
"""
import collections

import numpy as np
import pytest

import scene_ladder as SL
import test_gpu_materials_unbounded as MU
from conftest import CORNELL, CUBE_OBJ, SCENE0
from test_gpu_materials import (H_KS, REL_KE, TOL_KS_ENTRY, bits, dot64, oracle_hdr, pos_adj, scene_a, scene_b,
                                stencil)
from test_gpu_shadow_pair import write_glow

# ------------------------------------------------------------------ shared with the GPU file
RTOL, ATOL = 1e-9, 1e-12  # the Kd block's bar since the first adjoint (test_gpu.py)
NOISE = 1e-11             # the reference's own thread-order noise must stay a hundred times below RTOL
LONG = 17                 # vertices: a path this long replays under the tiny rings (1 and 17 slots)

# rows: (begin, end, step) or None for the full frame; adj: ("signed" | "pos", RandomState seed)
Frame = collections.namedtuple("Frame", "W H spp mb seed rows adj")


def F(W, H, spp, mb, seed, rows=None, adj=None):
    return Frame(W, H, spp, mb, seed, rows, adj or ("signed", W + spp))


B_BOUNDED = [F(32, 32, 8, 4, 11), F(20, 12, 3, 5, 2 ** 33 + 5), F(24, 16, 5, 20, 7), F(16, 16, 4, 0, 2),
             F(30, 21, 5, 1, 3, (1, 21, 3)), F(30, 30, 5, 3, 9, (9, 16, 1))]
B_UNBOUNDED = [F(32, 32, 8, None, 11), F(19, 13, 7, None, 2 ** 33 + 11), F(30, 21, 5, None, 3, (1, 21, 3))]
GLOW = [F(24, 16, 5, 4, 6), F(24, 16, 5, None, 6)]
SPHERE = [F(32, 24, 8, 4, 12), F(32, 24, 8, None, 12)]
# The 32x24x8 frame puts 510 (bounded) / 836 (unbounded) vertices on the sphere and leaves 110 / 139 Ks rows
# non-zero (330 / 417 entries): the Phong coefficient is exactly 0 at most vertices.  The smallest frame of this
# seed and aspect with at least 200 non-zero rows is 48x36x8 (204 / 235), so the sphere runs that one as well.
SPHERE_WIDE = [F(48, 36, 8, 4, 12), F(48, 36, 8, None, 12)]
BATCH_B = [F(32, 32, 8, 4, 11), F(32, 32, 8, 4, 11, (1, 32, 2))]
BATCH_GLOW = [F(24, 16, 5, 4, 6)]
N_SETS = 3
MAIN = {B_BOUNDED[0], B_UNBOUNDED[0], BATCH_B[0], BATCH_B[1]} | set(GLOW + SPHERE + SPHERE_WIDE + BATCH_GLOW)


def frame_id(f):
    rows = "" if f.rows is None else "-rows%d:%d:%d" % f.rows
    return "%dx%dx%d-mb%s-seed%d%s" % (f.W, f.H, f.spp, f.mb, f.seed, rows)


def frame_rows(f):
    return f.rows or (0, f.H, 1)


def frame_adj(f, b=0):
    kind, seed = f.adj
    if kind == "pos":
        return pos_adj(f.W, f.H, seed + b)
    return np.random.RandomState(seed + b).uniform(-1, 1, (f.H, f.W, 3)).astype(np.float32)


def glow_records(tmp):
    """The scenes/0 geometry with the cube emissive (test_gpu_shadow_pair.py): 30 triangles, 14 emitters, no lobe."""
    obj, mtl = write_glow(tmp, "glowcube", open(CUBE_OBJ).read())
    return CORNELL + [(SCENE0[1][0], SCENE0[1][1], SCENE0[1][2], obj, mtl)]


def emitter_objects(Q):
    """The emitter triangles per emitting object: the Cornell light (object 0, 18 triangles) and the rest."""
    e = np.flatnonzero(Q.emitter_mask)
    return [g for g in (e[e < 18], e[e >= 18]) if len(g)]


def hot_set(Q):
    """bool (nT,): the triangles whose gradient bins live in LDS when there are more triangles than bins -- the
    512 largest by area, ties in index order; the other rows go straight to global memory."""
    hot = np.zeros(Q.nT, bool)
    hot[np.argsort(-Q.triangles()[:, 24], kind="stable")[:512]] = True
    return hot


def facing(Q, rows):
    """Of the triangles `rows`, the one whose face looks most squarely at the camera (at the origin)."""
    t = Q.triangles()[rows].astype(np.float64)
    n, c = t[:, 18:21], t[:, 21:24]
    return int(rows[np.argmin((n * c).sum(1) / np.linalg.norm(c, axis=1))])


PROBE = (64, 48, 8, 4, 1)  # W, H, spp, mb, seed


def zero_rows(Q):
    """(lobe triangle or None, one emitter triangle per emitting object): the rows that get all-zero values.
    Emitters: the triangle of each object that faces the camera most squarely.  The lobe triangle: the Phong
    coefficient is exactly 0 wherever the mirrored light direction points away from the viewer, which on a
    triangle seen head-on is everywhere, so of the camera-facing lobe triangles the one with the largest Ks
    gradient on a probe frame of the oracle is taken (paths and flags do not depend on the values)."""
    if getattr(Q, "_zero_rows", None) is None:
        lobe = np.flatnonzero(Q.lobe_mask)
        zl = None
        if len(lobe):
            t = Q.triangles()[lobe].astype(np.float64)
            front = (t[:, 18:21] * t[:, 21:24]).sum(1) < 0
            W, H, spp, mb, seed = PROBE
            g = np.abs(Q.adjoint_materials(W, H, spp, mb, seed, pos_adj(W, H))[1][lobe]).sum(1)
            zl = int(lobe[np.argmax(np.where(front, g, -1.0))])
        Q._zero_rows = (zl, [facing(Q, g) for g in emitter_objects(Q)])
    return Q._zero_rows


def draw_values(Q, n_sets=1, junk=True):
    """n_sets x (kd, ks, ke), (nT, 3) float32 each, from one RandomState(5): Kd in U(0.05, 0.95), Ks in
    U(0.05, 0.6) on lobe rows, Ke in U(0.5, 12) on emitter rows, every row distinct; the rows of zero_rows()
    all-zero.  junk: the rows outside the masks carry junk, which every setter and the pack kernel must force to 0
    (as test_forward_with_overrides_is_the_oracles does)."""
    rs = np.random.RandomState(5)
    lobe, emit = Q.lobe_mask, Q.emitter_mask
    zl, ze = zero_rows(Q)
    sets = []
    for _ in range(n_sets):
        kd = rs.uniform(0.05, 0.95, (Q.nT, 3)).astype(np.float32)
        ks = rs.uniform(0.05, 0.6, (Q.nT, 3)).astype(np.float32)
        ke = rs.uniform(0.5, 12, (Q.nT, 3)).astype(np.float32)
        ks[~lobe] = 0.77 if junk else 0
        ke[~emit] = 5.0 if junk else 0
        if zl is not None:
            ks[zl] = 0
        ke[ze] = 0
        sets.append((kd, ks, ke))
    return sets


def reference(Q, f, b=0, stride=0):
    """(gkd, gks, gke, stats) of frame f from the oracle (set b of a batch: seed + b * stride, adjoint image b)."""
    return Q.adjoint_materials(f.W, f.H, f.spp, f.mb, f.seed + b * stride, frame_adj(f, b), *frame_rows(f), stats=True)


def first_hit_rows(Q, f):
    """bool (nT,): the emitters that are some path's first triangle.  With Kd = Ks = 0 every throughput past
    vertex 0 and every D_k is 0, so a Ke row is non-zero exactly if a camera ray of the frame hits it."""
    kd, ks, ke = Q.material_params()
    Q.set_material_params(kd=np.zeros_like(kd), ks=np.zeros_like(ks))
    try:
        g = Q.adjoint_materials(f.W, f.H, f.spp, f.mb, f.seed, pos_adj(f.W, f.H), *frame_rows(f))[2]
    finally:
        Q.set_material_params(kd=kd, ks=ks)
    return np.any(g != 0, axis=1)


def check_coverage(Q, f, stats, gks=None, zeroed=None, sphere=False):
    """The conditions under which frame f reaches what the GPU tests are about, from the oracle alone."""
    assert stats["paths"] > 0 and stats["vertices"] >= stats["paths"] and stats["shadow_found"] > 0
    # (an escape is a continuation ray that misses: there is none without a bounce)
    assert stats["escaped"] > 0 or f.mb == 0, "no escaped path: the stale re-add at the last vertex is not reached"
    if f.mb is None or f.mb >= LONG - 1:
        assert stats["longest"] >= LONG, "longest path %d: the tiny rings do not replay" % stats["longest"]
    if sphere:  # Ks through the hot-set bin map and straight to global memory, and at least 200 rows of it
        nz, hot = np.any(gks != 0, axis=1), hot_set(Q)
        assert Q.nT > 512 and (nz & hot).any() and (nz & ~hot).any()
        assert nz.sum() >= 200 or f not in SPHERE_WIDE, nz.sum()
    elif f in MAIN:  # per scene: the bands and the smallest frames do not see both emitter objects
        assert stats["tri0_emitter"] > 0
        hit = first_hit_rows(Q, f)
        for g in emitter_objects(Q):
            assert hit[g].any(), "no camera ray of this frame hits emitter object %s" % g
    # (gks row or None, gke rows) of the triangles that carry all-zero values.  Asserted on the first frame of
    # each instance: the Phong coefficient is exactly 0 on most vertices (a negative cosine under the power), so a
    # frame of a few hundred samples may leave one chosen triangle's Ks row at 0 by chance; there the row is
    # compared like every other, and each instance still meets a zero-valued row with a gradient.
    if zeroed is not None and f in MAIN:
        for row in zeroed:
            assert row is None or np.any(row != 0), "a zero-valued row gets no gradient on this frame"


def rel_diff(got, want):
    """Largest |got - want| / |want| over the non-zero entries of want (0 if there are none)."""
    nz = want != 0
    return float(np.max(np.abs(got - want)[nz] / np.abs(want)[nz])) if nz.any() else 0.0


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("oracle_materials")


@pytest.fixture(scope="module")
def QA(oracle):
    return oracle.OracleScene(scene_a())


@pytest.fixture(scope="module")
def QB(oracle, tmp):
    return oracle.OracleScene(scene_b(tmp))


def forward_F(oracle, Q, adj, W, H, spp, mb, seed):
    return dot64(adj, oracle_hdr(oracle, Q, W, H, spp, mb, seed))


# ------------------------------------------------------------------ 1. structure, masks, round trip
def test_setter_masks_and_structure_is_frozen(oracle, QA, QB):
    for Q in (QA, QB):
        kd0, ks0, ke0 = Q.material_params()
        t = Q.triangles()
        assert np.array_equal(kd0, t[:, 25:28]) and np.array_equal(ks0, t[:, 28:31]) and np.array_equal(ke0, t[:, 31:34])
        lobe, emit = Q.lobe_mask, Q.emitter_mask
        assert np.array_equal(lobe, np.any(ks0 != 0, axis=1)) and np.array_equal(emit, t[:, 56] >= 0)
        assert emit.sum() == Q.nE
        Q.set_material_params(ks=np.full((Q.nT, 3), 0.77, np.float32), ke=np.full((Q.nT, 3), 5.0, np.float32))
        kd, ks, ke = Q.material_params()
        assert np.array_equal(kd, kd0)
        assert np.all(ks[~lobe] == 0) and np.all(ks[lobe] == np.float32(0.77))
        assert np.all(ke[~emit] == 0) and np.all(ke[emit] == 5)
        Q.set_material_params(ks=np.zeros((Q.nT, 3), np.float32), ke=np.zeros((Q.nT, 3), np.float32))
        assert np.array_equal(Q.lobe_mask, lobe) and np.array_equal(Q.emitter_mask, emit) and Q.nE == emit.sum()
        Q.set_material_params(kd0, ks0, ke0)
    assert QA.lobe_mask.sum() == 12 and QA.emitter_mask.sum() == 2 and QB.emitter_mask.sum() == 14


@pytest.mark.parametrize("mb", [3, None])
def test_round_trip_restores_the_samples(QB, mb):
    """A lobe row and an emitter row set to zero change the samples; set back, the samples are the first ones, bit
    for bit -- which they cannot be if zeroing a row changed the emitter list or the sampling branch."""
    Q = QB
    c = (32, 32, 8, mb, 11)
    kd0, ks0, ke0 = Q.material_params()
    s0, casts0 = Q.render_samples(*c)
    zl, ze = zero_rows(Q)
    ks, ke = ks0.copy(), ke0.copy()
    ks[zl] = 0
    ke[ze] = 0
    Q.set_material_params(ks=ks, ke=ke)
    s1, casts1 = Q.render_samples(*c)
    assert casts1 == casts0, "the paths moved with the values"
    assert not np.array_equal(bits(s1), bits(s0))
    Q.set_material_params(ks=ks0, ke=ke0)
    s2, _ = Q.render_samples(*c)
    assert np.array_equal(bits(s2), bits(s0))


# ------------------------------------------------------------------ 2. the Kd block
@pytest.mark.parametrize("threads", [1, 16])
@pytest.mark.parametrize("mb,rows", [(4, (0, 32)), (None, (0, 32)), (3, (9, 20)), (None, (9, 20))])
def test_kd_block_is_oro_adjoint_bit_for_bit(oracle, QA, QB, threads, mb, rows):
    oracle.lib().oro_set_threads(threads)
    try:
        for Q in (QA, QB):
            adj = np.random.RandomState(32).uniform(-1, 1, (32, 32, 3)).astype(np.float32)
            gkd, gks, gke = Q.adjoint_materials(32, 32, 8, mb, 4, adj, *rows)
            want = Q.adjoint(32, 32, 8, mb, 4, adj, *rows)
            assert np.array_equal(gkd.view(np.uint64), want.view(np.uint64))
            assert np.all(gks[~Q.lobe_mask] == 0) and np.any(gks[Q.lobe_mask] != 0)
            assert np.all(gke[~Q.emitter_mask] == 0) and np.all(gke[Q.emitter_mask] != 0)
    finally:
        oracle.lib().oro_set_threads(0)


def test_row_step_is_the_masked_full_frame(QB):
    """rows 1::3 are the full frame under an adjoint image that is 0 elsewhere (to fp64 summation order)."""
    W, H, spp, seed = 30, 21, 5, 3
    adj = pos_adj(W, H)
    masked = np.zeros_like(adj)
    masked[1::3] = adj[1::3]
    for mb in (1, None):
        got = np.stack(QB.adjoint_materials(W, H, spp, mb, seed, adj, 1, H, 3))
        want = np.stack(QB.adjoint_materials(W, H, spp, mb, seed, masked))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
        assert np.array_equal(got == 0, want == 0) and np.any(got[2] != 0)


# ------------------------------------------------------------------ 3. Ke, every emitter entry
def distinct_ke(Q):
    ke = Q.material_params()[2]
    ke[Q.emitter_mask] = np.random.RandomState(5).uniform(0.5, 12, (Q.nE, 3)).astype(np.float32)
    return ke


@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("mb,rel", [(3, REL_KE), (None, MU.REL_KE)])
def test_ke_every_emitter_entry(oracle, QB, mb, rel, distinct):
    """The radiance is linear in each Ke entry, so zeroing entry (e, c) moves F = sum(adj * I) by
    Ke[e, c] * gKe[e, c].  The bar is the homogeneity identity's own (REL_KE |F|, calibrated on the oracle's Kd
    adjoint on this frame; the unbounded module's constant for the unbounded estimator).  Second round: every
    emitter triangle its own Ke, so a term credited to a neighbour of the same object is off by the ratio."""
    Q = QB
    W = H = 32
    spp, seed = 8, 11
    adj = pos_adj(W, H)
    ke_load = Q.material_params()[2]
    ke0 = distinct_ke(Q) if distinct else ke_load
    try:
        Q.set_material_params(ke=ke0)
        F0 = forward_F(oracle, Q, adj, W, H, spp, mb, seed)
        gke = Q.adjoint_materials(W, H, spp, mb, seed, adj)[2]
        emit = np.flatnonzero(Q.emitter_mask)
        assert len(emit) == 14
        worst = 0.0
        for e in emit:
            for c in range(3):
                ke = ke0.copy()
                ke[e, c] = 0
                Q.set_material_params(ke=ke)
                d = F0 - forward_F(oracle, Q, adj, W, H, spp, mb, seed)
                got = float(ke0[e, c]) * gke[e, c]
                worst = max(worst, abs(got - d) / (rel * abs(F0)))
                assert abs(got - d) <= rel * abs(F0), (e, c, got, d)
                assert d != 0
        print("Ke entries mb %s distinct %s: worst %.2e of the bar (F = %.9g)" % (mb, distinct, worst, F0))
    finally:
        Q.set_material_params(ke=ke_load)


# ------------------------------------------------------------------ 4. Ks, every lobe entry
@pytest.mark.parametrize("mb,centre,h", [(1, 0.5, H_KS), (2, 0.5, H_KS), (3, 0.5, H_KS), (3, 0.25, H_KS)])
def test_ks_every_lobe_entry(oracle, QA, mb, centre, h):
    """The five-point stencil (exact for mb <= 3: degree <= 4 in one entry) through the oracle's forward and the
    new setter, all 12 x 3 entries of the cube.  Centred at 0.25 the stencil's outer point is Ks = 0 exactly:
    it holds only if a lobe triangle with a zero entry keeps its lobe (the frozen flags)."""
    Q = QA
    W = H = 32
    spp, seed = 8, 11
    adj = pos_adj(W, H)
    ks_load = Q.material_params()[1]
    lobe = np.flatnonzero(Q.lobe_mask)
    assert len(lobe) == 12
    ks0 = ks_load.copy()
    ks0[lobe] = np.float32(centre)
    try:
        Q.set_material_params(ks=ks0)
        gks = Q.adjoint_materials(W, H, spp, mb, seed, adj)[1]
        worst = 0.0
        for ti in lobe:
            for c in range(3):
                def f(t):
                    ks = ks0.copy()
                    ks[ti, c] = np.float32(centre + t)
                    Q.set_material_params(ks=ks)
                    return forward_F(oracle, Q, adj, W, H, spp, mb, seed)
                want = stencil(f, h)
                worst = max(worst, abs(gks[ti, c] - want) / TOL_KS_ENTRY)
                assert abs(gks[ti, c] - want) <= TOL_KS_ENTRY, (ti, c, gks[ti, c], want)
        assert np.count_nonzero(gks[lobe]) > 12
        print("Ks entries mb %d centre %g: worst %.2e of the bar" % (mb, centre, worst))
    finally:
        Q.set_material_params(ks=ks_load)


def test_all_zero_rows_keep_their_gradient(QB):
    """§13.1: a lobe triangle with all-zero Ks and emitters with all-zero Ke still get their rows."""
    Q = QB
    kd0, ks0, ke0 = Q.material_params()
    zl, ze = zero_rows(Q)
    try:
        Q.set_material_params(*draw_values(Q)[0])
        kd, ks, ke = Q.material_params()
        assert np.all(ks[zl] == 0) and np.all(ke[ze] == 0) and np.all(ks[~Q.lobe_mask] == 0)
        assert len(np.unique(ke[Q.emitter_mask], axis=0)) == 13 and len(np.unique(ks[Q.lobe_mask], axis=0)) == 12
        for mb in (4, None):
            _, gks, gke = Q.adjoint_materials(32, 32, 8, mb, 11, pos_adj(32, 32))
            assert np.all(gks[zl] != 0) and np.all(gke[ze] != 0)
    finally:
        Q.set_material_params(kd0, ks0, ke0)


# ------------------------------------------------------------------ 5. the frames of the GPU file
def _scene(oracle, tmp, name):
    if name == "B":
        return oracle.OracleScene(scene_b(tmp, tag="g"))
    if name == "glow":
        return oracle.OracleScene(glow_records(tmp))
    if name.startswith("ladder:"):
        return oracle.OracleScene(SL.records(tmp, name[len("ladder:"):]))
    return oracle.OracleScene(MU.sphere_records(tmp))


GPU_FRAMES = ([("B", f, 1) for f in B_BOUNDED + B_UNBOUNDED] + [("glow", f, 1) for f in GLOW] +
              [("sphere", f, 1) for f in SPHERE + SPHERE_WIDE] + [("B", f, N_SETS) for f in BATCH_B] +
              [("glow", f, N_SETS) for f in BATCH_GLOW])
# the generated scenes of tests/test_gpu_scene_ladder.py (scene_ladder.py): the material adjoint's two frames on every
# rung with emitting or lobe shards, the 3-set batch, and the tangent rungs' frame
LADDER = {n: tuple(F(*f) for f in SL.mat_frames(n)) for n in SL.MAT_RUNGS}  # (bounded, unbounded)
LADDER_TAN = {n: F(*f) for n, (_, f, _) in SL.TANGENTS.items()}
GPU_FRAMES += ([("ladder:" + n, f, 1) for n in SL.MAT_RUNGS for f in LADDER[n]] +
               [("ladder:" + n, LADDER[n][0], N_SETS) for n in SL.MAT_BATCH_RUNGS] +
               [("ladder:" + n, f, 1) for n, f in LADDER_TAN.items()])
_SCENES = {}


@pytest.mark.parametrize("name,f,n_sets", GPU_FRAMES, ids=["%s-%s-S%d" % (n, frame_id(f), s) for n, f, s in GPU_FRAMES])
def test_gpu_frames_noise_and_coverage(oracle, tmp, name, f, n_sets):
    """What the GPU comparison needs of its reference, on every frame it uses: the oracle at 1 and at 16 threads
    (another split of the samples, another fp64 summation order) agrees to 1e-11 on every entry of every block --
    a hundredth of the GPU bar, so an entry that fails on the GPU is not the reference's own cancellation -- and
    the frame reaches the paths the GPU test is about."""
    if name not in _SCENES:
        _SCENES[name] = _scene(oracle, tmp, name)
    Q = _SCENES[name]
    sets = draw_values(Q, n_sets)
    zl, ze = zero_rows(Q)
    stride = f.W * f.H * f.spp
    try:
        for b, vals in enumerate(sets):
            Q.set_material_params(*vals)
            oracle.lib().oro_set_threads(1)
            g1 = np.stack(reference(Q, f, b, stride)[:3])
            oracle.lib().oro_set_threads(16)
            *g16, stats = reference(Q, f, b, stride)
            g16 = np.stack(g16)
            assert np.array_equal(g1 == 0, g16 == 0)
            noise = [rel_diff(a, w) for a, w in zip(g1, g16)]
            print("thread-order noise %s %s set %d: Kd %.2e Ks %.2e Ke %.2e; %s" %
                  (name, frame_id(f), b, noise[0], noise[1], noise[2], stats))
            assert max(noise) <= NOISE, noise
            zeroed = [None if zl is None else g16[1][zl]] + [g16[2][e] for e in ze]
            check_coverage(Q, f, stats, g16[1], zeroed, sphere=name == "sphere")
            if name == "glow":
                assert np.all(g16[1] == 0)
    finally:
        oracle.lib().oro_set_threads(0)
