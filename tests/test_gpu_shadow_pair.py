"""The small scenes' shadow cast decides target and partner with one evaluation
of the target's pair (ipt_device.h, shadow_hit_pairs_small) and skips
the cull when no other pair can occlude (run with -m gpu).

Every case sends about 1e5 rays through the probes and compares the culled
shadow cast -- Scene.closest_hit(O, D, targets=tg), and Scene.shadow_hit with
the source triangles, which adds the potential-occluder masks -- against the
brute-force loop Scene.closest_hit(O, D): visibility (index == target) must be
equal, and on visible rays t must be equal bit for bit.
"""
import os

import numpy as np
import pytest

from conftest import CORNELL, CUBE_OBJ, SCENE0, product_scene

pytestmark = pytest.mark.gpu

N = 100000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def verts(P):
    return P.triangles()[:, 0:9].reshape(-1, 3, 3).astype(np.float64)


def emitters(P):
    return np.nonzero(P.triangles()[:, 56] >= 0)[0]


def on_tri(v, idx, rng):
    a, b = rng.uniform(0, 1, (2, len(idx)))
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    return v[idx, 0] + a[:, None] * (v[idx, 1] - v[idx, 0]) + b[:, None] * (v[idx, 2] - v[idx, 0])


def rays(O, pt, scale=1.0):
    D = pt - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return O.astype(np.float32), (D * scale).astype(np.float32)


def check(P, O, D, tg, src, lo=None, hi=None):
    """Both probes against the brute-force loop; returns its (visible, index)."""
    tf, i_f = P.closest_hit(O, D)
    vis_f = i_f == tg
    for tc, ic in (P.closest_hit(O, D, targets=tg), P.shadow_hit(O, D, tg, src)):
        vis_c = ic == tg
        assert np.array_equal(vis_c, vis_f)
        assert np.array_equal(bits(tc[vis_c]), bits(tf[vis_f]))
    if lo is not None:
        assert lo < vis_f.mean() < hi, vis_f.mean()
    return vis_f, i_f


@pytest.fixture(scope="module")
def cornell():
    P = product_scene(CORNELL)
    yield P
    P.close()


@pytest.fixture(scope="module")
def scene0():
    P = product_scene(SCENE0)
    yield P
    P.close()


def write_glow(tmp, name, body):
    """(obj, mtl) in tmp: the OBJ text `body` under one emissive material."""
    mtl = os.path.join(str(tmp), name + ".mtl")
    with open(mtl, "w") as f:
        f.write("newmtl glow\nKd 0.4 0.4 0.4\nKe 3 2 1\n")
    obj = os.path.join(str(tmp), name + ".obj")
    i = body.index("\nf ") + 1
    with open(obj, "w") as f:
        f.write(body[:i] + "mtllib %s.mtl\nusemtl glow\n" % name + body[i:])
    return obj, mtl


@pytest.mark.parametrize("half", [0, 1])
def test_ties_inside_the_emitter_quad(cornell, half):
    """Rays from every Cornell triangle at the light quad's shared diagonal and
    its four vertices, exactly and one ulp off per coordinate: the two light
    triangles tie or nearly tie there.  Target the lower, then the upper one."""
    P = cornell
    v = verts(P)
    emit = emitters(P)
    assert len(emit) == 2 and emit[0] >> 1 == emit[1] >> 1  # one quad, one pair
    rng = np.random.RandomState(41 + half)
    a, b = v[emit[0]], v[emit[1]]
    shared = np.array([p for p in a if (np.abs(b - p).max(1) == 0).any()])
    assert len(shared) == 2
    corners = np.unique(np.concatenate([a, b]), axis=0)
    assert len(corners) == 4
    f = rng.uniform(0, 1, N)
    pt = shared[0] + f[:, None] * (shared[1] - shared[0])
    at_corner = rng.uniform(0, 1, N) < 0.3
    pt[at_corner] = corners[rng.randint(0, 4, int(at_corner.sum()))]
    pt = pt.astype(np.float32)
    step = rng.randint(-1, 2, (N, 3))  # -1, 0 or +1 ulp per coordinate
    pt = np.where(step < 0, np.nextafter(pt, np.float32(-np.inf)),
                  np.where(step > 0, np.nextafter(pt, np.float32(np.inf)), pt)).astype(np.float64)
    src = rng.randint(0, P.nT, N)
    O, D = rays(on_tri(v, src, rng), pt)
    tg = np.full(N, emit[half], np.int32)
    vis, _ = check(P, O, D, tg, src)
    assert 0.01 < vis.mean() < 0.99, vis.mean()  # ties go either way


@pytest.mark.parametrize("with_sources", [False, True])
def test_mixed_targets_in_one_wave(tmp_path, with_sources):
    """Consecutive rays alternate between targets in different pairs: scenes/0's
    geometry with the cube emissive too, so that its faces and the light are
    all emitter triangles (the probes take emitters only as targets)."""
    obj, mtl = write_glow(tmp_path, "glowcube", open(CUBE_OBJ).read())
    P = product_scene(CORNELL + [(SCENE0[1][0], SCENE0[1][1], SCENE0[1][2], obj, mtl)])
    try:
        v = verts(P)
        emit = emitters(P)
        assert P.nT == 30 and len(emit) == 14
        assert len(set(int(e) >> 1 for e in emit)) == 7
        rng = np.random.RandomState(43)
        # ray i aims at emitter pair i mod 7 (either half): neighbours never share a pair
        tg = emit[(2 * np.arange(N) + rng.randint(0, 2, N)) % len(emit)].astype(np.int32)
        assert ((tg[1:] >> 1) != (tg[:-1] >> 1)).all()
        src = rng.randint(0, P.nT, N)
        O, D = rays(on_tri(v, src, rng), on_tri(v, tg, rng))
        if not with_sources:
            src = np.full(N, -1)
        check(P, O, D, tg, src, 0.05, 0.98)
    finally:
        P.close()


FIVE = """v -1 0 -1
v 1 0 -1
v 1 0 1
v -1 0 1
v -0.3 0.5 -0.2
v 0.4 0.5 -0.1
v 0 0.5 0.5
v -0.5 1 -0.5
v 0.5 1 -0.5
v 0.5 1 0.5
v -0.5 1 0.5
f 1 2 3
f 1 3 4
f 5 6 7
f 8 9 10
f 8 10 11
"""


@pytest.mark.parametrize("which", ["last", "neighbour"])
def test_odd_triangle_count(tmp_path, which):
    """Five triangles: a floor quad, a blocker, a quad above it.  The last
    triangle's partner is the pair padding; its neighbour shares a pair with
    the blocker."""
    obj, mtl = write_glow(tmp_path, "five", FIVE)
    P = product_scene([((0, 0, 4), (0, 0, 0), (1, 1, 1), obj, mtl)])
    try:
        assert P.nT == 5 and len(emitters(P)) == 5
        v = verts(P)
        rng = np.random.RandomState(47)
        t = 4 if which == "last" else 3
        tg = np.full(N, t, np.int32)
        src = rng.randint(0, 3, N)  # floor and blocker
        pt = on_tri(v, tg, rng)
        edge = rng.uniform(0, 1, N) < 0.3  # on the quad's diagonal and corners: ties with the other half
        pt[edge] = v[t][rng.randint(0, 3, int(edge.sum()))]
        O, D = rays(on_tri(v, src, rng), pt)
        check(P, O, D, tg, src, 0.05, 0.98)
    finally:
        P.close()


def floor_rays(P, rng, scale=1.0):
    """scenes/0: origins on the floor around the cube's footprint, aimed at the light."""
    v = verts(P)
    emit = emitters(P)
    cube = np.arange(18, P.nT)
    ymin = v[:18].reshape(-1, 3)[:, 1].min()
    floor = np.nonzero((v[:18, :, 1] == ymin).all(1))[0]
    assert len(floor) == 2
    c = v[cube].reshape(-1, 3)
    lo, hi = c.min(0), c.max(0)
    mid, ext = (lo + hi) / 2, (hi - lo)
    O = np.stack([rng.uniform(mid[0] - ext[0], mid[0] + ext[0], N), np.full(N, ymin),
                  rng.uniform(mid[2] - ext[2], mid[2] + ext[2], N)], 1)
    # the floor triangle under each origin (the quad's two halves)
    a, b, cc = v[floor[0]]
    d0, d1, dp = b - a, cc - a, O - a
    den = d0[0] * d1[2] - d1[0] * d0[2]
    u = (dp[:, 0] * d1[2] - d1[0] * dp[:, 2]) / den
    w = (d0[0] * dp[:, 2] - dp[:, 0] * d0[2]) / den
    src = np.where((u >= 0) & (w >= 0) & (u + w <= 1), floor[0], floor[1])
    tg = emit[rng.randint(0, len(emit), N)].astype(np.int32)
    O, D = rays(O, on_tri(v, tg, rng), scale)
    return O, D, tg, src, cube


def test_rays_occluded_by_the_cube(scene0):
    """Sources on the floor under and around the cube, targets the light: the
    cube occludes a healthy share, so the box tests and the pair loop run."""
    O, D, tg, src, cube = floor_rays(scene0, np.random.RandomState(53))
    vis, i_f = check(scene0, O, D, tg, src, 0.05, 0.98)
    by_cube = np.isin(i_f, cube).mean()
    assert 0.05 < by_cube < 0.98, by_cube


@pytest.mark.parametrize("scale", [0.5, 3.0])
def test_directions_of_other_lengths(scene0, scale):
    """The probes take directions of any length; the pair route must not assume
    unit length (t scales, visibility does not)."""
    rng = np.random.RandomState(59)
    O, D, tg, src, _ = floor_rays(scene0, rng, scale)
    v = verts(scene0)
    k = N // 2  # the other half: from every triangle
    s2 = rng.randint(0, scene0.nT, k)
    O[:k], D[:k] = rays(on_tri(v, s2, rng), on_tri(v, tg[:k], rng), scale)
    src[:k] = s2
    check(scene0, O, D, tg, src, 0.05, 0.98)
