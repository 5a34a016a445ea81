"""Caller-supplied cameras: render and material adjoint over V views in one
launch (run with -m gpu).

ipt_render_views_dev / ipt_adjoint_views_dev trace V cameras over ONE
material set: view b must be the single-camera launch of camera b at seed
+ b * seed_stride (images bit for bit), the gradient the sum of the single-view
gradients (fp64 summation order, rtol 1e-10).  Through the scene's own camera
the launch is ipt_render_mat_dev's, hence the CPU oracle's.  The camera itself
is pinned twice without a reference counterpart: its rays bit for bit against a
restatement written here, and a translated camera statistically against the
oracle rendering the oppositely translated scene.
Shapes: scene A (SPEC brute force), Cornell (diffuse brute force), the north
star (BVH); W = 30 takes camera_local's dividing path, 32 its multiply path.
"""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, NORTHSTAR, SCENE0, product_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PHONG_OBJ = os.path.join(ASSETS, "phong", "cube_phong.obj")
PHONG_MTL = os.path.join(ASSETS, "phong", "cube_phong.mtl")
SCENE_A = CORNELL + [((0, -1.5, 4), (0, 0, 0), (1, 1, 1), PHONG_OBJ, PHONG_MTL)]  # assets/phong/scene0_phong.txt
RECORDS = {"A": SCENE_A, "cornell": CORNELL, "northstar": NORTHSTAR}
FRAME = {"A": (30, 24, 8), "cornell": (30, 24, 8), "northstar": (32, 24, 4)}
MB = 3
TAU = (0.5, 0.25, 0.75)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = product_scene(RECORDS[name])
    return _scenes[name]


_oracles = {}


def oracle_scene(oracle, name):
    if name not in _oracles:
        _oracles[name] = oracle.OracleScene(RECORDS[name])
    return _oracles[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cameras(P):
    """Own; translated by TAU; look_at from the side -- rotated, 60 degrees -- and moved."""
    from inverse_path_tracer_amd.scene import camera_at, camera_look_at

    own = P.camera()
    side = camera_at(camera_look_at((0, 0, 0), (0.5, -0.2, 1.0), (0, 1, 0), fov_deg=60), (-0.8, 0.3, 0.5))
    return np.stack([own, camera_at(own, TAU), side])


def pos_adj(V, W, H, seed=7):
    return np.random.RandomState(seed).uniform(0.5, 1.5, (V, H, W, 3)).astype(np.float32)


def render_mat_dev(P, W, H, spp, seed, band=(0, None, 1)):
    from inverse_path_tracer_amd import _native as N

    p = N.make_params(W, H, spp, MB, seed, *band)
    hdr = torch.empty((p.rows, W, 3), device="cuda", dtype=torch.float32)
    N.check(N.lib().ipt_render_mat_dev(P.handle, C.byref(p), None, None, None, hdr.data_ptr(), None,
                                       torch.cuda.current_stream().cuda_stream), "render_mat")
    return hdr.cpu().numpy()


# ------------------------------------------------------------------ 1. the scene's own camera
OWN_CASES = [("A", FRAME["A"], (0, None, 1)), ("cornell", FRAME["cornell"], (0, None, 1)),
             ("northstar", FRAME["northstar"], (0, None, 1)), ("A", (32, 32, 8), (0, None, 1)),
             ("A", FRAME["A"], (3, 21, 2))]


@pytest.mark.parametrize("name,frame,band", OWN_CASES, ids=["A", "cornell", "northstar", "A-32x32", "A-band"])
def test_own_camera_is_the_single_camera_launch_and_the_oracle(oracle, name, frame, band):
    P, Q = scene(name), oracle_scene(oracle, name)
    W, H, spp = frame
    seed = 2024
    rb, re_, rs = band
    v = P.views(P.camera()[None])
    img = P.render_views(v, W, H, spp, MB, seed, row_begin=rb, row_end=re_, row_step=rs)
    assert img.shape[0] == 1
    assert np.array_equal(bits(img[0]), bits(render_mat_dev(P, W, H, spp, seed, band)))
    want = Q.render(W, H, spp, MB, seed)[0][rb:re_:rs]
    assert np.array_equal(bits(img[0]), bits(want))
    # the host form is the same launch
    from inverse_path_tracer_amd import _native as N

    p = N.make_params(W, H, spp, MB, seed, rb, re_, rs)
    host = np.zeros_like(img)
    N.check(N.lib().ipt_render_views_host(P.handle, v.handle, C.byref(p), W * H * spp, host.ctypes.data_as(N.fp)))
    assert np.array_equal(bits(host), bits(img))

    adj = np.random.RandomState(3).uniform(-1, 1, (1, H, W, 3)).astype(np.float32)
    g = P.adjoint_views(v, adj, W, H, spp, MB, seed, row_begin=rb, row_end=re_, row_step=rs)
    ref = Q.adjoint_materials(W, H, spp, MB, seed, adj[0], rb, H if re_ is None else re_, rs)
    for blk, (got, exp) in enumerate(zip(g, ref)):
        print(name, "block", blk, "max|d|", np.abs(got - exp).max(), "max|g|", np.abs(exp).max())
        assert np.allclose(got, exp, rtol=1e-9, atol=1e-12), blk
        zero = ~exp.any(axis=1)
        assert not got[zero].any(), blk  # exact-zero rows stay exactly zero
    assert not g[1][~P.lobe_mask].any() and not g[2][~P.emitter_mask].any()
    gh = np.zeros_like(g)
    N.check(N.lib().ipt_adjoint_views_host(P.handle, v.handle, C.byref(p), W * H * spp, adj.ctypes.data_as(N.fp),
                                           gh.ctypes.data_as(N.dp)))
    assert np.allclose(gh, g, rtol=1e-10, atol=0)
    v.close()


# ------------------------------------------------------------------ 2. V views = V single-view launches
def overrides(P, on):
    if not on:
        return {}
    rs = np.random.RandomState(5)
    kd, ks, ke, _ = P.material_params()
    return {"kd": rs.uniform(0.2, 0.8, kd.shape).astype(np.float32),
            "ks": (ks * rs.uniform(0.5, 1.0, ks.shape)).astype(np.float32),
            "ke": (ke * rs.uniform(0.5, 1.5, ke.shape)).astype(np.float32)}


def check_views_equal_singles(P, cams, W, H, spp, seed, stride, mats):
    V = cams.shape[0]
    allv = P.views(cams)
    imgs = P.render_views(allv, W, H, spp, MB, seed, seed_stride=stride, **mats)
    adj = pos_adj(V, W, H)
    g = P.adjoint_views(allv, adj, W, H, spp, MB, seed, seed_stride=stride, **mats)
    total = np.zeros_like(g)
    singles = []
    st = W * H * spp if stride is None else stride
    for b in range(V):
        one = P.views(cams[b:b + 1])
        img = P.render_views(one, W, H, spp, MB, seed + b * st, **mats)
        assert np.array_equal(bits(imgs[b]), bits(img[0])), b
        singles.append(P.adjoint_views(one, adj[b:b + 1], W, H, spp, MB, seed + b * st, **mats))
        total += singles[-1]
        one.close()
    nz = total != 0
    print("V", V, "max rel", (np.abs(g - total)[nz] / np.abs(total)[nz]).max())
    assert np.allclose(g, total, rtol=1e-10, atol=0)
    assert not g[~nz].any()
    return allv, imgs, adj, g, singles


@pytest.mark.parametrize("name,mats", [("A", True), ("A", False), ("cornell", False), ("northstar", False)],
                         ids=["A-overrides", "A-null", "cornell-null", "northstar-null"])
def test_three_cameras_are_three_single_view_launches(name, mats):
    P = scene(name)
    W, H, spp = FRAME[name]
    cams = cameras(P)
    allv, imgs, adj, g, singles = check_views_equal_singles(P, cams, W, H, spp, 77, None, overrides(P, mats))
    # the three cameras see three different images
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[0], imgs[2])
    # 5. linearity in adj per view: an adjoint image that is zero in view 1 gives views 0 and 2 alone
    a0 = adj.copy()
    a0[1] = 0
    g02 = P.adjoint_views(allv, a0, W, H, spp, MB, 77, **overrides(P, mats))
    want = singles[0] + singles[2]
    assert np.allclose(g02, want, rtol=1e-10, atol=0) and not g02[want == 0].any()
    allv.close()


@pytest.mark.parametrize("mats", [True, False], ids=["overrides", "null"])
def test_five_views_do_not_divide_the_grid(mats):
    from inverse_path_tracer_amd.scene import camera_at

    P = scene("cornell")
    W, H, spp = FRAME["cornell"]
    c3 = cameras(P)
    cams = np.stack([c3[0], c3[1], c3[2], camera_at(c3[0], (-0.4, -0.6, 0.2)), camera_at(c3[2], (0.7, 0.1, 1.0))])
    m = overrides(P, mats)
    m.pop("ks", None)  # Cornell has no lobe: ks NULL, kd and ke given
    allv = check_views_equal_singles(P, cams, W, H, spp, 5, 1000, m)[0]  # a stride of its own, overlapping frames
    allv.close()


# ------------------------------------------------------------------ 3. rays, bit for bit
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
F = np.float32


def fmaf(a, b, c):
    return F(_libm.fmaf(float(a), float(b), float(c)))


def dot3(a, b):  # dot products are the fma chain z, y, x
    return fmaf(a[2], b[2], fmaf(a[1], b[1], F(a[0]) * F(b[0])))


def unit(v):  # Eigen normalize: IEEE sqrt and divisions
    n2 = dot3(v, v)
    if n2 > 0:
        s = np.sqrt(F(n2))
        return [F(v[0]) / s, F(v[1]) / s, F(v[2]) / s]
    return [F(x) for x in v]


def restated_ray(oracle, M, g, seed, W, H, spp):
    """path_trace.cu:150-165 + Ray::transform (scene_basics.h:307-319) for global sample g."""
    L = oracle.lib()
    pixel = g // spp
    r, c = pixel // W, pixel % W
    u0, u1 = F(L.oro_uniform_at(seed + g, 0)), F(L.oro_uniform_at(seed + g, 1))
    x = F(2) * (F(c) + u0) / F(W) - F(1)
    y = F(1) - F(2) * (F(r) + u1) / F(H)
    d0 = unit([x, y, F(1)])
    p, v = [], []
    for i in range(3):  # m * (p, 1) and m * (d, 0), each row the fma chain from column 0
        p.append(fmaf(M[i, 3], 1, fmaf(M[i, 2], 0, fmaf(M[i, 1], 0, F(M[i, 0]) * F(0)))))
        v.append(fmaf(M[i, 3], 0, fmaf(M[i, 2], d0[2], fmaf(M[i, 1], d0[1], F(M[i, 0]) * d0[0]))))
    return p, unit(v)


@pytest.mark.parametrize("W,H", [(30, 24), (32, 32)], ids=["divide", "multiply"])
def test_view_rays_bit_for_bit(oracle, W, H):
    P = scene("A")
    spp, seed = 8, 991
    cams = cameras(P)
    v = P.views(cams)
    n = W * H * spp
    idx = np.unique(np.concatenate([[0, spp - 1, n - spp, n - 1],
                                    np.random.RandomState(1).randint(0, n, 1996)])).astype(np.int64)
    old = np.seterr(all="ignore")
    try:
        for b in (0, 1, 2):  # the default camera first: if that disagrees, the restatement is wrong
            org, d = P.view_rays(v, b, W, H, spp, seed, idx)
            want = [restated_ray(oracle, cams[b], int(g), seed, W, H, spp) for g in idx]
            wo = np.array([w[0] for w in want], np.float32)
            wd = np.array([w[1] for w in want], np.float32)
            assert np.array_equal(bits(org), bits(wo)), b
            bad = np.flatnonzero((bits(d) != bits(wd)).any(axis=1))
            assert bad.size == 0, (b, bad[:5], d[bad[:5]], wd[bad[:5]])
    finally:
        np.seterr(**old)
    v.close()


# ------------------------------------------------------------------ 4. a moved camera is a moved scene
def tone_dist(X, Y):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    return float(np.abs(X / (1 + X) - Y / (1 + Y)).mean())


def test_translated_camera_against_the_oracle_of_the_shifted_scene(oracle):
    from inverse_path_tracer_amd.scene import camera_at

    W, H, spp = 48, 36, 256
    shifted = [(tuple(np.float32(p) - np.float32(t) for p, t in zip(r[0], TAU)),) + tuple(r[1:]) for r in SCENE0]
    Q = oracle.OracleScene(shifted)
    # Sample g of a frame draws from generator seed + g, so frames whose seeds lie closer than one frame
    # (W*H*spp = 442 368) share almost all their paths: the three seeds are billions apart.
    O1 = Q.render(W, H, spp, MB, 1_000_003)[0]
    O2 = Q.render(W, H, spp, MB, 2_000_000_011)[0]
    P = product_scene(SCENE0)
    own = P.camera()
    v = P.views(np.stack([camera_at(own, TAU), camera_at(own, tuple(-t for t in TAU))]))
    G = P.render_views(v, W, H, spp, MB, 3_000_000_019)
    noise, d_pos, d_neg = tone_dist(O1, O2), tone_dist(G[0], O1), tone_dist(G[1], O1)
    print("d(O1,O2) = %.6f  d(G,O1) = %.6f  d(G(-tau),O1) = %.6f" % (noise, d_pos, d_neg))
    assert d_pos <= 1.15 * noise
    assert d_neg > 1.15 * noise  # the test sees a camera moved the wrong way
    v.close()
    P.close()


# ------------------------------------------------------------------ 6. the torch op
def test_render_views_op_matches_adjoint_views():
    from inverse_path_tracer_amd import torch_ops

    P = scene("A")
    W, H, spp = FRAME["A"]
    v = P.views(cameras(P))
    kd0, ks0, ke0, _ = P.material_params()
    kd = torch.tensor(kd0, device="cuda", requires_grad=True)
    ks = torch.tensor(ks0, device="cuda", requires_grad=True)
    ke = torch.tensor(ke0, device="cuda")  # given, no gradient wanted
    img = torch_ops.render_views(P, v, kd, ks, ke, W, H, spp, MB, seed=9)
    assert tuple(img.shape) == (3, H, W, 3) and img.dtype == torch.float32
    assert np.array_equal(bits(img.detach().cpu().numpy()),
                          bits(P.render_views(v, W, H, spp, MB, 9, kd=kd0, ks=ks0, ke=ke0)))
    adj = pos_adj(3, W, H, seed=4)
    (img * torch.from_numpy(adj).cuda()).sum().backward()
    g = P.adjoint_views(v, adj, W, H, spp, MB, 9, kd=kd0, ks=ks0, ke=ke0)
    assert kd.grad.dtype == torch.float32 and ks.grad.dtype == torch.float32 and ke.grad is None
    assert np.allclose(kd.grad.cpu().numpy(), g[0].astype(np.float32), rtol=1e-6, atol=0)
    assert np.allclose(ks.grad.cpu().numpy(), g[1].astype(np.float32), rtol=1e-6, atol=0)
    # a decorrelated adjoint stream is another estimate of the same gradient
    kd2 = torch.tensor(kd0, device="cuda", requires_grad=True)
    img2 = torch_ops.render_views(P, v, kd2, None, None, W, H, spp, MB, seed=9, adjoint_seed=12345)
    (img2 * torch.from_numpy(adj).cuda()).sum().backward()
    g2 = P.adjoint_views(v, adj, W, H, spp, MB, 12345)
    assert np.allclose(kd2.grad.cpu().numpy(), g2[0].astype(np.float32), rtol=1e-6, atol=0)
    v.close()


# ------------------------------------------------------------------ 7. recovery
def recover(P, views, spp, truth, cube, steps=200):
    """Plain Adam on the cube's Kd from 0.5 against targets rendered at the truth; the final Kd."""
    from inverse_path_tracer_amd import torch_ops

    W = H = 64
    kd_true = torch.tensor(truth, device="cuda")
    with torch.no_grad():
        target = torch_ops.render_views(P, views, kd_true, None, None, W, H, 4 * spp, MB, seed=1 << 40)  # a stream of its own
    base = kd_true.clone()
    x = torch.full((len(cube), 3), 0.5, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([x], lr=0.02)
    ix = torch.tensor(cube, device="cuda")
    for step in range(steps):
        opt.zero_grad()
        kd = base.index_put((ix,), x)
        img = torch_ops.render_views(P, views, kd, None, None, W, H, spp, MB, seed=1000 + step * 10 * W * H * spp)
        ((img - target) ** 2).mean().backward()
        opt.step()
        with torch.no_grad():
            x.clamp_(0.0, 1.0)
    return x.detach().cpu().numpy()


def test_three_views_recover_the_cube_where_one_cannot():
    from inverse_path_tracer_amd.scene import camera_at, camera_look_at

    P = scene("A")
    truth = P.material_params()[0]
    cube = list(range(P.nT - 12, P.nT))
    tri = P.triangles()
    # the cube's two floor-facing triangles: face normal -y
    floor = [t for t in cube if tri[t, 19] < -0.99]
    assert len(floor) == 2
    seen = [t - cube[0] for t in cube if t not in floor]
    centre = np.array([0, -1.5, 4], np.float32)
    eyes = [np.array([-1.6, -0.4, 5.6], np.float32), np.array([1.6, -0.4, 2.4], np.float32)]
    assert max(np.abs(e).max() for e in eyes) <= P.camera_bound
    cams = [P.camera()] + [camera_at(camera_look_at((0, 0, 0), centre - e, (0, 1, 0)), e) for e in eyes]
    three, one = P.views(np.stack(cams)), P.views(cams[0][None])
    start = float(np.abs(0.5 - truth[cube][seen]).mean())
    err3 = float(np.abs(recover(P, three, 16, truth, cube)[seen] - truth[cube][seen]).mean())
    err1 = float(np.abs(recover(P, one, 48, truth, cube)[seen] - truth[cube][seen]).mean())
    print("recovery: start %.4f  three views %.4f  default view alone %.4f" % (start, err3, err1))
    assert err3 < 0.5 * start
    assert not err1 < 0.5 * start
    three.close()
    one.close()


# ------------------------------------------------------------------ 8. refusals on a device scene
def test_refusals_leave_the_stream_intact():
    from inverse_path_tracer_amd import _native as N

    P = scene("A")
    W, H, spp = FRAME["A"]
    v = P.views(cameras(P))
    adj = pos_adj(3, W, H)
    ref_img = P.render_views(v, W, H, spp, MB, 21)
    ref_g = P.adjoint_views(v, adj, W, H, spp, MB, 21)

    def intact():
        assert np.array_equal(bits(P.render_views(v, W, H, spp, MB, 21)), bits(ref_img))
        assert np.allclose(P.adjoint_views(v, adj, W, H, spp, MB, 21), ref_g, rtol=1e-10, atol=0)

    dead = P.views(P.camera()[None])
    dead.close()
    other = scene("cornell").views(scene("cornell").camera()[None])
    refused = [
        ("null views handle", lambda: P.render_views(dead, W, H, spp, MB, 21)),
        ("null views handle", lambda: P.adjoint_views(dead, adj[:1], W, H, spp, MB, 21)),
        ("0..62", lambda: P.adjoint_views(v, adj, W, H, spp, None, 21)),
        ("0..62", lambda: P.adjoint_views(v, adj, W, H, spp, 63, 21)),
        ("0..62", lambda: P.render_views(v, W, H, spp, 63, 21)),
        ("invalid render parameters", lambda: P.render_views(v, W, H, 0, MB, 21)),
        ("view outside", lambda: P.view_rays(v, 3, W, H, spp, 21, [0])),
        ("sample index", lambda: P.view_rays(v, 0, W, H, spp, 21, [W * H * spp])),
    ]
    for text, call in refused:
        with pytest.raises(N.NativeError, match=text):
            call()
        intact()
    # a handle of another scene, through the C ABI
    p = N.make_params(W, H, spp, MB, 21)
    out = torch.zeros((1, H, W, 3), device="cuda")
    assert N.lib().ipt_render_views_dev(P.handle, other.handle, C.byref(p), 1, None, None, None, out.data_ptr(),
                                        None) == -1
    assert "another scene" in N.last_error()
    intact()
    # a launch that fails after its counters and scratch are taken (the debug hook covers the new launches)
    for call in (lambda: P.render_views(v, W, H, spp, MB, 21), lambda: P.adjoint_views(v, adj, W, H, spp, MB, 21)):
        N.lib().ipt_debug_fail_launches(1)
        with pytest.raises(N.NativeError, match="on request"):
            call()
        N.lib().ipt_debug_fail_launches(0)
        intact()
    other.close()
    v.close()
