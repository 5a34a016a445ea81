"""The scene batch of the material adjoint: Kd, Ks, Ke over S material sets per
launch (run with -m gpu).

ipt_render_mat_batch_dev / ipt_adjoint_mat_batch_dev trace S sets over one
geometry in one launch; set b must be the single-set launch
(ipt_render_mat_dev / ipt_adjoint_mat_dev) of its arrays and of seed
+ b * seed_stride: images bit for bit, gradients to fp64 summation order
(rtol 1e-10, the tolerance test_gpu_materials.py uses for "same floats,
different fp64 order"), exact zeros staying exact zeros.  One set is also
checked against the CPU oracle, independently of the product's single-set path.
The shapes are the smallest that reach every new address computation: S = 3
(the resident grid does not divide evenly), both brute-force instances, the
BVH instance with more triangles than LDS bins, a row band, S = 1.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, CORNELL_MTL, CUBE_OBJ, SCENE0, SPHERE_OBJ, product_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PHONG_OBJ = os.path.join(ASSETS, "phong", "cube_phong.obj")
PHONG_MTL = os.path.join(ASSETS, "phong", "cube_phong.mtl")
CUBE_KD = (0.9041462985304743, 0.5854651848798454, 0.007022117649276849)

# Calibration (CPU oracle alone, scene B of test_gpu_materials.py, 32x32x8, mb 3, seed 11): the analogous
# identity on the oracle's own Kd adjoint -- the derivative of F = sum(adj * I) along t -> t * Kd_A at t = 1
# (five-point stencil, h = 0.125, exact for mb <= 3) against sum(Kd_A * gKd_A), per object A -- is off by at
# most 6.78e-8 of |F| (3.9e-4 absolute at F = 5812.9).  The bar is 8x that.
REL_KE = 8 * 6.78e-8


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def g9(v):
    return " ".join("%.9g" % float(x) for x in v)


def cornell_mtl(tmp, ke, name="cornell.mtl"):
    """The Cornell box's MTL with the light's Ke replaced."""
    text = open(CORNELL_MTL).read()
    assert "Ke 10 10 10" in text
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        f.write(text.replace("Ke 10 10 10", "Ke " + g9(ke)))
    return path


def phong_mtl(tmp, ks, name="phong.mtl"):
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        f.write("newmtl phong\nKd %s\nKs %s\nNs 20\n" % (g9(np.float32(CUBE_KD)), g9(ks)))
    return path


def scene_a(cornell=CORNELL_MTL, phong=PHONG_MTL):
    """Scene A: Cornell + the Phong cube (Ks 0.5, Ns 20), rotated: 30 triangles, 2 emitters."""
    return [((0, 0, 4), (0, 0, 0), (2, 2, 2), CORNELL[0][3], cornell),
            ((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1), PHONG_OBJ, phong)]


def glow_cube(tmp, ke, name):
    """A small emissive cube: (obj, mtl) with Ke in a temporary MTL."""
    mtl = os.path.join(str(tmp), name + ".mtl")
    with open(mtl, "w") as f:
        f.write("newmtl glow\nKd 0.4 0.4 0.4\nKe %s\n" % g9(ke))
    obj = os.path.join(str(tmp), name + ".obj")
    src = open(CUBE_OBJ).read()
    i = src.index("\nf ") + 1
    with open(obj, "w") as f:
        f.write(src[:i] + "mtllib %s.mtl\nusemtl glow\n" % name + src[i:])
    return obj, mtl


def scene_d(tmp, light_ke=(10, 10, 10), glow_ke=(3, 2, 1), tag="d"):
    """The diffuse many-emitter scene: scenes/0.txt (Cornell + a plain cube, no lobe anywhere) plus the
    emissive cube of test_gpu_materials.py's scene B: 14 emitters."""
    obj, mtl = glow_cube(tmp, glow_ke, "glow_" + tag)
    return [(CORNELL[0][0], CORNELL[0][1], CORNELL[0][2], CORNELL[0][3],
             cornell_mtl(tmp, light_ke, "cornell_%s.mtl" % tag)), SCENE0[1],
            ((1.0, 0.5, 4.5), (0, 0.5, 0), (0.3, 0.3, 0.3), obj, mtl)]


def oracle_hdr(oracle, Q, W, H, spp, mb, seed):
    s, _ = Q.render_samples(W, H, spp, mb, seed)
    return oracle.pixel_mean(s, W * H, spp)[0].reshape(H, W, 3)


def dot64(adj, hdr):
    return float((adj.astype(np.float64) * hdr.astype(np.float64)).sum())


def pos_adj(S, W, H, seed=7):
    """A different positive adjoint image per set."""
    return np.random.RandomState(seed).uniform(0.5, 1.5, (S, H, W, 3)).astype(np.float32)


def _dev(v):
    return None if v is None else torch.tensor(np.ascontiguousarray(v, np.float32), device="cuda")


def _ptrs(ts):
    return [None if t is None else t.data_ptr() for t in ts]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def render_single(P, kd, ks, ke, p):
    from inverse_path_tracer_amd import _native as N

    t = [_dev(v) for v in (kd, ks, ke)]
    hdr = torch.empty((p.rows, p.width, 3), device="cuda", dtype=torch.float32)
    N.check(N.lib().ipt_render_mat_dev(P.handle, C.byref(p), *_ptrs(t), hdr.data_ptr(), None, _stream()),
            "render_mat")
    return hdr.cpu().numpy()


def adjoint_single(P, kd, ks, ke, adj, p):
    from inverse_path_tracer_amd import _native as N

    t = [_dev(v) for v in (kd, ks, ke)]
    a = _dev(adj)
    g = torch.zeros((3, P.nT, 3), device="cuda", dtype=torch.float64)
    N.check(N.lib().ipt_adjoint_mat_dev(P.handle, C.byref(p), *_ptrs(t), a.data_ptr(), g.data_ptr(), _stream()),
            "adjoint_mat")
    return g.cpu().numpy()


def render_batch(P, kd, ks, ke, p, S, stride):
    from inverse_path_tracer_amd import _native as N

    t = [_dev(v) for v in (kd, ks, ke)]
    hdr = torch.empty((S, p.rows, p.width, 3), device="cuda", dtype=torch.float32)
    N.check(N.lib().ipt_render_mat_batch_dev(P.handle, C.byref(p), S, stride, *_ptrs(t), hdr.data_ptr(), _stream()),
            "render_mat_batch")
    return hdr.cpu().numpy()


def adjoint_batch(P, kd, ks, ke, adj, p, S, stride):
    from inverse_path_tracer_amd import _native as N

    t = [_dev(v) for v in (kd, ks, ke)]
    a = _dev(adj)
    g = torch.zeros((S, 3, P.nT, 3), device="cuda", dtype=torch.float64)
    N.check(N.lib().ipt_adjoint_mat_batch_dev(P.handle, C.byref(p), S, stride, *_ptrs(t), a.data_ptr(), g.data_ptr(),
                                              _stream()), "adjoint_mat_batch")
    return g.cpu().numpy()


def same_sums(got, want):
    """Same floats in another fp64 order; an exact 0 stays an exact 0."""
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    assert np.array_equal(got == 0, want == 0)


def draw_sets(P, S, seed, flat_set=None):
    """Per-set kd, ks, ke (S, nT, 3) from a fixed RandomState: Kd in [0.1, 0.9], Ks in [0.1, 0.9] on lobe rows,
    Ke in [5, 15] on emitter rows, 0 elsewhere.  Set `flat_set` gets ONE Ks colour for its lobe rows and ONE Ke
    colour for its emitter rows, so that MTL files can describe it to the oracle."""
    rs = np.random.RandomState(seed)
    nT = P.nT
    kd = rs.uniform(0.1, 0.9, (S, nT, 3)).astype(np.float32)
    ks = rs.uniform(0.1, 0.9, (S, nT, 3)).astype(np.float32) * P.lobe_mask[None, :, None]
    ke = rs.uniform(5, 15, (S, nT, 3)).astype(np.float32) * P.emitter_mask[None, :, None]
    if flat_set is not None:
        ks[flat_set, P.lobe_mask] = rs.uniform(0.1, 0.9, 3).astype(np.float32)
        ke[flat_set, P.emitter_mask] = rs.uniform(5, 15, 3).astype(np.float32)
    return kd, ks.astype(np.float32), ke.astype(np.float32)


def check_batch_equals_singles(P, kd, ks, ke, adj, p, S, stride, gb=None, hb=None):
    """Set b of the batched launches against the single-set launches of its arrays and seed."""
    from inverse_path_tracer_amd import _native as N

    if hb is None:
        hb = render_batch(P, kd, ks, ke, p, S, stride)
    if gb is None:
        gb = adjoint_batch(P, kd, ks, ke, adj, p, S, stride)
    for b in range(S):
        pb = N.make_params(p.width, p.height, p.spp, p.max_bounces, p.seed + b * stride, p.row_begin, p.row_end,
                           p.row_step)
        one = [None if v is None else v[b] for v in (kd, ks, ke)]
        assert np.array_equal(bits(hb[b]), bits(render_single(P, *one, pb))), b
        same_sums(gb[b], adjoint_single(P, *one, adj[b], pb))
    return hb, gb


# ------------------------------------------------------------- scene A: the SPEC brute-force instance
A_SHAPE = (32, 32, 8, 3, 21)  # W, H, spp, mb, seed
A_SETS = 3
FLAT = 1                      # the set the oracle also renders


@pytest.fixture(scope="module")
def A():
    """Scene A, its three material sets and adjoint images, and ONE batched forward + adjoint of them, shared
    (unchanged) by the tests below."""
    from inverse_path_tracer_amd import _native as N

    P = product_scene(scene_a())
    assert P.nT == 30 and P.nE == 2 and P.lobe_mask.sum() == 12
    W, H, spp, mb, seed = A_SHAPE
    kd, ks, ke = draw_sets(P, A_SETS, 31, flat_set=FLAT)
    adj = pos_adj(A_SETS, W, H)
    p = N.make_params(W, H, spp, mb, seed)
    stride = W * H * spp
    hb = render_batch(P, kd, ks, ke, p, A_SETS, stride)
    gb = adjoint_batch(P, kd, ks, ke, adj, p, A_SETS, stride)
    yield dict(P=P, kd=kd, ks=ks, ke=ke, adj=adj, p=p, stride=stride, hb=hb, gb=gb)
    P.close()


def test_batch_equals_single_launches_spec(A, oracle, tmp_path):
    P, W, H, spp, mb, seed = (A["P"],) + A_SHAPE
    # junk outside the masks must be forced to 0 by the pack kernel, in every set
    ks_j, ke_j = A["ks"].copy(), A["ke"].copy()
    ks_j[:, ~P.lobe_mask] = 0.77
    ke_j[:, ~P.emitter_mask] = 5.0
    hb = render_batch(P, A["kd"], ks_j, ke_j, A["p"], A_SETS, A["stride"])
    assert np.array_equal(bits(hb), bits(A["hb"]))
    check_batch_equals_singles(P, A["kd"], A["ks"], A["ke"], A["adj"], A["p"], A_SETS, A["stride"], A["gb"], A["hb"])
    for blk in A["gb"].reshape(-1, P.nT, 3):
        assert np.any(blk != 0)
    assert np.all(A["gb"][:, 1][:, ~P.lobe_mask] == 0) and np.all(A["gb"][:, 2][:, ~P.emitter_mask] == 0)
    # independently of the product's single-set path: set FLAT against the CPU oracle, built from MTL files
    # carrying that set's cube Ks and light Ke, with the set's Kd and seed
    b = FLAT
    Q = oracle.OracleScene(scene_a(cornell_mtl(tmp_path, A["ke"][b][P.emitter_mask][0]),
                                   phong_mtl(tmp_path, A["ks"][b][P.lobe_mask][0])))
    Q.set_materials(A["kd"][b])
    sb = seed + b * A["stride"]
    assert np.array_equal(bits(A["hb"][b]), bits(oracle_hdr(oracle, Q, W, H, spp, mb, sb)))
    np.testing.assert_allclose(A["gb"][b, 0], Q.adjoint(W, H, spp, mb, sb, A["adj"][b]), rtol=1e-9, atol=1e-12)


def test_set_isolation(A):
    """A set whose adjoint image is 0 gets an all-zero slice, and its neighbours' slices do not move: a wrong
    set stride (3 nT instead of 9 nT) would still sum to the right total."""
    P = A["P"]
    adj = A["adj"].copy()
    adj[1] = 0
    g = adjoint_batch(P, A["kd"], A["ks"], A["ke"], adj, A["p"], A_SETS, A["stride"])
    assert g.shape == (A_SETS, 3, P.nT, 3)
    assert np.all(g[1] == 0)
    for b in (0, 2):
        same_sums(g[b], A["gb"][b])


def test_row_bands(A):
    from inverse_path_tracer_amd import _native as N

    P, W, H, spp, mb, seed = (A["P"],) + A_SHAPE
    S = 2
    band = N.make_params(W, H, spp, mb, seed, 1, H, 3)
    kd, ks, ke, adj = (A[k][:S] for k in ("kd", "ks", "ke", "adj"))
    hb = render_batch(P, kd, ks, ke, band, S, A["stride"])
    assert hb.shape == (S, len(range(1, H, 3)), W, 3)
    assert np.array_equal(bits(hb), bits(A["hb"][:S, 1::3]))
    gb = adjoint_batch(P, kd, ks, ke, adj, band, S, A["stride"])
    for b in range(S):
        pb = N.make_params(W, H, spp, mb, seed + b * A["stride"], 1, H, 3)
        same_sums(gb[b], adjoint_single(P, kd[b], ks[b], ke[b], adj[b], pb))
        assert np.any(gb[b] != 0) and not np.allclose(gb[b], A["gb"][b], rtol=1e-3)  # a band, not the frame


def test_one_set_is_the_single_launch(A):
    P = A["P"]
    kd, ks, ke, adj = (A[k][2:3] for k in ("kd", "ks", "ke", "adj"))
    # a stride is irrelevant with one set; NULL arrays are the scene's own values
    check_batch_equals_singles(P, kd, ks, ke, adj, A["p"], 1, 12345)
    check_batch_equals_singles(P, None, None, None, adj, A["p"], 1, 0)


# ------------------------------------------------------------- the diffuse instance, many emitters
def test_diffuse_instance_many_emitters(oracle, tmp_path):
    from inverse_path_tracer_amd import _native as N

    W, H, spp, mb, seed, S = 24, 24, 4, 2, 17, 2
    P = product_scene(scene_d(tmp_path))
    assert P.nE == 14 and not P.lobe_mask.any()
    light = np.zeros(P.nT, bool)
    light[:18] = P.emitter_mask[:18]
    glow = P.emitter_mask & ~light
    assert light.sum() == 2 and glow.sum() == 12
    # ke only (kd_dev = ks_dev = NULL): one colour per emitter object and set, which MTL files can carry
    rs = np.random.RandomState(41)
    cols = rs.uniform(5, 15, (S, 2, 3)).astype(np.float32)
    ke = np.zeros((S, P.nT, 3), np.float32)
    for b in range(S):
        ke[b, light], ke[b, glow] = cols[b, 0], cols[b, 1]
    adj = pos_adj(S, W, H, 8)
    p = N.make_params(W, H, spp, mb, seed)
    stride = W * H * spp
    hb, gb = check_batch_equals_singles(P, None, None, ke, adj, p, S, stride)
    assert np.all(gb[:, 1] == 0)                                  # no lobe: the Ks block is exactly 0 in every set
    assert np.all(gb[:, 2][:, ~P.emitter_mask] == 0) and np.all(gb[:, 2][:, P.emitter_mask] != 0)
    # per set: sum Ke * gKe = sum adj * I (radiance is linear and homogeneous in Ke) against the oracle's forward
    for b in range(S):
        Q = oracle.OracleScene(scene_d(tmp_path, cols[b, 0], cols[b, 1], tag="s%d" % b))
        hdr = oracle_hdr(oracle, Q, W, H, spp, mb, seed + b * stride)
        assert np.array_equal(bits(hb[b]), bits(hdr))
        for c in range(3):
            want = dot64(adj[b, :, :, c], hdr[:, :, c])
            got = float((ke[b, :, c].astype(np.float64) * gb[b, 2, :, c]).sum())
            print("set %d channel %d: sum Ke gKe %.9g vs sum adj I %.9g (%.2e of the bar)" %
                  (b, c, got, want, abs(got - want) / (REL_KE * abs(want))))
            assert abs(got - want) <= REL_KE * abs(want), (b, c)
    P.close()


# ------------------------------------------------------------- BVH + SPEC, the hot-set bin map
def test_bvh_spec_instance_and_hot_set(tmp_path):
    """The Phong-sphere scene of test_gpu_materials.py: more triangles than LDS bins, so the bins of triangles
    outside the hot set go straight to global atomics, which must land inside the set's slice."""
    from inverse_path_tracer_amd import _native as N

    mtl = tmp_path / "shiny.mtl"
    mtl.write_text("newmtl shiny\nKd 0.2 0.6 0.3\nKs 0.4 0.4 0.4\nNs 30\n")
    src = open(SPHERE_OBJ).read()
    i = src.index("\nf ") + 1
    obj = tmp_path / "sphere_shiny.obj"
    obj.write_text(src[:i] + "mtllib shiny.mtl\nusemtl shiny\n" + src[i:])
    P = product_scene(SCENE0 + [((-1.2, -1.35, 4.6), (0, 0, 0), (1.2, 1.2, 1.2), str(obj), str(mtl))])
    assert P.nT > 1000 and P.bvh_info()["accel"] == "bvh" and P.lobe_mask.sum() == 1280
    W, H, spp, mb, seed, S = 24, 24, 4, 3, 12, 2
    kd, ks, ke = draw_sets(P, S, 43)
    adj = pos_adj(S, W, H, 9)
    p = N.make_params(W, H, spp, mb, seed)
    _, gb = check_batch_equals_singles(P, kd, ks, ke, adj, p, S, W * H * spp)
    for blk in gb.reshape(-1, P.nT, 3):
        assert np.any(blk != 0)
    assert np.count_nonzero(gb[:, 1][:, P.lobe_mask]) > 100
    P.close()


# ------------------------------------------------------------- the torch op
def test_torch_op(A):
    from inverse_path_tracer_amd import torch_ops

    P = A["P"]
    W, H, spp, mb, seed, S = 40, 24, 8, 4, 6, 3
    kd, ks, ke = (torch.tensor(A[k], device="cuda", requires_grad=True) for k in ("kd", "ks", "ke"))
    img = torch_ops.render_materials_batch(P, kd, ks, ke, W, H, spp, mb, seed)
    assert img.shape == (S, H, W, 3)
    frame = W * H * spp                               # the default stride: one frame
    with torch.no_grad():
        want_img = torch.stack([torch_ops.render_materials(P, kd[b], ks[b], ke[b], W, H, spp, mb, seed + b * frame)
                                for b in range(S)])
    assert torch.equal(img.detach(), want_img)
    adj = torch.tensor(pos_adj(S, W, H, 3), device="cuda")
    (img * adj).sum().backward()
    want = P.adjoint_materials_batch(adj.cpu().numpy(), A["kd"], A["ks"], A["ke"], W, H, spp, mb, seed)
    assert want.shape == (S, 3, P.nT, 3) and want.dtype == np.float64
    for i, t in enumerate((kd, ks, ke)):
        assert t.grad is not None and t.grad.dtype == torch.float32 and t.grad.shape == (S, P.nT, 3)
        np.testing.assert_allclose(t.grad.cpu().numpy(), want[:, i], rtol=1e-6, atol=1e-30)
    # a None input (the scene's own Kd in every set) and a no-grad input
    ks2 = torch.tensor(A["ks"], device="cuda", requires_grad=True)
    img2 = torch_ops.render_materials_batch(P, None, ks2, ke.detach(), W, H, spp, mb, seed, seed_stride=frame)
    with torch.no_grad():
        want2 = torch.stack([torch_ops.render_materials(P, None, ks2[b], ke[b], W, H, spp, mb, seed + b * frame)
                             for b in range(S)])
    assert torch.equal(img2.detach(), want2)
    (img2 * adj).sum().backward()
    g2 = P.adjoint_materials_batch(adj.cpu().numpy(), None, A["ks"], A["ke"], W, H, spp, mb, seed)
    np.testing.assert_allclose(ks2.grad.cpu().numpy(), g2[:, 1], rtol=1e-6, atol=1e-30)
    with pytest.raises(ValueError):
        torch_ops.render_materials_batch(P, kd, ks[:2], ke, W, H, spp, mb, seed)
    with pytest.raises(ValueError):
        torch_ops.render_materials_batch(P, None, None, None, W, H, spp, mb, seed)
    with pytest.raises(ValueError):
        torch_ops.render_materials_batch(P, kd[0], None, None, W, H, spp, mb, seed)


def test_torch_op_adjoint_seed():
    """The backward on a stream of its own, one input None and one without a gradient: the op's gradient is
    the host method's at that seed (two launches of one adjoint: test_torch_op's bound)."""
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.scene import Scene

    P = Scene.from_file(os.path.join(ASSETS, "phong", "scene0_phong.txt"))
    W, H, spp, mb, seed, aseed, S = 8, 8, 4, 2, 6, 12345, 2
    _, ks0, ke0, _ = P.material_params()
    ks0 = np.stack([ks0, 0.5 * ks0])
    ke0 = np.stack([ke0, 2 * ke0])
    ks = torch.tensor(ks0, device="cuda", requires_grad=True)
    img = torch_ops.render_materials_batch(P, None, ks, torch.tensor(ke0, device="cuda"), W, H, spp, mb, seed,
                                           adjoint_seed=aseed)
    adj = pos_adj(S, W, H, 3)
    (img * torch.tensor(adj, device="cuda")).sum().backward()
    want = P.adjoint_materials_batch(adj, None, ks0, ke0, W, H, spp, mb, aseed)
    assert np.any(want[0, 1] != 0) and np.any(want[1, 1] != 0)
    np.testing.assert_allclose(ks.grad.cpu().numpy(), want[:, 1], rtol=1e-6, atol=1e-30)
    assert not np.allclose(ks.grad.cpu().numpy(), P.adjoint_materials_batch(adj, None, ks0, ke0, W, H, spp, mb,
                                                                             seed)[:, 1], rtol=1e-6, atol=1e-30)
    P.close()


# ------------------------------------------------------------- refusals
def test_refusals_leave_the_stream_usable(A):
    from inverse_path_tracer_amd import NativeError, torch_ops
    from inverse_path_tracer_amd import _native as N

    P, W, H, spp, mb, seed = (A["P"],) + A_SHAPE
    kd = torch.tensor(A["kd"], device="cuda")
    with pytest.raises(NativeError, match="unbounded estimator"):
        torch_ops.render_materials_batch(P, kd, None, None, W, H, spp, None, seed)
    with pytest.raises(NativeError, match="0..62"):
        torch_ops.render_materials_batch(P, kd, None, None, W, H, spp, 63, seed)
    for bad in (None, 63):
        with pytest.raises(NativeError, match="max_bounces"):
            P.adjoint_materials_batch(A["adj"], A["kd"], A["ks"], A["ke"], W, H, spp, bad, seed)
    zero = N.make_params(W, H, spp, mb, seed)
    g = torch.zeros((3, P.nT, 3), device="cuda", dtype=torch.float64)
    a = torch.tensor(A["adj"][0], device="cuda")
    N.lib().ipt_clear_error()
    assert N.lib().ipt_adjoint_mat_batch_dev(P.handle, C.byref(zero), 0, 0, None, None, None, a.data_ptr(),
                                             g.data_ptr(), _stream()) == -1 and "n_scenes" in N.last_error()
    assert float(g.abs().sum()) == 0
    # later batched launches on the same stream reproduce the earlier results
    assert np.array_equal(bits(render_batch(P, A["kd"], A["ks"], A["ke"], A["p"], A_SETS, A["stride"])), bits(A["hb"]))
    same_sums(adjoint_batch(P, A["kd"], A["ks"], A["ke"], A["adj"], A["p"], A_SETS, A["stride"]), A["gb"])


# ------------------------------------------------------------- the optimizer
def _variant_files(tmp, ks_true, ke_true):
    """Scene files of scene A variants: one geometry, the cube's Ks and the light's Ke from temporary MTLs."""
    from inverse_path_tracer_amd.scene import format_object_block

    files = []
    for i, (ks, ke) in enumerate(zip(ks_true, ke_true)):
        recs = scene_a(cornell_mtl(tmp, ke, "cornell_v%d.mtl" % i), phong_mtl(tmp, ks, "phong_v%d.mtl" % i))
        path = os.path.join(str(tmp), "variant_%d.txt" % i)
        with open(path, "w") as f:
            for pos, ori, scl, obj, mtl in recs:
                f.write("OBJECT\n" + format_object_block(obj, mtl, pos, ori, scl))
        files.append(path)
    return files


def test_optimizer_learns_ks_and_ke_through_the_batch(tmp_path, monkeypatch):
    from inverse_path_tracer_amd import _native as N
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    W = H = 64
    spp, mb, steps = 16, 3, 200
    ks_true = [(0.2, 0.8, 0.3), (0.8, 0.25, 0.7), (0.15, 0.2, 0.85), (0.85, 0.8, 0.2)]
    ke_true = [(6.0, 14.0, 7.0), (14.0, 6.5, 13.0), (5.5, 7.0, 14.5), (15.0, 13.0, 6.0)]
    dev = torch.device("cuda")
    tasks = build_tasks(_variant_files(tmp_path, ks_true, ke_true), W, H, 256, mb, 0.5, dev, learn=("ks", "ke"),
                        init_ks=0.5, init_ke=10.0)
    sc = tasks[0].scene
    assert all(t.scene is sc for t in tasks), "the variants differ only in Ks / Ke values: one geometry handle"
    lobe, emit = torch.tensor(sc.lobe_mask, device=dev), torch.tensor(sc.emitter_mask, device=dev)
    for t, ks, ke in zip(tasks, ks_true, ke_true):
        assert torch.equal(t.kd, t.truth) and not t.kd.requires_grad           # Kd is held at the truth
        assert torch.equal(t.truth_ks[lobe], torch.tensor(ks, device=dev).expand(12, 3))
        assert torch.equal(t.truth_ke[emit], torch.tensor(ke, device=dev).expand(2, 3))
    # observable Ks rows (optimize.observable_mask's rule): lobe rows whose initial |dL/dKs| exceeds 0.25 of
    # the largest -- the cube's back and bottom faces never reach the camera
    obs = []
    for t in tasks:
        ks = t.ks.detach().clone().requires_grad_(True)
        img = torch_ops.render_materials(sc, t.kd, ks, t.ke.detach(), W, H, 64, mb, seed=5)
        ((img - t.target) ** 2).mean().backward()
        g = ks.grad.abs().sum(1)
        obs.append(lobe & (g > 0.25 * float(g.max())))
        assert 2 <= int(obs[-1].sum()) <= 12

    def errors():
        return [(float((t.ks.detach() - t.truth_ks)[m].abs().mean()),
                 float((t.ke.detach() - t.truth_ke)[emit].abs().mean())) for t, m in zip(tasks, obs)]

    calls = {}
    for name in ("ipt_render_mat_batch_dev", "ipt_adjoint_mat_batch_dev", "ipt_render_mat_dev", "ipt_adjoint_mat_dev",
                 "ipt_render_batch_dev", "ipt_adjoint_batch_dev"):
        def wrap(*a, _f=getattr(N.lib(), name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        monkeypatch.setattr(N.lib(), name, wrap)
    opt = MaterialOptimizer(tasks, W, H, spp, mb, lr={"ks": 0.02, "ke": 0.2}, learn=("ks", "ke"))
    e0 = errors()
    opt.run(steps)
    e1 = errors()
    monkeypatch.undo()
    # every step is ONE batched forward and ONE batched material adjoint for the four scenes
    assert calls == {"ipt_render_mat_batch_dev": steps, "ipt_adjoint_mat_batch_dev": steps}, calls
    for i, (a, b) in enumerate(zip(e0, e1)):
        print("scene %d (%d observable Ks rows): Ks error %.4f -> %.4f, Ke error %.4f -> %.4f" %
              (i, int(obs[i].sum()), a[0], b[0], a[1], b[1]))
    for t in tasks:
        assert len(t.history) == steps and t.history[-1] < t.history[0]
        assert torch.all(t.ks.detach()[~lobe] == 0) and torch.all(t.ke.detach()[~emit] == 0)  # frozen rows stay 0
        ks, ke = t.ks.detach(), t.ke.detach()
        assert float(ks.min()) >= 0 and float(ks.max()) <= 1 and float(ke.min()) >= 0
    for a, b in zip(e0, e1):
        assert b[0] <= 0.5 * a[0] and b[1] <= 0.5 * a[1]


def test_optimizer_default_learn_is_the_kd_optimizer():
    """learn=("kd",) over three steps against the Kd-only optimiser written out by hand: render_batch, Adam,
    frames 2 t n + i for the forward and n frames later for the adjoint."""
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    root = os.path.join(os.path.dirname(ASSETS), "assets", "scenes")
    files = [os.path.join(root, "%d.txt" % i) for i in range(3)]
    W, H, spp, mb, n = 32, 32, 8, 3, 3
    dev = torch.device("cuda")
    histories = []
    for kw in ({}, {"learn": ("kd",)}):
        tasks = build_tasks(files, W, H, 32, mb, 0.5, dev, **kw)
        MaterialOptimizer(tasks, W, H, spp, mb, lr=1e-2, **kw).run(3)
        histories.append([t.history for t in tasks])
    assert histories[0] == histories[1]
    tasks = build_tasks(files, W, H, 32, mb, 0.5, dev)
    kd = torch.stack([t.kd.detach() for t in tasks]).clone().requires_grad_(True)
    target = torch.stack([t.target for t in tasks])
    adam = torch.optim.Adam([kd], lr=1e-2)
    frame, want = W * H * spp, []
    for step in range(3):
        adam.zero_grad(set_to_none=False)
        base = 2 * step * n * frame
        img = torch_ops.render_batch(tasks[0].scene, kd, W, H, spp, mb, seed=base, seed_stride=frame,
                                     adjoint_seed=base + n * frame)
        per = ((img - target) ** 2).mean(dim=(1, 2, 3))
        per.sum().backward()
        adam.step()
        with torch.no_grad():
            kd.clamp_(0.0, 1.0)
        want.append(per.detach().float().cpu().tolist())
    assert histories[1] == [[want[s][i] for s in range(3)] for i in range(n)]
