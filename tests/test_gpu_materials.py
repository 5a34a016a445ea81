"""Gradients for specular Ks and emission Ke alongside Kd (run with -m gpu).

The material adjoint (trace_mat_kernel) returns
d(sum adj*I)/d(Kd, Ks, Ke) of the bounded estimator under the forward's own
paths.  With the paths fixed a sample's radiance is a polynomial in Kd and Ks
and exactly linear and homogeneous in Ke, so the new blocks are checked here
by identities (tests/test_gpu_materials_oracle.py compares every entry with
the oracle's material adjoint, which these identities pin on the CPU):
  * the forward with overrides is the oracle's, bit for bit;
  * the Kd block is the existing adjoint's (rtol 1e-9 against the oracle);
  * Ke: sum Ke * gKe equals the oracle's forward (homogeneity), per channel
    and per emitter object (doubling Ke is exact in fp32);
  * Ks: a five-point stencil, exact for polynomials of degree <= 4 (mb <= 3);
  * row bands sum to the full gradient, all blocks are linear in adj;
  * the torch op, a recovery run, and the refusals.

Tolerances of the identities are reference-only: measured on the CPU oracle's
own Kd adjoint by tools/matgrad_calibrate.py (CPU only; its figures are
written beside the constants, the bars are 8x them).
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
    """Scene A: Cornell + the Phong cube (Ks 0.5, Ns 20), rotated."""
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


def scene_b(tmp, light_ke=(10, 10, 10), glow_ke=(3, 2, 1), tag="b"):
    """Scene A plus a second emissive object."""
    obj, mtl = glow_cube(tmp, glow_ke, "glow_" + tag)
    return scene_a(cornell=cornell_mtl(tmp, light_ke, "cornell_%s.mtl" % tag)) + [
        ((1.0, 0.5, 4.5), (0, 0.5, 0), (0.3, 0.3, 0.3), obj, mtl)]


def oracle_hdr(oracle, Q, W, H, spp, mb, seed):
    s, _ = Q.render_samples(W, H, spp, mb, seed)
    return oracle.pixel_mean(s, W * H, spp)[0].reshape(H, W, 3)


def dot64(adj, hdr):
    return float((adj.astype(np.float64) * hdr.astype(np.float64)).sum())


def pos_adj(W, H, seed=7):
    # positive: a signed image cancels in sum(adj * I) and buries the identities' signal
    return np.random.RandomState(seed).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)


def render_mat_dev(P, kd, ks, ke, W, H, spp, mb, seed):
    """ipt_render_mat_dev with device arrays (None: the scene's own)."""
    from inverse_path_tracer_amd import _native as N

    t = [None if v is None else torch.tensor(np.ascontiguousarray(v, np.float32), device="cuda") for v in (kd, ks, ke)]
    hdr = torch.empty((H, W, 3), device="cuda", dtype=torch.float32)
    p = N.make_params(W, H, spp, mb, seed)
    N.check(N.lib().ipt_render_mat_dev(P.handle, C.byref(p), *[None if x is None else x.data_ptr() for x in t],
                                       hdr.data_ptr(), None, torch.cuda.current_stream().cuda_stream), "render_mat")
    return hdr.cpu().numpy()


@pytest.fixture(scope="module")
def A(oracle):
    P, Q = product_scene(scene_a()), oracle.OracleScene(scene_a())
    yield P, Q
    P.close()


# ------------------------------------------------------------- 1. forward with overrides
def test_forward_with_overrides_is_the_oracles(oracle, tmp_path):
    ks_new, ke_new = (0.3, 0.45, 0.6), (7.5, 9.25, 11.0)
    P = product_scene(scene_a())
    Q = oracle.OracleScene(scene_a(cornell_mtl(tmp_path, ke_new), phong_mtl(tmp_path, ks_new)))
    kd, ks, ke, _ = P.material_params()
    ks[P.lobe_mask] = np.float32(ks_new)
    ke[P.emitter_mask] = np.float32(ke_new)
    cases = [(32, 32, 8, 4, 3), (24, 16, 5, None, 9)]
    want = {c: Q.render_samples(*c)[0] for c in cases}
    # (b) first, on the scene's load-time values: device-pointer overrides; rows outside the masks are
    # given junk, which the pack kernel must force to 0
    junk_ks, junk_ke = ks.copy(), ke.copy()
    junk_ks[~P.lobe_mask] = 0.77
    junk_ke[~P.emitter_mask] = 5.0
    for c in cases:
        W, H, spp = c[:3]
        hq = oracle.pixel_mean(want[c], W * H, spp)[0]
        got = render_mat_dev(P, None, junk_ks, junk_ke, *c)
        assert np.array_equal(bits(got.reshape(-1, 3)), bits(hq)), c
    # an override launch leaves the scene's own tables alone
    s0, _ = oracle.OracleScene(scene_a()).render_samples(*cases[0])
    assert np.array_equal(bits(P.render_samples(*cases[0])), bits(s0))
    # (a) set_material_params: the samples are the oracle's
    P.set_material_params(ks=ks, ke=ke)
    for c in cases:
        assert np.array_equal(bits(P.render_samples(*c)), bits(want[c])), c
    P.close()


# ------------------------------------------------------------- 2. the Kd block
@pytest.mark.parametrize("W,H,spp,mb", [(32, 32, 8, 4), (20, 12, 3, 5), (24, 16, 5, 20)])
def test_kd_block_is_the_existing_adjoint(A, W, H, spp, mb):
    P, Q = A
    adj = np.random.RandomState(W).uniform(-1, 1, (H, W, 3)).astype(np.float32)
    gkd, gks, gke = P.adjoint_materials(adj, W, H, spp, mb, 4)
    np.testing.assert_allclose(gkd, Q.adjoint(W, H, spp, mb, 4, adj), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gkd, P.adjoint(adj, W, H, spp, mb, 4), rtol=1e-9, atol=1e-12)
    assert np.all(gks[~P.lobe_mask] == 0) and np.any(gks[P.lobe_mask] != 0)
    assert np.all(gke[~P.emitter_mask] == 0) and np.all(gke[P.emitter_mask] != 0)


def test_kd_block_non_spec_instance(oracle):
    P, Q = product_scene(SCENE0), oracle.OracleScene(SCENE0)
    adj = np.random.RandomState(2).uniform(-1, 1, (16, 16, 3)).astype(np.float32)
    gkd, gks, gke = P.adjoint_materials(adj, 16, 16, 4, 0, 1)
    np.testing.assert_allclose(gkd, Q.adjoint(16, 16, 4, 0, 1, adj), rtol=1e-9, atol=1e-12)
    assert not P.lobe_mask.any() and np.all(gks == 0)
    assert np.all(gke[~P.emitter_mask] == 0) and np.all(gke[P.emitter_mask] != 0)
    P.close()


def test_kd_block_spec_bvh_instance_and_hot_set(oracle, tmp_path):
    """The Phong-sphere scene of test_gpu.py (SPEC x BVH; nT > 512: the hot-set bin map)."""
    mtl = tmp_path / "shiny.mtl"
    mtl.write_text("newmtl shiny\nKd 0.2 0.6 0.3\nKs 0.4 0.4 0.4\nNs 30\n")
    src = open(SPHERE_OBJ).read()
    i = src.index("\nf ") + 1
    obj = tmp_path / "sphere_shiny.obj"
    obj.write_text(src[:i] + "mtllib shiny.mtl\nusemtl shiny\n" + src[i:])
    recs = SCENE0 + [((-1.2, -1.35, 4.6), (0, 0, 0), (1.2, 1.2, 1.2), str(obj), str(mtl))]
    P, Q = product_scene(recs), oracle.OracleScene(recs)
    assert P.nT > 1000 and P.bvh_info()["accel"] == "bvh"
    W, H, spp, mb, seed = 32, 24, 8, 4, 12
    adj = np.random.RandomState(3).uniform(-1, 1, (H, W, 3)).astype(np.float32)
    gkd, gks, gke = P.adjoint_materials(adj, W, H, spp, mb, seed)
    np.testing.assert_allclose(gkd, Q.adjoint(W, H, spp, mb, seed, adj), rtol=1e-9, atol=1e-12)
    lobe, emit = P.lobe_mask, P.emitter_mask
    assert lobe.sum() == 1280 and emit.sum() == P.nE
    assert np.all(gks[~lobe] == 0) and np.all(gke[~emit] == 0)
    assert np.count_nonzero(gks[lobe]) > 100 and np.all(gke[emit] != 0)
    P.close()


# ------------------------------------------------------------- 3. Ke by homogeneity
# Calibration (CPU oracle alone, the same frames: scene B, 32x32x8, mb 3, seed 11, the adjoint image
# below): the analogous identity on the oracle's own Kd adjoint -- the derivative of F = sum(adj * I) along
# t -> t * Kd_A at t = 1 (five-point stencil, h = 0.125, exact for mb <= 3) against sum(Kd_A * gKd_A), per
# object A -- is off by at most 6.78e-8 of |F| (3.9e-4 absolute at F = 5812.9).  The bar is 8x that.
REL_KE = 8 * 6.78e-8


def test_ke_by_homogeneity(oracle, tmp_path):
    W = H = 32
    spp, mb, seed = 8, 3, 11
    adj = pos_adj(W, H)
    P = product_scene(scene_b(tmp_path))
    Q = oracle.OracleScene(scene_b(tmp_path))
    assert P.nE == 14
    ke = P.material_params()[2].astype(np.float64)
    hdr = oracle_hdr(oracle, Q, W, H, spp, mb, seed)
    F = dot64(adj, hdr)
    for rows in (slice(0, H), slice(0, H, 2), slice(1, H, 2)):  # the full frame and both interleaved shares
        step = rows.step or 1
        _, _, gke = P.adjoint_materials(adj, W, H, spp, mb, seed, rows.start, H, step)
        for c in range(3):
            want = dot64(adj[rows, :, c], hdr[rows, :, c])
            got = float((ke[:, c] * gke[:, c]).sum())
            print("Ke homogeneity rows %s channel %d: %.9g vs %.9g (%.2e of the bar)" %
                  (rows, c, got, want, abs(got - want) / (REL_KE * abs(want))))
            assert abs(got - want) <= REL_KE * abs(want), (rows, c)
    # per emitter object: phi(2 Ke_A) - phi(Ke_A) = sum_c Ke_A[c] * sum_{e in A} gKe[e, c]
    _, _, gke = P.adjoint_materials(adj, W, H, spp, mb, seed)
    light = np.zeros(P.nT, bool)
    light[:18] = P.emitter_mask[:18]
    glow = P.emitter_mask & ~light
    assert light.sum() == 2 and glow.sum() == 12
    for mask, kw in ((light, {"light_ke": (20, 20, 20)}), (glow, {"glow_ke": (6, 4, 2)})):
        Q2 = oracle.OracleScene(scene_b(tmp_path, tag="x%d" % mask.sum(), **kw))
        d = dot64(adj, oracle_hdr(oracle, Q2, W, H, spp, mb, seed)) - F
        got = float((ke[mask] * gke[mask]).sum())
        print("Ke doubling (%d triangles): %.9g vs %.9g (%.2e of the bar)" %
              (mask.sum(), got, d, abs(got - d) / (REL_KE * abs(F))))
        assert abs(got - d) <= REL_KE * abs(F)
    P.close()


# ------------------------------------------------------------- 4. Ks by a five-point stencil
# Calibration (CPU oracle alone; scene A, 32x32x8, mb 1-3, seed 11, the adjoint image below, h = 0.125):
# the identical stencil on Kd against the oracle's Kd adjoint.  Worst absolute discrepancy over the
# per-material directions (five materials, all channels and each channel; derivatives up to 2077): 2.02e-4;
# over six single (triangle, channel) entries of the cube (derivatives up to 11.2): 2.39e-5.  The bars are
# 8x those.
TOL_KS_MATERIAL = 8 * 2.02e-4
TOL_KS_ENTRY = 8 * 2.39e-5
H_KS = 0.125


def stencil(f, h=H_KS):
    return (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)


@pytest.mark.parametrize("mb", [1, 2, 3])
def test_ks_by_five_point_stencil(A, oracle, tmp_path, mb):
    W = H = 32
    spp, seed = 8, 11
    adj = pos_adj(W, H)
    P0, _ = A
    _, gks, _ = P0.adjoint_materials(adj, W, H, spp, mb, seed)
    lobe = P0.lobe_mask
    # per material, through the oracle forward and MTL files: all channels, then each channel
    for d in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        def f(t):
            ks = [0.5 + t * x for x in d]
            Q = oracle.OracleScene(scene_a(phong=phong_mtl(tmp_path, ks, "ks_%d_%s.mtl" % (mb, g9(ks).replace(" ", "_")))))
            return dot64(adj, oracle_hdr(oracle, Q, W, H, spp, mb, seed))
        want = stencil(f)
        got = float((gks[lobe] * np.float64(d)).sum())
        print("Ks material direction %s mb %d: adjoint %.9g stencil %.9g (%.2e of the bar)" %
              (d, mb, got, want, abs(got - want) / TOL_KS_MATERIAL))
        assert abs(got - want) <= TOL_KS_MATERIAL, d
    # six single (triangle, channel) entries of the cube, through the GPU forward and set_material_params
    P = product_scene(scene_a())
    ks0 = P.material_params()[1]
    cube = np.flatnonzero(lobe)
    for ti, c in [(cube[0], 0), (cube[3], 1), (cube[5], 2), (cube[6], 0), (cube[8], 1), (cube[11], 2)]:
        def f(t):
            ks = ks0.copy()
            ks[ti, c] = np.float32(0.5 + t)
            P.set_material_params(ks=ks)
            return dot64(adj, P.render(W, H, spp, mb, seed))
        want = stencil(f)
        print("Ks entry (%d, %d) mb %d: adjoint %.9g stencil %.9g (%.2e of the bar)" %
              (ti, c, mb, gks[ti, c], want, abs(gks[ti, c] - want) / TOL_KS_ENTRY))
        assert abs(gks[ti, c] - want) <= TOL_KS_ENTRY, (ti, c)
    P.close()


# ------------------------------------------------------------- 5. sharding and linearity
def test_row_bands_sum_to_full_and_linearity(A):
    from inverse_path_tracer_amd.distributed import shard_rows

    P, _ = A
    W, H, spp, mb, seed = 32, 32, 8, 4, 5
    a1, a2 = pos_adj(W, H, 1), pos_adj(W, H, 2)
    full = np.stack(P.adjoint_materials(a1, W, H, spp, mb, seed))
    parts = sum(np.stack(P.adjoint_materials(a1, W, H, spp, mb, seed, *shard_rows(H, 4, r))) for r in range(4))
    np.testing.assert_allclose(parts, full, rtol=1e-10)
    # linear in the adjoint image: doubling is exact in fp32 (only the fp64 summation order differs) ...
    np.testing.assert_allclose(np.stack(P.adjoint_materials(2 * a1, W, H, spp, mb, seed)), 2 * full, rtol=1e-10)
    # ... and additivity holds to the float32 rounding of a1 + a2 and of the per-sample products
    # adj/spp * g (<= 4 roundings of 2^-24 on sums of same-signed terms: 2.4e-7)
    g2 = np.stack(P.adjoint_materials(a2, W, H, spp, mb, seed))
    g12 = np.stack(P.adjoint_materials(a1 + a2, W, H, spp, mb, seed))
    np.testing.assert_allclose(g12, full + g2, rtol=2.4e-7)
    for blk in full:
        assert np.any(blk != 0)


# ------------------------------------------------------------- 6. the torch op
def test_torch_op(A, oracle):
    from inverse_path_tracer_amd import torch_ops

    P, Q = A
    W, H, spp, mb, seed = 40, 24, 8, 4, 6
    kd0, ks0, ke0, _ = P.material_params()
    kd, ks, ke = (torch.tensor(v, device="cuda", requires_grad=True) for v in (kd0, ks0, ke0))
    img = torch_ops.render_materials(P, kd, ks, ke, W, H, spp, mb, seed)
    assert np.array_equal(bits(img.detach().cpu().numpy()), bits(oracle_hdr(oracle, Q, W, H, spp, mb, seed)))
    adj = torch.tensor(pos_adj(W, H, 3), device="cuda")
    (img * adj).sum().backward()
    want = P.adjoint_materials(adj.cpu().numpy(), W, H, spp, mb, seed)
    for t, g in zip((kd, ks, ke), want):
        assert t.grad is not None and t.grad.dtype == torch.float32
        np.testing.assert_allclose(t.grad.cpu().numpy(), g, rtol=1e-6, atol=1e-30)
    # None and no-grad inputs
    ks2 = torch.tensor(ks0, device="cuda", requires_grad=True)
    img2 = torch_ops.render_materials(P, None, ks2, ke.detach(), W, H, spp, mb, seed)
    assert torch.equal(img2, img.detach())
    (img2 * adj).sum().backward()
    np.testing.assert_allclose(ks2.grad.cpu().numpy(), want[1], rtol=1e-6, atol=1e-30)
    # a band with interleaved rows
    ke3 = torch.tensor(ke0, device="cuda", requires_grad=True)
    band = torch_ops.render_materials(P, None, None, ke3, W, H, spp, mb, seed, row_begin=1, row_step=3)
    assert torch.equal(band, img.detach()[1::3])
    (band * adj[1::3]).sum().backward()
    np.testing.assert_allclose(ke3.grad.cpu().numpy(),
                               P.adjoint_materials(adj.cpu().numpy(), W, H, spp, mb, seed, 1, H, 3)[2],
                               rtol=1e-6, atol=1e-30)


@pytest.mark.parametrize("band", [(2, 8, 2), (3, 7, 1)], ids=["rows-2-4-6", "rows-3-to-6"])
def test_torch_op_band_with_adjoint_seed(band):
    """A band of interleaved rows (scattered into a full frame) and a band of consecutive rows (the band's
    pointer moved back by row_begin rows), each with the backward on a stream of its own: the op's gradient
    is the host method's at that seed and band (two launches of one adjoint: test_torch_op's bound)."""
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.scene import Scene

    P = Scene.from_file(os.path.join(ASSETS, "phong", "scene0_phong.txt"))
    W, H, spp, mb, seed, aseed = 8, 8, 4, 2, 6, 6 + 8 * 8 * 4
    rb, re_, rs = band
    kd0, ks0, ke0, _ = P.material_params()
    kd, ks, ke = (torch.tensor(v, device="cuda", requires_grad=True) for v in (kd0, ks0, ke0))
    img = torch_ops.render_materials(P, kd, ks, ke, W, H, spp, mb, seed, rb, re_, adjoint_seed=aseed, row_step=rs)
    assert np.array_equal(bits(img.detach().cpu().numpy()), bits(P.render(W, H, spp, mb, seed)[rb:re_:rs]))
    adj = pos_adj(W, H, 3)
    (img * torch.tensor(adj[rb:re_:rs], device="cuda")).sum().backward()
    want = P.adjoint_materials(adj, W, H, spp, mb, aseed, rb, re_, rs)
    for t, g in zip((kd, ks, ke), want):
        assert np.any(g != 0)
        np.testing.assert_allclose(t.grad.cpu().numpy(), g, rtol=1e-6, atol=1e-30)
    P.close()


# ------------------------------------------------------------- 7. recovery
def test_recovery_of_cube_ks_and_light_ke():
    from inverse_path_tracer_amd import torch_ops

    P = product_scene(scene_a())
    W = H = 64
    spp, mb, seed = 16, 3, 100
    _, ks0, ke0, _ = P.material_params()
    lobe = torch.tensor(P.lobe_mask, device="cuda")[:, None].float()
    emit = torch.tensor(P.emitter_mask, device="cuda")[:, None].float()
    true_ks, true_ke = torch.full((3,), 0.5, device="cuda"), torch.full((3,), 10.0, device="cuda")
    with torch.no_grad():
        target = torch_ops.render_materials(P, None, lobe * true_ks, emit * true_ke, W, H, spp, mb, seed)
    assert torch.equal(target, torch.tensor(P.render(W, H, spp, mb, seed), device="cuda"))
    # one parameter vector per material: the cube's Ks, the light's Ke (back faces get no gradient of their own)
    ks_p = torch.tensor([0.2, 0.8, 0.3], device="cuda", requires_grad=True)
    ke_p = torch.tensor([6.0, 14.0, 7.0], device="cuda", requires_grad=True)
    e0 = (float((ks_p.detach() - true_ks).abs().mean()), float((ke_p.detach() - true_ke).abs().mean()))
    opt = torch.optim.Adam([{"params": [ks_p], "lr": 0.02}, {"params": [ke_p], "lr": 0.2}])
    frame = W * H * spp
    for step in range(200):
        opt.zero_grad()
        img = torch_ops.render_materials(P, None, lobe * ks_p, emit * ke_p, W, H, spp, mb, seed,
                                         adjoint_seed=seed + (step + 1) * frame)
        ((img - target) ** 2).mean().backward()
        opt.step()
    e1 = (float((ks_p.detach() - true_ks).abs().mean()), float((ke_p.detach() - true_ke).abs().mean()))
    print("recovery: Ks error %.4f -> %.4f, Ke error %.4f -> %.4f" % (e0[0], e1[0], e0[1], e1[1]))
    assert e1[0] <= 0.5 * e0[0] and e1[1] <= 0.5 * e0[1]
    P.close()


# ------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_stream_usable(A):
    from inverse_path_tracer_amd import NativeError, torch_ops

    P, _ = A
    W, H, spp, mb, seed = 16, 16, 4, 3, 2
    adj = pos_adj(W, H)
    before = np.stack(P.adjoint_materials(adj, W, H, spp, mb, seed))
    with pytest.raises(NativeError, match="unbounded estimator"):
        P.adjoint_materials(adj, W, H, spp, None, seed)
    with pytest.raises(NativeError, match="max_bounces <= 62"):
        P.adjoint_materials(adj, W, H, spp, 63, seed)
    kd = torch.tensor(P.materials, device="cuda")
    with pytest.raises(NativeError, match="unbounded estimator"):
        torch_ops.render_materials(P, kd, None, None, W, H, spp, None, seed)
    with pytest.raises(NativeError, match="scene batch"):
        torch_ops.render_materials(P, kd[None].repeat(2, 1, 1), None, None, W, H, spp, mb, seed)
    # later ordinary launches on the same stream are unaffected
    np.testing.assert_allclose(np.stack(P.adjoint_materials(adj, W, H, spp, mb, seed)), before, rtol=1e-10)
    np.testing.assert_allclose(P.adjoint(adj, W, H, spp, mb, seed), before[0], rtol=1e-9, atol=1e-12)
