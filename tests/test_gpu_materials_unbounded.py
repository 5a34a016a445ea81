"""Gradients for Kd, Ks and Ke of the reference's own estimator: no bounce cap,
paths end by Russian roulette or a miss (run with -m gpu).

The unbounded material adjoint (trace_matu_kernel) is the
unbounded adjoint's ring-and-replay sweep with the material adjoint's blocks.
These tests predate the oracle's material adjoint (every entry is compared with
it in tests/test_gpu_materials_oracle.py), so -- as tests/test_gpu_materials.py
does for the bounded one -- the new blocks are checked by identities:
  * the Kd block is the oracle's unbounded adjoint (rtol 1e-9);
  * all three blocks equal the bounded material adjoint at a bounce cap that
    no path of the frame reaches, at the default ring and at rings
    forced tiny (replays: where the first-triangle carry and the carried
    suffix can go wrong);
  * Ke: sum Ke * gKe equals the oracle's unbounded forward (homogeneity);
  * Ks: a five-point stencil on the oracle's / the GPU's unbounded forward;
  * row bands, linearity, the torch op, a recovery run, the refusals.

The identities' tolerances are reference-only: measured on the CPU oracle's
own unbounded Kd adjoint by tools/matgrad_calibrate_unbounded.py (its figures
are written beside the constants, the bars are 8x them).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ASSETS, SCENE0, SPHERE_OBJ, product_scene
from test_gpu_materials import (bits, dot64, g9, oracle_hdr, phong_mtl, pos_adj, scene_a, scene_b, stencil)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RINGS = [None, (1, 1), (2, 1), (3, 2), (1, 4)]  # ipt_debug_adju_ring (pool chunks per wave, LDS slots per lane)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


class ring:
    """The unbounded adjoints' record ring forced small for the block (None: the launch's choice)."""

    def __init__(self, size):
        self.size = size

    def __enter__(self):
        from inverse_path_tracer_amd import _native as N

        if self.size:
            N.lib().ipt_debug_adju_ring(*self.size)

    def __exit__(self, *exc):
        from inverse_path_tracer_amd import _native as N

        N.lib().ipt_debug_adju_ring(0, 0)
        return False


def sphere_records(tmp):
    """The Phong-sphere scene of test_gpu_materials.py (SPEC x BVH; nT > 512: the hot-set bin map)."""
    mtl = tmp / "shiny.mtl"
    mtl.write_text("newmtl shiny\nKd 0.2 0.6 0.3\nKs 0.4 0.4 0.4\nNs 30\n")
    src = open(SPHERE_OBJ).read()
    i = src.index("\nf ") + 1
    obj = tmp / "sphere_shiny.obj"
    obj.write_text(src[:i] + "mtllib shiny.mtl\nusemtl shiny\n" + src[i:])
    return SCENE0 + [((-1.2, -1.35, 4.6), (0, 0, 0), (1.2, 1.2, 1.2), str(obj), str(mtl))]


@pytest.fixture(scope="module")
def A(oracle):
    P, Q = product_scene(scene_a()), oracle.OracleScene(scene_a())
    yield P, Q
    P.close()


@pytest.fixture(scope="module")
def SPH(oracle, tmp_path_factory):
    recs = sphere_records(tmp_path_factory.mktemp("sphere"))
    P, Q = product_scene(recs), oracle.OracleScene(recs)
    assert P.nT > 1000 and P.bvh_info()["accel"] == "bvh"
    yield P, Q
    P.close()


# ------------------------------------------------------------- 1. the Kd block
def check_kd_block(P, Q, W, H, spp, seed, rs):
    adj = np.random.RandomState(rs).uniform(-1, 1, (H, W, 3)).astype(np.float32)
    gkd, gks, gke = P.adjoint_materials_unbounded(adj, W, H, spp, seed)
    np.testing.assert_allclose(gkd, Q.adjoint(W, H, spp, None, seed, adj), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gkd, P.adjoint(adj, W, H, spp, None, seed), rtol=1e-9, atol=1e-12)
    lobe, emit = P.lobe_mask, P.emitter_mask
    assert np.all(gks[~lobe] == 0) and np.all(gke[~emit] == 0)
    assert emit.sum() == P.nE and np.all(gke[emit] != 0)
    return gks[lobe]


def test_kd_block_is_the_oracles_unbounded_adjoint(A):
    P, Q = A
    assert np.any(check_kd_block(P, Q, 32, 32, 8, 4, 32) != 0)


def test_kd_block_non_spec_instance(oracle):
    P, Q = product_scene(SCENE0), oracle.OracleScene(SCENE0)
    assert not P.lobe_mask.any()
    assert check_kd_block(P, Q, 16, 16, 4, 1, 2).size == 0
    P.close()


def test_kd_block_spec_bvh_instance_and_hot_set(SPH):
    P, Q = SPH
    gl = check_kd_block(P, Q, 32, 24, 8, 12, 3)
    assert P.lobe_mask.sum() == 1280 and np.count_nonzero(gl) > 100


@pytest.mark.parametrize("W,H,spp,rows", [(30, 30, 3, (0, None, 1)), (30, 30, 5, (9, 16, 1)), (30, 21, 5, (1, None, 3))])
def test_sample_counts_that_are_no_multiple_of_64(A, oracle, W, H, spp, rows):
    """Launches whose sample count is no multiple of the wave size (2700 samples; a 7-row band of 30 x 5; 7
    interleaved rows of 30 x 5): the last wave's grab is partial, so some of its lanes never trace a path
    and never write the words their owner-lane state lives in.  Brute force (scene A, scenes/0.txt) and
    BVH (the sphere is covered by its own fixture below)."""
    P, Q = A
    adj = np.random.RandomState(W + spp).uniform(-1, 1, (H, W, 3)).astype(np.float32)
    band = (rows[0], H if rows[1] is None else rows[1], rows[2])
    assert (len(range(*band)) * W * spp) % 64 != 0
    masked = np.zeros_like(adj)  # the oracle takes no row_step: the full frame with adj = 0 outside the band
    masked[band[0]:band[1]:band[2]] = adj[band[0]:band[1]:band[2]]
    want = Q.adjoint(W, H, spp, None, 21, masked)
    for size in (None, (1, 1)):
        with ring(size):
            gkd, gks, gke = P.adjoint_materials_unbounded(adj, W, H, spp, 21, *band)
        np.testing.assert_allclose(gkd, want, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gkd, P.adjoint(adj, W, H, spp, None, 21, *band), rtol=1e-9, atol=1e-12)
        assert np.all(gks[~P.lobe_mask] == 0) and np.all(gke[~P.emitter_mask] == 0)
        assert np.any(gks != 0) and np.all(gke[P.emitter_mask] != 0)


def test_sample_counts_that_are_no_multiple_of_64_other_instances(SPH, oracle):
    """The same on the diffuse brute-force instance (scenes/0.txt) and the SPEC x BVH one."""
    P0, Q0 = product_scene(SCENE0), oracle.OracleScene(SCENE0)
    for P, Q in ((P0, Q0), SPH):
        adj = np.random.RandomState(5).uniform(-1, 1, (30, 30, 3)).astype(np.float32)
        gkd, _, gke = P.adjoint_materials_unbounded(adj, 30, 30, 3, 21)
        np.testing.assert_allclose(gkd, Q.adjoint(30, 30, 3, None, 21, adj), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gkd, P.adjoint(adj, 30, 30, 3, None, 21), rtol=1e-9, atol=1e-12)
        assert np.all(gke[P.emitter_mask] != 0)
    P0.close()


# ------------------------------------------------------------- 2. against the bounded material adjoint
# The cap.  The bounded adjoint keeps max_bounces + 1 vertex records per lane in LDS, and both scenes run the
# SPEC instances, whose records are 5 words: 63 records are 315 KiB per workgroup, so trace_mat_kernel
# refuses max_bounces = 62 there (160 KiB).  The caps below are what the
# bounded launch takes on each scene (scene A: 28, 30 is refused; the sphere, with 24 KiB of bins: 24).
# The precondition -- the oracle's samples at the cap are bitwise the unbounded samples -- is asserted.
# On the sphere it is not enough: on the 32x24x8 seed 12 frame it holds from 24 bounces on, yet paths of up to
# 37 vertices exist whose tails are below half an ulp of their fp32 sample but 3.7e-9 of a gradient entry
# (measured: 11 of 3930 Kd entries, the same figures at every ring size).  So the sphere runs the 24x16x8
# frame at seed 40012, whose longest path has 24 vertices, and asserts the stronger precondition that the
# cast counts agree as well (no path goes past the cap at all); the 32x24x8 frame checks the tiny rings
# against the default ring instead (63 slots: no path of it replays).
_CAPPED = {}


def capped_reference(name, P, Q, W, H, spp, cap, seed, adj, casts):
    """The bounded material adjoint at max_bounces = cap, once per scene, on a frame where no path
    reaches the cap: the oracle's samples at the cap are bitwise the unbounded ones."""
    if name not in _CAPPED:
        sc, nc = Q.render_samples(W, H, spp, cap, seed)
        su, nu = Q.render_samples(W, H, spp, None, seed)
        assert np.array_equal(bits(sc), bits(su)), "a path of this frame reaches the cap of %d bounces" % cap
        assert not casts or nc == nu, "a path of this frame goes past the cap of %d bounces" % cap
        _CAPPED[name] = np.stack(P.adjoint_materials(adj, W, H, spp, cap, seed))
    return _CAPPED[name]


def check_equals_capped(name, P, Q, W, H, spp, cap, seed, size, casts=False):
    adj = pos_adj(W, H)
    want = capped_reference(name, P, Q, W, H, spp, cap, seed, adj, casts)
    with ring(size):
        got = np.stack(P.adjoint_materials_unbounded(adj, W, H, spp, seed))
    # the two sweeps form the same per-vertex floats; only the fp64 summation order differs, and with a
    # positive adjoint image every bin's terms have one sign
    for blk, g, w in zip(("Kd", "Ks", "Ke"), got, want):
        assert np.array_equal(g == 0, w == 0), blk
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=0, err_msg=blk)
    assert all(np.any(w != 0) for w in want)


@pytest.mark.parametrize("size", RINGS)
def test_equals_the_bounded_material_adjoint_scene_a(A, size):
    P, Q = A
    check_equals_capped("A", P, Q, 32, 32, 8, 28, 11, size)


@pytest.mark.parametrize("size", RINGS)
def test_equals_the_bounded_material_adjoint_phong_sphere(SPH, size):
    P, Q = SPH
    check_equals_capped("sphere", P, Q, 24, 16, 8, 24, 40012, size, casts=True)
    # the larger frame (paths of up to 37 vertices): every ring size against the default ring
    W, H, spp, seed = 32, 24, 8, 12
    adj = pos_adj(W, H)
    if "sphere_default" not in _CAPPED:
        _CAPPED["sphere_default"] = np.stack(P.adjoint_materials_unbounded(adj, W, H, spp, seed))
    with ring(size):
        got = np.stack(P.adjoint_materials_unbounded(adj, W, H, spp, seed))
    assert np.array_equal(got == 0, _CAPPED["sphere_default"] == 0)
    np.testing.assert_allclose(got, _CAPPED["sphere_default"], rtol=1e-10, atol=0)


# ------------------------------------------------------------- 3. Ke by homogeneity
# Calibration (CPU oracle alone, tools/matgrad_calibrate_unbounded.py; scene B, 32x32x8, unbounded, seed 11,
# the adjoint image below): the analogous identity on the oracle's own unbounded Kd adjoint -- the derivative
# of F = sum(adj * I) along t -> t * Kd_A at t = 1 (five-point stencil, h = 0.125) against
# sum(Kd_A * gKd_A), per object A -- is off by at most 2.553e-6 of |F| (F = 5894.01; the stencil is not exact
# for long paths: the bounded figure was 6.78e-8).  The bar is 8x that.
REL_KE = 8 * 2.553e-6


@pytest.mark.parametrize("size", [None, (1, 1)])
def test_ke_by_homogeneity(oracle, tmp_path, size):
    W = H = 32
    spp, seed = 8, 11
    adj = pos_adj(W, H)
    P = product_scene(scene_b(tmp_path))
    Q = oracle.OracleScene(scene_b(tmp_path))
    assert P.nE == 14
    ke = P.material_params()[2].astype(np.float64)
    hdr = oracle_hdr(oracle, Q, W, H, spp, None, seed)
    F = dot64(adj, hdr)
    with ring(size):
        for rows in (slice(0, H), slice(0, H, 2), slice(1, H, 2)):  # the full frame and both interleaved shares
            _, _, gke = P.adjoint_materials_unbounded(adj, W, H, spp, seed, rows.start, H, rows.step or 1)
            for c in range(3):
                want = dot64(adj[rows, :, c], hdr[rows, :, c])
                got = float((ke[:, c] * gke[:, c]).sum())
                print("Ke homogeneity ring %s rows %s channel %d: %.9g vs %.9g (%.2e of the bar)" %
                      (size, rows, c, got, want, abs(got - want) / (REL_KE * abs(want))))
                assert abs(got - want) <= REL_KE * abs(want), (rows, c)
        _, _, gke = P.adjoint_materials_unbounded(adj, W, H, spp, seed)
    # per emitter object: phi(2 Ke_A) - phi(Ke_A) = sum_c Ke_A[c] * sum_{e in A} gKe[e, c]
    light = np.zeros(P.nT, bool)
    light[:18] = P.emitter_mask[:18]
    glow = P.emitter_mask & ~light
    assert light.sum() == 2 and glow.sum() == 12
    for mask, kw in ((light, {"light_ke": (20, 20, 20)}), (glow, {"glow_ke": (6, 4, 2)})):
        Q2 = oracle.OracleScene(scene_b(tmp_path, tag="x%d" % mask.sum(), **kw))
        d = dot64(adj, oracle_hdr(oracle, Q2, W, H, spp, None, seed)) - F
        got = float((ke[mask] * gke[mask]).sum())
        print("Ke doubling ring %s (%d triangles): %.9g vs %.9g (%.2e of the bar)" %
              (size, mask.sum(), got, d, abs(got - d) / (REL_KE * abs(F))))
        assert abs(got - d) <= REL_KE * abs(F)
    P.close()


# ------------------------------------------------------------- 4. Ks by a five-point stencil
# Calibration (CPU oracle alone, tools/matgrad_calibrate_unbounded.py; scene A, 32x32x8, unbounded, seed 11,
# the adjoint image below, h = 0.125): the identical stencil on Kd against the oracle's unbounded Kd adjoint,
# for the directions used here.  The cube's material, all channels and each channel (derivatives 70.4, 26.0,
# 22.3, 22.1): off by 1.33e-5, 8.19e-6, 2.66e-5, 2.15e-5 -- worst 2.657e-5.  The six single (triangle,
# channel) entries of the cube: worst 2.427e-5.  The bars are 8x those.  (The stencil is not exact here:
# paths are long, the radiance a polynomial of high degree; smaller h was worse, fp32 noise.)
TOL_KS_MATERIAL = 8 * 2.657e-5
TOL_KS_ENTRY = 8 * 2.427e-5


def test_ks_by_five_point_stencil(A, oracle, tmp_path):
    W = H = 32
    spp, seed = 8, 11
    adj = pos_adj(W, H)
    P0, _ = A
    _, gks, _ = P0.adjoint_materials_unbounded(adj, W, H, spp, seed)
    lobe = P0.lobe_mask
    # per material, through the oracle forward and MTL files: all channels, then each channel
    for d in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        def f(t):
            ks = [0.5 + t * x for x in d]
            Q = oracle.OracleScene(scene_a(phong=phong_mtl(tmp_path, ks, "ks_%s.mtl" % g9(ks).replace(" ", "_"))))
            return dot64(adj, oracle_hdr(oracle, Q, W, H, spp, None, seed))
        want = stencil(f)
        got = float((gks[lobe] * np.float64(d)).sum())
        print("Ks material direction %s: adjoint %.9g stencil %.9g (%.2e of the bar)" %
              (d, got, want, abs(got - want) / TOL_KS_MATERIAL))
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
            return dot64(adj, P.render(W, H, spp, None, seed))
        want = stencil(f)
        print("Ks entry (%d, %d): adjoint %.9g stencil %.9g (%.2e of the bar)" %
              (ti, c, gks[ti, c], want, abs(gks[ti, c] - want) / TOL_KS_ENTRY))
        assert abs(gks[ti, c] - want) <= TOL_KS_ENTRY, (ti, c)
    P.close()


# ------------------------------------------------------------- 5. sharding and linearity
def test_row_bands_sum_to_full_and_linearity(A):
    from inverse_path_tracer_amd.distributed import shard_rows

    P, _ = A
    W, H, spp, seed = 32, 32, 8, 5
    a1 = pos_adj(W, H, 1)
    with ring((2, 1)):
        full = np.stack(P.adjoint_materials_unbounded(a1, W, H, spp, seed))
        parts = sum(np.stack(P.adjoint_materials_unbounded(a1, W, H, spp, seed, *shard_rows(H, 4, r)))
                    for r in range(4))
        twice = np.stack(P.adjoint_materials_unbounded(2 * a1, W, H, spp, seed))
    np.testing.assert_allclose(parts, full, rtol=1e-10)
    # doubling the adjoint image is exact in fp32: only the fp64 summation order differs
    np.testing.assert_allclose(twice, 2 * full, rtol=1e-10)
    for blk in full:
        assert np.any(blk != 0)


# ------------------------------------------------------------- 6. the torch op
def test_torch_op(A, oracle):
    from inverse_path_tracer_amd import torch_ops

    P, Q = A
    W, H, spp, seed = 40, 24, 8, 6
    kd0, ks0, ke0, _ = P.material_params()
    kd, ks, ke = (torch.tensor(v, device="cuda", requires_grad=True) for v in (kd0, ks0, ke0))
    img = torch_ops.render_materials_unbounded(P, kd, ks, ke, W, H, spp, seed)
    assert np.array_equal(bits(img.detach().cpu().numpy()), bits(oracle_hdr(oracle, Q, W, H, spp, None, seed)))
    adj = torch.tensor(pos_adj(W, H, 3), device="cuda")
    (img * adj).sum().backward()
    want = P.adjoint_materials_unbounded(adj.cpu().numpy(), W, H, spp, seed)
    for t, g in zip((kd, ks, ke), want):
        assert t.grad is not None and t.grad.dtype == torch.float32
        np.testing.assert_allclose(t.grad.cpu().numpy(), g, rtol=1e-6, atol=1e-30)
    # None and no-grad inputs
    ks2 = torch.tensor(ks0, device="cuda", requires_grad=True)
    img2 = torch_ops.render_materials_unbounded(P, None, ks2, ke.detach(), W, H, spp, seed)
    assert torch.equal(img2, img.detach())
    (img2 * adj).sum().backward()
    np.testing.assert_allclose(ks2.grad.cpu().numpy(), want[1], rtol=1e-6, atol=1e-30)
    # a band with interleaved rows
    ke3 = torch.tensor(ke0, device="cuda", requires_grad=True)
    band = torch_ops.render_materials_unbounded(P, None, None, ke3, W, H, spp, seed, row_begin=1, row_step=3)
    assert torch.equal(band, img.detach()[1::3])
    (band * adj[1::3]).sum().backward()
    np.testing.assert_allclose(ke3.grad.cpu().numpy(),
                               P.adjoint_materials_unbounded(adj.cpu().numpy(), W, H, spp, seed, 1, H, 3)[2],
                               rtol=1e-6, atol=1e-30)
    # an independent sample stream for the backward: the adjoint of that frame
    ke4 = torch.tensor(ke0, device="cuda", requires_grad=True)
    img4 = torch_ops.render_materials_unbounded(P, None, None, ke4, W, H, spp, seed, adjoint_seed=seed + W * H * spp)
    assert torch.equal(img4, img.detach())
    (img4 * adj).sum().backward()
    np.testing.assert_allclose(ke4.grad.cpu().numpy(),
                               P.adjoint_materials_unbounded(adj.cpu().numpy(), W, H, spp, seed + W * H * spp)[2],
                               rtol=1e-6, atol=1e-30)


@pytest.mark.parametrize("band", [(2, 8, 2), (3, 7, 1)], ids=["rows-2-4-6", "rows-3-to-6"])
def test_torch_op_band_with_adjoint_seed(band):
    """A band of interleaved rows (scattered into a full frame) and a band of consecutive rows (the band's
    pointer moved back by row_begin rows), each with the backward on a stream of its own: the op's gradient
    is the host method's at that seed and band (two launches of one adjoint: test_torch_op's bound)."""
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.scene import Scene

    P = Scene.from_file(os.path.join(ASSETS, "phong", "scene0_phong.txt"))
    W, H, spp, seed, aseed = 8, 8, 4, 6, 6 + 8 * 8 * 4
    rb, re_, rs = band
    kd0, ks0, ke0, _ = P.material_params()
    kd, ks, ke = (torch.tensor(v, device="cuda", requires_grad=True) for v in (kd0, ks0, ke0))
    img = torch_ops.render_materials_unbounded(P, kd, ks, ke, W, H, spp, seed, rb, re_, adjoint_seed=aseed,
                                               row_step=rs)
    assert np.array_equal(bits(img.detach().cpu().numpy()), bits(P.render(W, H, spp, None, seed)[rb:re_:rs]))
    adj = pos_adj(W, H, 3)
    (img * torch.tensor(adj[rb:re_:rs], device="cuda")).sum().backward()
    want = P.adjoint_materials_unbounded(adj, W, H, spp, aseed, rb, re_, rs)
    for t, g in zip((kd, ks, ke), want):
        assert np.any(g != 0)
        np.testing.assert_allclose(t.grad.cpu().numpy(), g, rtol=1e-6, atol=1e-30)
    P.close()


# ------------------------------------------------------------- 7. recovery
def test_recovery_of_cube_ks_and_light_ke():
    from inverse_path_tracer_amd import torch_ops

    P = product_scene(scene_a())
    W = H = 64
    spp, seed = 16, 100
    lobe = torch.tensor(P.lobe_mask, device="cuda")[:, None].float()
    emit = torch.tensor(P.emitter_mask, device="cuda")[:, None].float()
    true_ks, true_ke = torch.full((3,), 0.5, device="cuda"), torch.full((3,), 10.0, device="cuda")
    with torch.no_grad():
        target = torch_ops.render_materials_unbounded(P, None, lobe * true_ks, emit * true_ke, W, H, spp, seed)
    assert torch.equal(target, torch.tensor(P.render(W, H, spp, None, seed), device="cuda"))
    ks_p = torch.tensor([0.2, 0.8, 0.3], device="cuda", requires_grad=True)
    ke_p = torch.tensor([6.0, 14.0, 7.0], device="cuda", requires_grad=True)
    e0 = (float((ks_p.detach() - true_ks).abs().mean()), float((ke_p.detach() - true_ke).abs().mean()))
    opt = torch.optim.Adam([{"params": [ks_p], "lr": 0.02}, {"params": [ke_p], "lr": 0.2}])
    frame = W * H * spp
    for step in range(200):
        opt.zero_grad()
        img = torch_ops.render_materials_unbounded(P, None, lobe * ks_p, emit * ke_p, W, H, spp, seed,
                                                   adjoint_seed=seed + (step + 1) * frame)
        ((img - target) ** 2).mean().backward()
        opt.step()
    e1 = (float((ks_p.detach() - true_ks).abs().mean()), float((ke_p.detach() - true_ke).abs().mean()))
    print("unbounded recovery: Ks error %.4f -> %.4f, Ke error %.4f -> %.4f" % (e0[0], e1[0], e0[1], e1[1]))
    assert e1[0] <= 0.5 * e0[0] and e1[1] <= 0.5 * e0[1]
    P.close()


# ------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_stream_usable(A):
    from inverse_path_tracer_amd import NativeError, torch_ops
    from inverse_path_tracer_amd import _native as N

    P, _ = A
    W, H, spp, seed = 16, 16, 4, 2
    adj = pos_adj(W, H)
    before = np.stack(P.adjoint_materials_unbounded(adj, W, H, spp, seed))
    capped = np.stack(P.adjoint_materials(adj, W, H, spp, 3, seed))
    # the new entry point takes no bounce cap, and says which call does
    a = torch.tensor(adj, device="cuda")
    g = torch.zeros((3, P.nT, 3), device="cuda", dtype=torch.float64)
    p3 = N.make_params(W, H, spp, 3, seed)
    rc = N.lib().ipt_adjoint_mat_unbounded_dev(P.handle, C.byref(p3), None, None, None, a.data_ptr(), g.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and "ipt_adjoint_mat_dev" in N.last_error(), N.last_error()
    assert float(g.abs().sum()) == 0.0
    # ... and an invalid frame is refused with the frame's message
    p0 = N.make_params(W, H, 0, None, seed)
    rc = N.lib().ipt_adjoint_mat_unbounded_dev(P.handle, C.byref(p0), None, None, None, a.data_ptr(), g.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and "invalid render parameters" in N.last_error(), N.last_error()
    # the bounded entry points still refuse the unbounded estimator, and name the new one
    with pytest.raises(NativeError, match="unbounded estimator") as e:
        P.adjoint_materials(adj, W, H, spp, None, seed)
    assert "ipt_adjoint_mat_unbounded_dev" in str(e.value)
    kd = torch.tensor(P.materials, device="cuda")
    with pytest.raises(NativeError, match="unbounded estimator") as e:
        torch_ops.render_materials(P, kd, None, None, W, H, spp, None, seed)
    assert "render_materials_unbounded" in str(e.value)
    with pytest.raises(NativeError, match="unbounded estimator"):
        torch_ops.render_materials_batch(P, kd[None].repeat(2, 1, 1), None, None, W, H, spp, None, seed)
    with pytest.raises(NativeError, match="scene batch"):
        torch_ops.render_materials_unbounded(P, kd[None].repeat(2, 1, 1), None, None, W, H, spp, seed)
    # later ordinary launches on the same stream are unaffected
    np.testing.assert_allclose(np.stack(P.adjoint_materials_unbounded(adj, W, H, spp, seed)), before, rtol=1e-10)
    np.testing.assert_allclose(np.stack(P.adjoint_materials(adj, W, H, spp, 3, seed)), capped, rtol=1e-10)
    np.testing.assert_allclose(P.adjoint(adj, W, H, spp, None, seed), before[0], rtol=1e-9, atol=1e-12)
