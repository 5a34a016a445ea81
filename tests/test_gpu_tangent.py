"""The tangent launch on the GPU (run with -m gpu): ipt_tangent_mat_dev / trace_tan_kernel.

tan[k, p, c] is <the material adjoint's gradient under the one-hot adjoint image at p, tangent k> in channel c, so
every entry is compared with the CPU oracle's material adjoint (tests/test_oracle_tangent.py owns the reference, the
tangents and the bar: |T - T_ref| <= 1e-9 A_ref + 1e-12 with A_ref the sum of the absolute products, exact zeros where
A_ref is 0).  Instances: SPEC brute force (scene B, tangent tables in LDS), non-SPEC with many emitters (the emissive
cube), SPEC x BVH with the tangents read from global memory by triangle (the Phong sphere).  Then: K tangents in one
launch against K launches, the dot-product identity with Scene.adjoint_materials at a larger frame, device overrides,
forward-mode AD through render_materials, the Gauss-Newton driver, and the stream after a refused call.
"""
import numpy as np
import pytest

import test_oracle_materials as OM
import test_oracle_tangent as OT
from conftest import SCENE0, product_scene
from test_gpu_materials import bits, scene_b

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


class Pair:
    """A scene in the product and in the oracle under the same drawn values (masked rows carry junk)."""

    def __init__(self, oracle, name, records):
        self.name = name
        self.P, self.Q = product_scene(records), oracle.OracleScene(records)
        self.values = OM.draw_values(self.Q, 2)
        self.P.set_material_params(*self.values[0])
        self.Q.set_material_params(*self.values[0])
        for got, want in zip(self.P.material_params()[:3], self.Q.material_params()):
            assert np.array_equal(bits(got), bits(want))

    def run(self, f, K, seed=77):
        tang = OT.draw_tangents(self.Q, K, seed)
        got = self.P.tangent_materials(*tang, f.W, f.H, f.spp, f.mb, f.seed, *OM.frame_rows(f))
        T, A = OT.reference(self.Q, self.name, f, tang)
        OT.compare(got, T, A, tag="%s %s K=%d" % (self.name, OM.frame_id(f), K))
        return got, T, A


@pytest.fixture(scope="module")
def B(oracle, tmp_path_factory):
    pair = Pair(oracle, "B", scene_b(tmp_path_factory.mktemp("tan_b"), tag="t"))
    assert pair.P.nT == 42 and pair.P.nE == 14 and pair.P.lobe_mask.sum() == 12
    yield pair
    pair.P.close()


@pytest.fixture(scope="module")
def GLOW(oracle, tmp_path_factory):
    pair = Pair(oracle, "glow", OM.glow_records(tmp_path_factory.mktemp("tan_glow")))
    assert pair.P.nT == 30 and pair.P.nE == 14 and not pair.P.lobe_mask.any()
    yield pair
    pair.P.close()


@pytest.fixture(scope="module")
def SPH(oracle, tmp_path_factory):
    from test_gpu_materials_unbounded import sphere_records

    pair = Pair(oracle, "sphere", sphere_records(tmp_path_factory.mktemp("tan_sphere")))
    assert pair.P.nT == 1310 and pair.P.bvh_info()["accel"] == "bvh" and pair.P.lobe_mask.sum() == 1280
    yield pair
    pair.P.close()


# ------------------------------------------------------------- against the oracle, every entry
@pytest.mark.parametrize("f", OM.B_BOUNDED, ids=OM.frame_id)
def test_spec_brute_force(B, f):
    """32x32x8 at 4 bounces; spp 3 and 5 (the division branch); a seed >= 2^33; 20 bounces (paths of up to 21 tasks
    cross sweep rounds); 0 bounces (one vertex per path); a band with step 3 and a contiguous band."""
    B.run(f, 3)


@pytest.mark.parametrize("K", [1, 16])
def test_non_spec_many_emitters(GLOW, K):
    GLOW.run(OM.GLOW[0], K)


def test_spec_bvh_global_tangents(SPH):
    """1310 triangles: no LDS tables, the tangents are read from global memory by triangle; the lobe rows reach
    beyond the 512 hot slots of the adjoint's bin map, which must play no part here."""
    assert (SPH.P.lobe_mask & ~OM.hot_set(SPH.Q)).any()
    SPH.run(OM.SPHERE[0], 2)


def test_one_launch_is_k_launches(B):
    f, K = OM.B_BOUNDED[0], 3
    tang = OT.draw_tangents(B.Q, K)
    _, A = OT.reference(B.Q, "B", f, tang)
    args = (f.W, f.H, f.spp, f.mb, f.seed) + OM.frame_rows(f)
    together = B.P.tangent_materials(*tang, *args)
    for k in range(K):
        alone = B.P.tangent_materials(*[t[k] for t in tang], *args)  # (nT, 3): K = 1
        assert alone.shape == (1,) + together.shape[1:]
        assert np.all(np.abs(alone[0] - together[k]) <= 1e-12 * A[k] + 1e-15)
    # each block alone, the others NULL: the three sum to the whole
    parts = sum(B.P.tangent_materials(*[t if i == j else None for j, t in enumerate(tang)], *args) for i in range(3))
    assert np.all(np.abs(parts - together) <= 1e-12 * A + 1e-15)


def test_dot_product_identity_at_a_larger_frame(B):
    """<adj, J v> = <J^T adj, v> with the adjoint from Scene.adjoint_materials, no oracle: 64x48x8, the adjoint image
    from {0, 0.25, 0.5, 1, 2}, so adj * (1/spp) and its products with g are exact scalings of the tangent's terms."""
    W, H, spp, mb, seed, K = 64, 48, 8, 4, 21, 3
    adj = np.random.RandomState(3).choice(np.array([0, 0.25, 0.5, 1, 2], np.float32), (H, W, 3))
    tang = OT.draw_tangents(B.Q, K, seed=5)
    tan = B.P.tangent_materials(*tang, W, H, spp, mb, seed)
    A = B.P.tangent_materials(*[np.abs(t) for t in tang], W, H, spp, mb, seed)
    grad = np.stack(B.P.adjoint_materials(adj, W, H, spp, mb, seed))
    assert np.all(A >= 0) and A.max() > 0
    for k in range(K):
        lhs = float((adj.astype(np.float64) * tan[k]).sum())
        rhs = float(sum((grad[b] * tang[b][k].astype(np.float64)).sum() for b in range(3)))
        bound = 1e-9 * float((adj.astype(np.float64) * A[k]).sum()) + 1e-12
        print("dot product k=%d: %.12g vs %.12g, |d| %.2e of the bound" % (k, lhs, rhs, abs(lhs - rhs) / bound))
        assert lhs != 0 and abs(lhs - rhs) <= bound


def test_device_overrides_are_the_scenes_values(B):
    from inverse_path_tracer_amd import torch_ops

    f, K = OM.B_BOUNDED[5], 2
    args = (f.W, f.H, f.spp, f.mb, f.seed) + OM.frame_rows(f)
    tang = OT.draw_tangents(B.Q, K, seed=9)
    other = B.values[1]
    base = B.P.tangent_materials(*tang, *args)
    dev = [torch.tensor(v, device="cuda") for v in other + tang]
    over = torch_ops.tangent_materials(B.P, *dev, *args)
    assert over.dtype == torch.float64 and over.is_cuda and tuple(over.shape) == base.shape
    A = B.P.tangent_materials(*[np.abs(t) for t in tang], *args)
    try:
        B.P.set_material_params(*other)
        want = B.P.tangent_materials(*tang, *args)
        A = np.maximum(A, B.P.tangent_materials(*[np.abs(t) for t in tang], *args))
    finally:
        B.P.set_material_params(*B.values[0])
    assert np.all(np.abs(over.cpu().numpy() - want) <= 1e-12 * A + 1e-15)
    assert not np.allclose(want, base, rtol=1e-3, atol=0)  # the other values do move the tangents
    # kd alone overridden: ks and ke stay the scene's own
    kd_only = torch_ops.tangent_materials(B.P, dev[0], None, None, *dev[3:], *args).cpu().numpy()
    try:
        B.P.set_material_params(kd=other[0])
        want = B.P.tangent_materials(*tang, *args)
    finally:
        B.P.set_material_params(*B.values[0])
    assert np.all(np.abs(kd_only - want) <= 1e-12 * A + 1e-15)


# ------------------------------------------------------------- torch: forward-mode AD
def test_forward_ad_through_render_materials(B):
    import torch.autograd.forward_ad as fwAD

    from inverse_path_tracer_amd import NativeError, torch_ops

    W, H, spp, mb, seed = 24, 16, 4, 3, 6
    kd, ks, ke = (torch.tensor(v, device="cuda") for v in B.values[1])
    tkd, tks, tke = (torch.tensor(t[0], device="cuda") for t in OT.draw_tangents(B.Q, 1, seed=4))
    plain = torch_ops.render_materials(B.P, kd, ks, ke, W, H, spp, mb, seed)

    def jvp(tangents):
        with fwAD.dual_level():
            duals = [v if t is None else fwAD.make_dual(v, t) for v, t in zip((kd, ks, ke), tangents)]
            out = fwAD.unpack_dual(torch_ops.render_materials(B.P, *duals, W, H, spp, mb, seed))
            return out.primal.clone(), None if out.tangent is None else out.tangent.clone()

    img, tan = jvp((tkd, tks, tke))
    assert torch.equal(img.view(torch.int32), plain.view(torch.int32))  # the image, bit for bit
    want = torch_ops.tangent_materials(B.P, kd, ks, ke, tkd, tks, tke, W, H, spp, mb, seed)
    assert tan.dtype == torch.float32 and tan.shape == plain.shape and bool(tan.abs().max() > 0)
    assert torch.equal(tan, want[0].float())  # one launch at K = 1, cast once
    # an input without a tangent contributes nothing: only kd's direction
    _, tan_kd = jvp((tkd, None, None))
    want_kd = torch_ops.tangent_materials(B.P, kd, ks, ke, tkd, None, None, W, H, spp, mb, seed)
    assert torch.equal(tan_kd, want_kd[0].float())
    # a None input (the scene's own values) has no tangent either
    with fwAD.dual_level():
        out = fwAD.unpack_dual(torch_ops.render_materials(B.P, fwAD.make_dual(kd, tkd), None, None, W, H, spp, mb, seed))
        own = torch_ops.tangent_materials(B.P, kd, None, None, tkd, None, None, W, H, spp, mb, seed)
        assert torch.equal(out.tangent, own[0].float())
    # backward is what it was
    kd_g = kd.clone().requires_grad_(True)
    torch_ops.render_materials(B.P, kd_g, ks, ke, W, H, spp, mb, seed).sum().backward()
    assert kd_g.grad is not None and bool(kd_g.grad.abs().max() > 0)
    # the other routes have no tangent kernel and say which op has
    with fwAD.dual_level():
        with pytest.raises(NativeError, match="render_materials "):
            torch_ops.render_materials_unbounded(B.P, fwAD.make_dual(kd, tkd), ks, ke, W, H, spp, seed)
    with fwAD.dual_level():
        with pytest.raises(NativeError, match="render_materials "):
            torch_ops.render_materials_batch(B.P, fwAD.make_dual(kd[None].contiguous(), tkd[None].contiguous()), None,
                                             None, W, H, spp, mb, seed)
    v = B.P.views(B.P.camera()[None])
    try:
        with fwAD.dual_level():
            with pytest.raises(NativeError, match="render_materials "):
                torch_ops.render_views(B.P, v, fwAD.make_dual(kd, tkd), ks, ke, W, H, spp, mb, seed)
        with fwAD.dual_level():
            with pytest.raises(NativeError, match="render_materials "):
                torch_ops.render_views_batch(B.P, v, fwAD.make_dual(kd[None].contiguous(), tkd[None].contiguous()),
                                             None, None, W, H, spp, mb, seed)
        with fwAD.dual_level():
            with pytest.raises(NativeError, match="render_materials "):
                torch_ops.render_views_batch_unbounded(B.P, v, fwAD.make_dual(kd[None].contiguous(),
                                                                              tkd[None].contiguous()), None, None, W,
                                                       H, spp, seed)
    finally:
        v.close()


# ------------------------------------------------------------- Gauss-Newton
@pytest.mark.parametrize("groups", [[("kd", range(18, 30))],
                                    [("kd", range(18, 30)), ("kd", range(12, 14)), ("kd", range(14, 16))]],
                         ids=["cube", "cube+walls"])
def test_gauss_newton_recovers_tied_kd(groups):
    """scenes/0 at 16x16x8, 3 bounces, seed 4; the target is the render at the loaded Kd with the same seed, so the
    residual is exactly 0 at the truth (material values do not move the paths).  Start 0.5; after 4 steps
    max|Kd - truth| <= 1e-5 (the oracle's own Gauss-Newton reaches 2.7e-8 and 6.0e-8)."""
    from inverse_path_tracer_amd import optimize

    W = H = 16
    spp, mb, seed = 8, 3, 4
    P = product_scene(SCENE0)
    try:
        truth = P.materials.copy()
        target = P.render(W, H, spp, mb, seed)
        start = truth.copy()
        for _, rows in groups:
            start[list(rows)] = 0.5
        P.materials = start
        hist = optimize.gauss_newton_materials(P, target, groups, W, H, spp, mb, seed, steps=4)
        assert hist.shape == (4, len(groups), 3)
        assert np.array_equal(P.materials, start)  # the scene's own values are not changed
        errs = [max(float(np.abs(hist[s, k] - truth[list(rows)]).max()) for k, (_, rows) in enumerate(groups))
                for s in range(4)]
        print("Gauss-Newton max|Kd - truth| after steps 1..4:", " ".join("%.2e" % e for e in errs))
        assert errs[-1] <= 1e-5
    finally:
        P.close()


# ------------------------------------------------------------- the stream after a refusal
def test_launch_after_a_refused_call_on_the_same_stream(B):
    from inverse_path_tracer_amd import NativeError, torch_ops

    f = OM.B_BOUNDED[3]
    args = (f.W, f.H, f.spp, f.mb, f.seed) + OM.frame_rows(f)
    tang = OT.draw_tangents(B.Q, 1)
    T, A = OT.reference(B.Q, "B", f, tang)
    dev = [torch.tensor(t, device="cuda") for t in tang]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with pytest.raises(NativeError, match="n_tangents must be in 1..16"):
            torch_ops.tangent_materials(B.P, None, None, None, *[t.expand(17, -1, -1).contiguous() for t in dev], *args)
        with pytest.raises(NativeError, match="max_bounces in 0..62"):
            torch_ops.tangent_materials(B.P, None, None, None, *dev, f.W, f.H, f.spp, None, f.seed)
        got = torch_ops.tangent_materials(B.P, None, None, None, *dev, *args)
    st.synchronize()
    OT.compare(got.cpu().numpy(), T, A, tag="after a refusal")
