"""Every instance of the material adjoint against the CPU oracle's material adjoint, entry by entry
(run with -m gpu).

OracleScene.adjoint_materials forms the kernels' fp32 products in the kernels' order (pinned on the CPU by
tests/test_oracle_materials.py), so all three blocks -- not only Kd -- meet the Kd block's bar: rtol 1e-9,
atol 1e-12, every entry, exact zeros staying exact zeros.  The values are per-triangle distinct (RandomState(5)),
so a term credited to a neighbouring emitter or lobe triangle, or a value read from one, shows; one lobe
triangle carries Ks = 0 and one triangle of each emitter object Ke = 0 (§13.1: they keep their gradient rows).
The forward is compared bit for bit in every case: per-triangle values and zero rows are new to it as well.

Instances: SPEC brute force bounded and unbounded (scene B, values through set_material_params; the unbounded
one at the default ring and at the tiny rings, under which long paths replay), the non-SPEC many-emitter
instance (the emissive cube), SPEC x BVH with the hot-set bin map and the straight-to-global Ks path (the Phong
sphere; its unbounded frame has paths longer than the bounded kernel can record), and the scene batch with
device overrides.  The frames, the values and the coverage conditions live in tests/test_oracle_materials.py,
which has already checked the reference's own summation-order noise (<= 1e-11) and the coverage on the CPU.
"""
import numpy as np
import pytest

import test_oracle_materials as OM
from conftest import product_scene
from test_gpu_materials import bits, scene_b
from test_gpu_materials_batch import adjoint_batch, render_batch
from test_gpu_materials_unbounded import RINGS, ring, sphere_records

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


class Instance:
    """A scene in the product and in the oracle under the same drawn values, and the oracle's results per frame."""

    def __init__(self, oracle, name, records):
        self.oracle, self.name = oracle, name
        self.P, self.Q = product_scene(records), oracle.OracleScene(records)
        assert np.array_equal(self.P.lobe_mask, self.Q.lobe_mask)
        assert np.array_equal(self.P.emitter_mask, self.Q.emitter_mask)
        self.sets = OM.draw_values(self.Q, OM.N_SETS)  # masked rows carry junk: both setters must drop it
        self.zl, self.ze = OM.zero_rows(self.Q)
        self.P.set_material_params(*self.sets[0])
        self.Q.set_material_params(*self.sets[0])
        for got, want in zip(self.P.material_params()[:3], self.Q.material_params()):
            assert np.array_equal(bits(got), bits(want))
        self.refs = {}

    def reference(self, f, b=0):
        """(3 blocks, stats, samples) of frame f under set b, at seed + b * one frame of samples; computed once."""
        if (f, b) not in self.refs:
            stride = f.W * f.H * f.spp
            self.Q.set_material_params(*self.sets[b])
            *g, stats = OM.reference(self.Q, f, b, stride)
            g = np.stack(g)
            zeroed = [None if self.zl is None else g[1][self.zl]] + [g[2][e] for e in self.ze]
            OM.check_coverage(self.Q, f, stats, g[1], zeroed, sphere=self.name == "sphere")
            s, _ = self.Q.render_samples(f.W, f.H, f.spp, f.mb, f.seed + b * stride)
            rb, re, step = OM.frame_rows(f)
            s = s.reshape(f.H, f.W * f.spp, 3)[rb:re:step]
            self.Q.set_material_params(*self.sets[0])
            g.setflags(write=False)
            self.refs[(f, b)] = (g, stats, s)
        return self.refs[(f, b)]

    def compare(self, f, got, b=0, tag=""):
        want, stats, _ = self.reference(f, b)
        lobe, emit = self.P.lobe_mask, self.P.emitter_mask
        assert np.all(got[1][~lobe] == 0) and np.all(got[2][~emit] == 0)
        diffs = [OM.rel_diff(g, w) for g, w in zip(got, want)]
        print("GPU/oracle %s %s%s set %d: Kd %.2e Ks %.2e Ke %.2e (longest path %d)" %
              (self.name, OM.frame_id(f), tag, b, diffs[0], diffs[1], diffs[2], stats["longest"]))
        for blk, g, w in zip(("Kd", "Ks", "Ke"), got, want):
            np.testing.assert_allclose(g, w, rtol=OM.RTOL, atol=OM.ATOL, err_msg=blk)
            assert np.array_equal(g == 0, w == 0), blk
        assert np.any(want[0] != 0) and np.any(want[2] != 0) and (np.any(want[1] != 0) or not lobe.any())

    def forward(self, f):
        got = self.P.render_samples(f.W, f.H, f.spp, f.mb, f.seed, *OM.frame_rows(f))
        assert np.array_equal(bits(got), bits(self.reference(f)[2].reshape(-1, 3))), "the forward differs"

    def close(self):
        self.P.close()


@pytest.fixture(scope="module")
def B(oracle, tmp_path_factory):
    inst = Instance(oracle, "B", scene_b(tmp_path_factory.mktemp("mo_b")))
    assert inst.P.nT == 42 and inst.P.nE == 14 and inst.P.lobe_mask.sum() == 12
    yield inst
    inst.close()


@pytest.fixture(scope="module")
def GLOW(oracle, tmp_path_factory):
    inst = Instance(oracle, "glow", OM.glow_records(tmp_path_factory.mktemp("mo_glow")))
    assert inst.P.nT == 30 and inst.P.nE == 14 and not inst.P.lobe_mask.any()
    yield inst
    inst.close()


@pytest.fixture(scope="module")
def SPH(oracle, tmp_path_factory):
    inst = Instance(oracle, "sphere", sphere_records(tmp_path_factory.mktemp("mo_sphere")))
    assert inst.P.nT == 1310 and inst.P.bvh_info()["accel"] == "bvh" and inst.P.lobe_mask.sum() == 1280
    ks = inst.P.material_params()[1][inst.P.lobe_mask]
    assert len(np.unique(ks, axis=0)) == 1280  # 1279 drawn rows and the zero row
    yield inst
    inst.close()


def run_bounded(inst, f):
    inst.forward(f)
    inst.compare(f, np.stack(inst.P.adjoint_materials(OM.frame_adj(f), f.W, f.H, f.spp, f.mb, f.seed,
                                                      *OM.frame_rows(f))))


def run_unbounded(inst, f, size):
    inst.forward(f)
    with ring(size):
        got = np.stack(inst.P.adjoint_materials_unbounded(OM.frame_adj(f), f.W, f.H, f.spp, f.seed, *OM.frame_rows(f)))
    inst.compare(f, got, tag=" ring %s" % (size,))


# ------------------------------------------------------------- SPEC, brute force
@pytest.mark.parametrize("f", OM.B_BOUNDED, ids=OM.frame_id)
def test_spec_bounded(B, f):
    run_bounded(B, f)


@pytest.mark.parametrize("size", RINGS, ids=str)
@pytest.mark.parametrize("f", OM.B_UNBOUNDED, ids=OM.frame_id)
def test_spec_unbounded(B, f, size):
    run_unbounded(B, f, size)


# ------------------------------------------------------------- non-SPEC, many emitters
def test_non_spec_many_emitters_bounded(GLOW):
    run_bounded(GLOW, OM.GLOW[0])
    assert np.all(GLOW.reference(OM.GLOW[0])[0][1] == 0)  # the Ks block is exactly 0 (compare() held the GPU to it)


@pytest.mark.parametrize("size", RINGS, ids=str)
def test_non_spec_many_emitters_unbounded(GLOW, size):
    run_unbounded(GLOW, OM.GLOW[1], size)
    assert np.all(GLOW.reference(OM.GLOW[1])[0][1] == 0)


# ------------------------------------------------------------- SPEC x BVH: hot-set bins and global Ks
@pytest.mark.parametrize("f", [OM.SPHERE[0], OM.SPHERE_WIDE[0]], ids=OM.frame_id)
def test_spec_bvh_bounded(SPH, f):
    run_bounded(SPH, f)


@pytest.mark.parametrize("size", [None, (1, 1)], ids=str)
@pytest.mark.parametrize("f", [OM.SPHERE[1], OM.SPHERE_WIDE[1]], ids=OM.frame_id)
def test_spec_bvh_unbounded(SPH, f, size):
    """The 32x24x8 frame has paths of 37 vertices, more than trace_mat_kernel can record on this scene (24
    bounces): the case the bounded-against-unbounded comparison of §16.4 had to leave out."""
    run_unbounded(SPH, f, size)
    assert SPH.reference(f)[1]["longest"] > 25


# ------------------------------------------------------------- the scene batch, device overrides
def run_batch(inst, f):
    from inverse_path_tracer_amd import _native as N

    S, stride = OM.N_SETS, f.W * f.H * f.spp
    kd, ks, ke = (np.stack([s[i] for s in inst.sets]) for i in range(3))
    for a, m in ((kd, np.ones(inst.P.nT, bool)), (ks, inst.P.lobe_mask), (ke, inst.P.emitter_mask)):
        rows = a[:, m].reshape(-1, 3)
        rows = rows[np.any(rows != 0, axis=1)]  # all but the zero-valued rows: distinct within and across the sets
        assert len(np.unique(rows, axis=0)) == len(rows) >= S * (m.sum() - 2)
    adj = np.stack([OM.frame_adj(f, b) for b in range(S)])
    rb, re, step = OM.frame_rows(f)
    p = N.make_params(f.W, f.H, f.spp, f.mb, f.seed, rb, re, step)
    hb = render_batch(inst.P, kd, ks, ke, p, S, stride)
    gb = adjoint_batch(inst.P, kd, ks, ke, adj, p, S, stride)
    for b in range(S):
        _, _, s = inst.reference(f, b)
        hdr = inst.oracle.pixel_mean(s.reshape(-1, 3), s.shape[0] * f.W, f.spp)[0]
        assert np.array_equal(bits(hb[b].reshape(-1, 3)), bits(hdr)), "the forward of set %d differs" % b
        inst.compare(f, gb[b], b, tag=" batch")
    # the batch launches leave the scene's own tables alone
    inst.forward(f)


@pytest.mark.parametrize("f", OM.BATCH_B, ids=OM.frame_id)
def test_scene_batch_spec(B, f):
    run_batch(B, f)


def test_scene_batch_non_spec(GLOW):
    run_batch(GLOW, OM.BATCH_GLOW[0])
