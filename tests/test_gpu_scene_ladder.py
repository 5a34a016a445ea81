"""Every kernel-instance boundary on generated mid-size scenes (run with -m gpu; tests/scene_ladder.py).

The host picks another kernel instance or LDS layout at 32/33 triangles, 16/17 emitters, 39/40 triangles (graph),
63/64 (brute force / BVH), 512/513 (Kd and tangent tables, gradient bins) and 128 wide BVH nodes.  Each rung of
scene_ladder.RUNGS sits on one side of such a switch; each case first asserts, from ipt_debug_last_launch, that the
launch took the path the rung is there for, and then compares with the CPU oracle at the bars the suite uses for the
same quantities: samples and the fused frame bit for bit, fp64 sums at rtol 1e-9 / atol 1e-12, the graph's compressed
floats at rtol 1e-6 / atol 1e-7, the material blocks and the tangents at their modules' bars (test_oracle_materials.py,
test_oracle_tangent.py), BVH casts bit for bit against the brute-force loop.

One product/oracle pair per rung, loaded once.  The forward, the Kd adjoint and the graph run under the scenes' own
values, the material adjoint and the tangents under OM.draw_values; tests/test_scene_ladder.py has checked on the CPU
that every (rung, frame) used here lights the scene and reaches its glow and shiny rows.
"""
import contextlib

import numpy as np
import pytest

import scene_ladder as SL
import test_oracle_materials as OM
import test_oracle_tangent as OT
from test_gpu_materials_oracle import Instance, run_batch, run_bounded, run_unbounded
from test_gpu_shade_tables import bits, check_forward

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


CU_LDS = 160 * 1024
# Resident workgroups per CU that the registers allow (256 lanes a workgroup; tests/test_oracle_tangent.py and the
# code-object test pin the counts): the BVH forwards hold 96 VGPRs, five waves per SIMD; every other BVH instance
# (adjoint, graph, material adjoint, tangents) 105..128, four.  The brute-force bounded adjoint: 96, five.
CAP_FORWARD, CAP_OTHER = 5, 4


def bvh_pick(rec, wide, big_pairs, cap):
    """launch_bvh_pick (ipt_hip.hip) from a launch's record: of (tree staged, large pairs copied) in the order
    (1, 1), (1, 0), (0, 1), (0, 0), the first with the most resident workgroups per CU, min(cap, 160 KiB / bytes).
    Returns (wide nodes in LDS, pairs copied) as the record must show them."""
    stage = wide * 256 if wide <= SL.WIDE_LDS_NODES else 0  # WideNode; a tree past 32 KiB is never staged
    copy = 12 + big_pairs * (144 + 8) if big_pairs else 0   # big_lds_bytes: TriPair + two indices per pair
    bare = rec["lds_bytes"] - (stage if rec["bvh_wide_lds"] else 0) - (copy if rec["bvh_big_lds"] else 0)
    best = None
    for s, b in ((1, 1), (1, 0), (0, 1), (0, 0)):
        n = bare + s * stage + b * copy
        per_cu = min(cap, CU_LDS // n) if n <= CU_LDS else 0
        if best is None or per_cu > best[0]:
            best = (per_cu, wide if s and stage else 0, b)
    return best[1], best[2]


def shade_kind(rec, r, cap):
    """launch<> (ipt_hip.hip): a brute-force scene of at most 32 triangles and 16 emitters runs the instance with
    the shading tables in LDS (KIND 7) unless their bytes cost a resident workgroup (shade_keeps_residency)."""
    if not (r.nT <= 32 and 0 < r.nE <= 16):
        return SL.KIND_TRACE
    tables = ((16 + (r.nT + 1) * 17 + r.nE * 21 + 3) & ~3) * 4  # shade_table_words (scene_layout.h)
    bare = rec["lds_bytes"] - (tables if rec["kind"] == SL.KIND_SHADE else 0)
    keeps = bare + tables <= CU_LDS and min(cap, CU_LDS // (bare + tables)) >= min(cap, CU_LDS // bare)
    return SL.KIND_SHADE if keeps else SL.KIND_TRACE


class Rung(Instance):
    """Instance (product + oracle under the drawn values, references cached) that can run under its own values."""

    def __init__(self, oracle, name, records):
        self.own = oracle.OracleScene(records).material_params()
        super().__init__(oracle, "ladder:" + name, records)
        self.rung, self.r = name, SL.RUNGS[name]
        self.info = self.P.bvh_info()
        assert (self.P.nT, self.P.nE, int(self.P.lobe_mask.sum())) == (self.r.nT, self.r.nE, self.r.lobes)

    @contextlib.contextmanager
    def own_values(self):
        for S in (self.P, self.Q):
            S.set_material_params(*self.own)
        try:
            yield
        finally:
            for S in (self.P, self.Q):
                S.set_material_params(*self.sets[0])

    def launched(self, what, call, cap=CAP_OTHER, **want):
        """Runs call(), which must launch; checks the launch's record against the rung and `want`.  cap: the resident
        workgroups per CU that the instance's registers allow, for the BVH instances' choice of LDS extras."""
        before = SL.last_launch()["launches"]
        out = call()
        rec = SL.last_launch()
        print("LAUNCH %s %s: %s" % (self.rung, what, {k: v for k, v in rec.items() if k != "launches"}))
        assert rec["launches"] > before, "nothing was launched"
        r, bvh = self.r, self.r.nT >= SL.BVH_MIN_TRIS
        assert (rec["nT"], rec["nE"]) == (r.nT, r.nE)
        assert rec["bvh"] == int(bvh) == int(self.info["accel"] == "bvh")
        assert rec["spec"] == int(r.lobes > 0)
        assert rec["small_pairs"] & 1 == int(r.nT <= 32)
        assert rec["emit_lds"] == int(bvh and r.nE <= 16)
        if not bvh:
            assert rec["bvh_wide_lds"] == 0 and rec["bvh_big_lds"] == 0
        else:  # the tree staged whole where that costs no resident workgroup, and never past 32 KiB
            staged, copied = bvh_pick(rec, self.info["wide_nodes"], self.info["big_pairs"], cap)
            assert (rec["bvh_wide_lds"], rec["bvh_big_lds"]) == (staged, copied), (rec, staged, copied)
            assert staged == 0 or staged == self.info["wide_nodes"] <= SL.WIDE_LDS_NODES
        assert 0 <= rec["lds_bytes"] <= 160 * 1024 and rec["grid"] > 0  # (a graph launch with its bins in global memory has none)
        for k, v in want.items():
            assert rec[k] in v if isinstance(v, tuple) else rec[k] == v, (k, rec[k], v)
        return out


@pytest.fixture(scope="module")
def rungs(oracle, tmp_path_factory):
    tmp, made = tmp_path_factory.mktemp("gpu_ladder"), {}

    def get(name):
        if name not in made:
            made[name] = Rung(oracle, name, SL.records(tmp, name))
        return made[name]

    yield get
    for inst in made.values():
        inst.close()


def _frame_id(c):
    (W, H, spp, mb, seed), rows = c
    return "%dx%dx%d-mb%s%s" % (W, H, spp, mb, "" if rows is None else "-rows%d:%d:%d" % rows)


CASES = [(n, c) for n in SL.GPU_RUNGS for c in SL.frames(n)]
CASE_IDS = ["%s-%s" % (n, _frame_id(c)) for n, c in CASES]


def kd_tables(r):
    return int(r.nT <= SL.KD_TABLE_TRIS)


def fused(spp, mb, bvh):
    """fused_shape (ipt_hip.hip): whether Scene.render fuses the pixel mean into the trace launch -- brute-force
    scenes whose ring of 6 KiB per wave holds two groups of pixels (four with long paths) of at least 32 samples."""
    if bvh:
        return False
    cap = min(16, 6144 // (12 * spp)) // (4 if mb is None or mb > 8 else 2)
    g = 1
    while 2 * g <= cap and 2 * g * spp <= 256:
        g *= 2
    return cap >= 1 and g * spp >= 32


# ------------------------------------------------------------- forward
@pytest.mark.parametrize("name,case", CASES, ids=CASE_IDS)
def test_forward_and_fused_equal_oracle(rungs, oracle, name, case):
    inst = rungs(name)
    (W, H, spp, mb, seed), rows = case
    P, Q, r = inst.P, inst.Q, inst.r
    shade = r.nT <= 32 and r.nE <= 16  # the shading tables: a forward's few KiB of LDS always keep their residency
    kind = SL.KIND_SHADE if shade else SL.KIND_TRACE
    # a forward's LDS is small: every tree of the rungs up to 513 triangles (at most 27 nodes, 6.8 KiB) is staged;
    # the tree rungs' is not -- 105 nodes cost the fifth workgroup, 150 do not fit the stage
    staged = {"bvh_wide_lds": inst.info["wide_nodes"] if 64 <= r.nT <= 513 else 0}
    with inst.own_values():
        rb, re_, step = rows or (0, H, 1)
        got = inst.launched("forward", lambda: P.render_samples(W, H, spp, mb, seed, rb, re_, step), cap=CAP_FORWARD,
                            mode=SL.MODE_FWD, kind=kind, kd_tables=kd_tables(r), small_pairs=3 if shade else int(r.nT <= 32), **staged)
        mode = SL.MODE_FWDM if fused(spp, mb, r.nT >= SL.BVH_MIN_TRIS) else SL.MODE_FWD
        assert (mode == SL.MODE_FWDM) == (r.nT < SL.BVH_MIN_TRIS and (W, H, spp, mb, seed) == SL.FRAME_4)
        hdr = inst.launched("render", lambda: P.render(W, H, spp, mb, seed, rb, re_, row_step=step), cap=CAP_FORWARD,
                            mode=mode, kind=kind, kd_tables=kd_tables(r), **staged)
        if rows is None:
            check_forward(oracle, P, Q, W, H, spp, mb, seed)
        want, _ = Q.render_samples(W, H, spp, mb, seed)
        want = want.reshape(H, W * spp, 3)[rb:re_:step].reshape(-1, 3)
        assert np.array_equal(bits(got), bits(want))
        hq, _ = oracle.pixel_mean(want, want.shape[0] // spp, spp)
        assert np.array_equal(bits(hdr.reshape(-1, 3)), bits(hq))


# ------------------------------------------------------------- Kd adjoint, bounded and unbounded
@pytest.mark.parametrize("name,case", CASES, ids=CASE_IDS)
def test_kd_adjoint_equals_oracle(rungs, name, case):
    inst = rungs(name)
    (W, H, spp, mb, seed), rows = case
    P, Q, r = inst.P, inst.Q, inst.r
    rb, re_, step = rows or (0, H, 1)
    adj = OM.frame_adj(OM.F(W, H, spp, mb, seed))
    want = dict(kd_tables=kd_tables(r), grad_slots=min(r.nT, 512))
    if mb is None:
        want.update(mode=SL.MODE_ADJU, kind=SL.KIND_TRACE)
    else:  # (the six-wave instance is for launches of 8 M samples and more: IPT_ADJW_MIN_SAMPLES)
        want.update(mode=SL.MODE_ADJ, rec_cap=mb + 1)
    if mb == 20 and name in SL.TREE_RUNGS:
        # 21 records per lane: one workgroup per CU with or without the nodes, so the 105-node tree is staged
        want.update(bvh_wide_lds=inst.info["wide_nodes"] if name == "tree-fits" else 0)
        assert (inst.info["wide_nodes"] <= SL.WIDE_LDS_NODES) == (name == "tree-fits")
    with inst.own_values():
        got = inst.launched("Kd adjoint", lambda: P.adjoint(adj, W, H, spp, mb, seed, rb, re_, step), **want)
        rec = SL.last_launch()
        if mb is None:
            assert rec["rec_lds"] >= 1
        else:  # the shading tables: where the scene fits them and they cost no workgroup, and nowhere else
            assert rec["kind"] == shade_kind(rec, r, 5 if r.nT < SL.BVH_MIN_TRIS else CAP_OTHER)
            assert r.nT <= 32 and r.nE <= 16 or rec["kind"] == SL.KIND_TRACE
        if step == 1:
            ref = Q.adjoint(W, H, spp, mb, seed, adj, rb, re_)
        else:  # (the oracle's Kd block over an interleaved band is its material adjoint's, bit for bit)
            ref = Q.adjoint_materials(W, H, spp, mb, seed, adj, rb, re_, step)[0]
    assert np.mean(np.any(ref != 0, axis=1)) >= 0.4
    np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-12)
    assert np.array_equal(got == 0, ref == 0)


# ------------------------------------------------------------- graph
@pytest.mark.parametrize("name", SL.GRAPH_RUNGS)
def test_graph_equals_oracle(rungs, name):
    inst = rungs(name)
    P, Q, r = inst.P, inst.Q, inst.r
    W, H, spp, mb, seed = SL.FRAME_4
    tgt = np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
    in_lds = ((r.nT + 1) * r.nT * 5 + (r.nT + 1) * r.nE * 3) * 8 <= 64 * 1024  # graph_lds_doubles (ipt_hip.hip)
    assert in_lds == (name == "39-2-0")
    with inst.own_values():
        acc, data = inst.launched("graph", lambda: P.graph(tgt, W, H, spp, mb, seed), mode=SL.MODE_GRAPH,
                                  kind=SL.KIND_TRACE, lds_edges=int(in_lds), kd_tables=0)
        acc_q, data_q = Q.graph(W, H, spp, mb, seed, tgt)
    assert np.count_nonzero(acc_q) > 0
    np.testing.assert_allclose(acc, acc_q, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(data, data_q, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------- material adjoint (Kd, Ks, Ke) under drawn values
def _mat_launch(inst, mode):
    rec = SL.last_launch()
    print("LAUNCH %s material adjoint: %s" % (inst.rung, rec))
    assert (rec["mode"], rec["kind"], rec["nT"]) == (mode, SL.KIND_MATG, inst.r.nT)
    assert rec["spec"] == int(inst.r.lobes > 0) and rec["bvh"] == int(inst.r.nT >= SL.BVH_MIN_TRIS)
    assert rec["kd_tables"] == kd_tables(inst.r) and rec["grad_slots"] == min(inst.r.nT, 512)
    assert rec["emit_lds"] == int(rec["bvh"] and inst.r.nE <= 16)
    if rec["bvh"]:
        assert (rec["bvh_wide_lds"], rec["bvh_big_lds"]) == bvh_pick(rec, inst.info["wide_nodes"], inst.info["big_pairs"],
                                                                  CAP_OTHER)


@pytest.mark.parametrize("name", SL.MAT_RUNGS)
def test_material_adjoint_bounded(rungs, name):
    inst = rungs(name)
    before = SL.last_launch()["launches"]
    run_bounded(inst, OM.LADDER[name][0])
    assert SL.last_launch()["launches"] > before
    _mat_launch(inst, SL.MODE_ADJ)


@pytest.mark.parametrize("name", SL.MAT_RUNGS)
def test_material_adjoint_unbounded(rungs, name):
    inst = rungs(name)
    before = SL.last_launch()["launches"]
    run_unbounded(inst, OM.LADDER[name][1], None)
    assert SL.last_launch()["launches"] > before
    _mat_launch(inst, SL.MODE_ADJU)
    assert inst.reference(OM.LADDER[name][1])[1]["longest"] >= OM.LONG


@pytest.mark.parametrize("name", SL.MAT_BATCH_RUNGS)
def test_material_adjoint_batch_of_three(rungs, name):
    run_batch(rungs(name), OM.LADDER[name][0])


# ------------------------------------------------------------- tangents
@pytest.mark.parametrize("name", list(SL.TANGENTS))
def test_tangents(rungs, name):
    """K tangent images against the oracle; where the tangent tables live is the host's choice:
    LDS up to 512 triangles while they fit beside the vertex records -- K = 16 at 300 triangles and 2 bounces still
    does --, global memory past 512 triangles and for K = 16 at 512 triangles, which no LDS holds."""
    inst = rungs(name)
    K, _, in_lds = SL.TANGENTS[name]
    f = OM.LADDER_TAN[name]
    tang = OT.draw_tangents(inst.Q, K)
    got = inst.launched("tangents K=%d" % K,
                        lambda: inst.P.tangent_materials(*tang, f.W, f.H, f.spp, f.mb, f.seed, *OM.frame_rows(f)),
                        mode=SL.MODE_ADJ, kind=SL.KIND_TANG, kd_tables=in_lds, rec_cap=f.mb + 1)
    T, A = OT.reference(inst.Q, inst.name, f, tang)
    OT.compare(got, T, A, tag="%s %s K=%d" % (inst.name, OM.frame_id(f), K))


# ------------------------------------------------------------- BVH casts == the brute-force loop == the oracle
@pytest.mark.parametrize("name", SL.RAY_RUNGS)
def test_bvh_closest_hit_equals_brute_force(rungs, name):
    from inverse_path_tracer_amd import _native as N
    from test_gpu import _rays

    inst = rungs(name)
    P, Q = inst.P, inst.Q
    assert inst.info["accel"] == "bvh"
    O, D = _rays(P, 8000, 100000, 3 + inst.r.nT)
    try:
        P.set_accel(N.ACCEL_BVH)
        tb, ib = P.closest_hit(O, D)
        P.set_accel(N.ACCEL_BRUTE)
        tf, i_f = P.closest_hit(O, D)
    finally:
        P.set_accel(N.ACCEL_AUTO)
    assert np.array_equal(ib, i_f)
    assert np.array_equal(bits(tb), bits(tf))
    assert (ib >= 0).mean() > 0.5 and (ib >= 18).mean() > 0.1  # the shards are hit, not only the walls
    tq, iq = Q.closest_hit(O[:20000], D[:20000])
    assert np.array_equal(iq, ib[:20000])
    hit = iq >= 0
    assert np.array_equal(bits(tq[hit]), bits(tb[:20000][hit]))
