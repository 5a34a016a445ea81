"""The generated scenes of tests/scene_ladder.py without a GPU: the generator, the host's choice of acceleration
structure on every rung, the tangent launch's LDS limit on host-only scenes, ipt_debug_last_launch as declared and
bound, and the REFERENCE-ONLY conditions of every (rung, frame) that tests/test_gpu_scene_ladder.py compares -- from
the oracle alone, under the values the GPU module runs (OM.draw_values, set 0):

    at least 0.25 of the samples are non-black,
    at least 0.4 of the Kd gradient rows are non-zero,
    at least half of the glow rows have a non-zero Ke gradient, half of the shiny rows a non-zero Ks gradient
    (on the material adjoint's frames).

These are conditions on the scenes, not tolerances: a rung that misses one gets another seed or shard size in
scene_ladder.RUNGS.  (The thread-order noise of the reference on the material and tangent frames is checked by
test_oracle_materials.py::test_gpu_frames_noise_and_coverage, the tangent coverage by test_oracle_tangent.py.)
"""
import ctypes as C
import filecmp
import re

import numpy as np
import pytest

import scene_ladder as SL
import test_oracle_materials as OM
from conftest import product_scene

MIN_SAMPLES, MIN_KD_ROWS, MIN_KE_ROWS, MIN_KS_ROWS = 0.25, 0.4, 0.5, 0.5


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("scene_ladder")


@pytest.fixture(scope="module")
def hosts(tmp):
    """name -> host-only product scene, loaded once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = product_scene(SL.records(tmp, name), device=False)
        return made[name]

    yield get
    for P in made.values():
        P.close()


@pytest.fixture(scope="module")
def oracles(oracle, tmp):
    """name -> oracle scene under OM.draw_values' first set, loaded once."""
    made = {}

    def get(name):
        if name not in made:
            Q = oracle.OracleScene(SL.records(tmp, name))
            Q.set_material_params(*OM.draw_values(Q, 1)[0])
            made[name] = Q
        return made[name]

    return get


# ------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("name", list(SL.RUNGS))
def test_generator(oracle, hosts, tmp, tmp_path, name):
    r = SL.RUNGS[name]
    P, Q = hosts(name), oracle.OracleScene(SL.records(tmp, name))
    for S in (P, Q):
        assert (S.nT, S.nE, int(S.lobe_mask.sum())) == (r.nT, r.nE, r.lobes)
        assert S.emitter_mask[18:18 + r.nE - 2].all() and S.emitter_mask.sum() == r.nE
        assert S.lobe_mask[16 + r.nE:16 + r.nE + r.lobes].all()
    assert np.array_equal(P.triangles().view(np.uint32), Q.triangles().view(np.uint32))
    again = SL.records(tmp_path, name)
    for a, b in zip(SL.records(tmp, name)[1][3:5], again[1][3:5]):
        assert filecmp.cmp(a, b, shallow=False)
    # free-floating: every shard has its own three vertices, inside the box (centre + 2/3 of the longest edges)
    v = P.triangles()[18:, 0:9].reshape(-1, 3)
    assert len(np.unique(v, axis=0)) == 3 * (r.nT - 18)
    reach = 2.0 / 3.0 * 2 * r.size[1]
    assert np.all(v >= np.array(SL.BOX_LO) - reach) and np.all(v <= np.array(SL.BOX_HI) + reach)


# ------------------------------------------------------------------ 2. what the host selects
@pytest.mark.parametrize("name", list(SL.RUNGS))
def test_selection(hosts, name):
    info = hosts(name).bvh_info()
    assert info["status"] == "ok" and info["has_bvh"]
    assert info["accel"] == ("bvh" if SL.RUNGS[name].nT >= SL.BVH_MIN_TRIS else "brute")
    if name == "tree-fits":
        assert 64 < info["wide_nodes"] <= SL.WIDE_LDS_NODES
    elif name == "tree-global":
        assert info["wide_nodes"] > SL.WIDE_LDS_NODES
    else:
        assert info["wide_nodes"] <= SL.WIDE_LDS_NODES


def test_last_launch_is_declared_exported_and_bound():
    from inverse_path_tracer_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+ipt_debug_last_launch\s*\(\s*int32_t\s*\*out\s*,\s*int\s+n\s*\)\s*;", header)
    assert hasattr(C.CDLL(N.LIB_PATH), "ipt_debug_last_launch")
    assert N.lib().ipt_abi_version() == 6 == N.ABI_VERSION
    L = N.lib()
    n = len(SL.LAUNCH_FIELDS)
    assert L.ipt_debug_last_launch(None, 0) == n and L.ipt_debug_last_launch(None, n) == n
    out = (C.c_int32 * (n + 2))(*([-7] * (n + 2)))
    assert L.ipt_debug_last_launch(out, 3) == n and list(out[3:]) == [-7] * (n - 1)  # only the first 3 are written
    assert L.ipt_debug_last_launch(out, n + 2) == n and list(out[n:]) == [-7, -7]    # never more than there are
    assert SL.last_launch()["launches"] >= 0


# ------------------------------------------------------------------ 3. the tangent launch's limits
@pytest.mark.parametrize("mb", [4, 20])
@pytest.mark.parametrize("name", ["300-22-100", "512-8-256", "450-2-300"])
def test_tangent_launch_is_not_refused_for_being_small(hosts, name, mb):
    """The documented contract is K <= 16.  A host-only scene meets every refusal of the call and reports itself last,
    so "host-only" means that every other check passed.  Up to 512 triangles the tangents are staged in LDS beside
    the Kd tables; where K x (2 nT + nE) x 3 floats do not fit beside the vertex records the launch reads them from
    global memory, as every scene past 512 triangles does -- it is not refused."""
    from inverse_path_tracer_amd import _native as N

    P = hosts(name)
    L = N.lib()
    par = N.make_params(8, 8, 2, mb)
    t = np.ones((16, P.nT, 3), np.float32)
    out = np.zeros((16, 8, 8, 3))
    tp, tf = t.ctypes.data, t.ctypes.data_as(N.fp)
    for K in (1, 8, 12, 16):
        for call in (lambda: L.ipt_tangent_mat_dev(P.handle, C.byref(par), None, None, None, K, tp, tp, tp,
                                                   out.ctypes.data, None),
                     lambda: L.ipt_tangent_mat_host(P.handle, C.byref(par), K, tf, tf, tf, out.ctypes.data_as(N.dp))):
            L.ipt_clear_error()
            rc, err = call(), N.last_error()
            L.ipt_clear_error()
            assert rc == -1 and "host-only" in err and "LDS" not in err, (name, mb, K, err)
    assert np.all(out == 0)


def test_tangent_launch_still_refuses_what_fits_nowhere(hosts):
    """62 bounces: 63 records x 5 fields x 256 lanes x 4 B of LDS alone -- the tangents' memory does not matter."""
    from inverse_path_tracer_amd import _native as N

    P = hosts("300-22-100")
    t = np.ones((1, P.nT, 3), np.float32)
    out = np.zeros((1, 8, 8, 3))
    par = N.make_params(8, 8, 2, 62)
    assert N.lib().ipt_tangent_mat_host(P.handle, C.byref(par), 1, t.ctypes.data_as(N.fp), None, None,
                                        out.ctypes.data_as(N.dp)) == -1
    assert "LDS footprint" in N.last_error()
    N.lib().ipt_clear_error()


# ------------------------------------------------------------------ 4. the reference on the GPU module's frames
def _cases():
    for name in SL.GPU_RUNGS:
        for frame, rows in SL.frames(name):
            yield name, frame, rows


def _id(c):
    name, (W, H, spp, mb, seed), rows = c[:3]
    return "%s-%dx%dx%d-mb%s%s" % (name, W, H, spp, mb, "" if not rows else "-rows%d:%d:%d" % rows)


@pytest.mark.parametrize("case", list(_cases()), ids=_id)
def test_reference_reaches_the_scene(oracle, tmp, case):
    """The frames of the forward and the Kd adjoint, under the scene's own values."""
    name, (W, H, spp, mb, seed), rows = case
    Q = oracle.OracleScene(SL.records(tmp, name))
    rb, re_, step = rows or (0, H, 1)
    s, _ = Q.render_samples(W, H, spp, mb, seed)
    s = s.reshape(H, W * spp, 3)[rb:re_:step].reshape(-1, 3)
    lit = float(np.any(s != 0, axis=1).mean())
    g = Q.adjoint(W, H, spp, mb, seed, OM.frame_adj(OM.F(W, H, spp, mb, seed)), rb, re_) if step == 1 else \
        Q.adjoint_materials(W, H, spp, mb, seed, OM.frame_adj(OM.F(W, H, spp, mb, seed)), rb, re_, step)[0]
    kd_rows = float(np.any(g != 0, axis=1).mean())
    print("coverage %s: samples %.2f, Kd rows %.2f" % (_id(case), lit, kd_rows))
    assert lit >= MIN_SAMPLES
    assert kd_rows >= MIN_KD_ROWS


@pytest.mark.parametrize("case", [(n, f, None, b) for n in SL.MAT_RUNGS for b, f in enumerate(SL.mat_frames(n))], ids=_id)
def test_material_reference_reaches_the_glow_and_shiny_rows(oracles, case):
    """The frames of the material adjoint, under the drawn values it runs with."""
    name, (W, H, spp, mb, seed), _, _ = case
    r, Q = SL.RUNGS[name], oracles(name)
    gkd, gks, gke, stats = OM.reference(Q, OM.F(W, H, spp, mb, seed))
    kd_rows = float(np.any(gkd != 0, axis=1).mean())
    ke_rows = float(np.any(gke[18:16 + r.nE] != 0, axis=1).mean()) if r.nE > 2 else None
    ks_rows = float(np.any(gks[Q.lobe_mask] != 0, axis=1).mean()) if r.lobes else None
    print("coverage %s drawn values: Kd rows %.2f, Ke rows %s, Ks rows %s; %s" %
          (_id(case), kd_rows, ke_rows and "%.2f" % ke_rows, ks_rows and "%.2f" % ks_rows, stats))
    assert kd_rows >= MIN_KD_ROWS
    assert ke_rows is None or ke_rows >= MIN_KE_ROWS
    assert ks_rows is None or ks_rows >= MIN_KS_ROWS
    assert np.all(gks[~Q.lobe_mask] == 0) and np.all(gke[~Q.emitter_mask] == 0)
    if mb is None:
        assert stats["longest"] >= OM.LONG  # paths that outgrow the LDS ring slots
