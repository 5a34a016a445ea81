"""The tangent launch without a GPU: the C ABI of ipt_tangent_mat_dev / ipt_tangent_mat_host
(declared, exported, bound, every refusal with its message), the code object of trace_tan_kernel, and the
REFERENCE the GPU file compares with, from the CPU oracle as it stands:

    T_ref[k, p, c] = sum over blocks and rows of g_p[block][row][c] * v_k[block][row][c]
    A_ref[k, p, c] = the same with the absolute values of both factors

where g_p is OracleScene.adjoint_materials under the adjoint image that is (1, 1, 1) at pixel p and 0 elsewhere (one
row-restricted call per pixel; all arithmetic is per channel, so one call gives the three channels).  This module owns
what tests/test_gpu_tangent.py shares with it: the tangents, the reference and its cache, the bar.
"""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import scene_ladder as SL
import test_oracle_materials as OM
from conftest import ASSETS, CORNELL, product_scene
from test_gpu_materials import scene_b
from test_gpu_materials_unbounded import sphere_records

NAMES = ("ipt_tangent_mat_dev", "ipt_tangent_mat_host")
COVERAGE = 0.85  # A_ref > 0 in at least this share of a frame's entries
# (scene, frame, K) of the GPU file's comparisons with the oracle
GPU_FRAMES = [("B", f, 3) for f in OM.B_BOUNDED] + [("glow", OM.GLOW[0], 16), ("sphere", OM.SPHERE[0], 2)]
# ... and of tests/test_gpu_scene_ladder.py: the generated scenes (scene_ladder.py)
GPU_FRAMES += [("ladder:" + n, OM.LADDER_TAN[n], K) for n, (K, _, _) in SL.TANGENTS.items()]
SCENE_A = CORNELL + [((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1), os.path.join(ASSETS, "phong", "cube_phong.obj"),
                      os.path.join(ASSETS, "phong", "cube_phong.mtl"))]


# ------------------------------------------------------------------ shared with the GPU file
def records(tmp, name):
    if name.startswith("ladder:"):
        return SL.records(tmp, name[len("ladder:"):])
    return {"B": lambda: scene_b(tmp, tag="t"), "glow": lambda: OM.glow_records(tmp),
            "sphere": lambda: sphere_records(tmp)}[name]()


def draw_tangents(Q, K, seed=77):
    """(tkd, tks, tke), (K, nT, 3) float32 each: signed, uniform(-1, 1), every entry distinct; the rows outside the
    masks carry junk that must never be read into a result."""
    rs = np.random.RandomState(seed)
    tkd, tks, tke = (rs.uniform(-1, 1, (K, Q.nT, 3)).astype(np.float32) for _ in range(3))
    tks[:, ~Q.lobe_mask] = 1.0e3
    tke[:, ~Q.emitter_mask] = -7.0e2
    return tkd, tks, tke


def pixel_gradients(Q, f):
    """Yields (band row index, column, g) with g the (3, nT, 3) one-hot material gradient of that pixel."""
    rb, re_, step = OM.frame_rows(f)
    for i, y in enumerate(range(rb, re_, step)):
        for x in range(f.W):
            onehot = np.zeros((f.H, f.W, 3), np.float32)
            onehot[y, x] = 1.0
            yield i, x, np.stack(Q.adjoint_materials(f.W, f.H, f.spp, f.mb, f.seed, onehot, y, y + 1))


_REFS = {}


def reference(Q, name, f, tangents):
    """(T_ref, A_ref), (K, rows, W, 3) float64 each, of frame f under the oracle's current values; one oracle sweep
    per (scene, frame, tangents), shared by the tests that need it and left unchanged."""
    key = (name, f, tuple(None if t is None else t.tobytes() for t in tangents))
    if key not in _REFS:
        K = next(t for t in tangents if t is not None).shape[0]
        V = np.stack([np.zeros((K, Q.nT, 3)) if t is None else t.astype(np.float64) for t in tangents], axis=1)
        rb, re_, step = OM.frame_rows(f)
        T = np.zeros((K, len(range(rb, re_, step)), f.W, 3))
        A = np.zeros_like(T)
        for i, x, g in pixel_gradients(Q, f):
            T[:, i, x] = np.einsum("brc,kbrc->kc", g, V)
            A[:, i, x] = np.einsum("brc,kbrc->kc", np.abs(g), np.abs(V))
        T.setflags(write=False)
        A.setflags(write=False)
        _REFS[key] = (T, A)
    return _REFS[key]


def coverage(A):
    return float(np.count_nonzero(A)) / A.size


def compare(got, T, A, rtol=OM.RTOL, atol=OM.ATOL, tag=""):
    """Every entry: |T - T_ref| <= rtol * A_ref + atol; an entry whose A_ref is 0 is exactly 0."""
    assert got.shape == T.shape and got.dtype == np.float64
    err = np.abs(got - T)
    worst = float(np.max(err / (rtol * A + atol)))
    print("tangent %s: worst %.3e of the bar, max|T| %.3e, coverage %.1f%%" % (tag, worst, np.abs(T).max(),
                                                                             100 * coverage(A)))
    assert np.all(err <= rtol * A + atol), worst
    assert np.all(got[A == 0] == 0)
    assert coverage(A) >= COVERAGE


# ------------------------------------------------------------------ 1. the C ABI
@pytest.fixture(scope="module")
def scene():
    S = product_scene(SCENE_A, device=False)
    yield S
    S.close()


def test_declared_exported_and_bound():
    from inverse_path_tracer_amd import _native as N
    from inverse_path_tracer_amd import optimize, torch_ops
    from inverse_path_tracer_amd.scene import Scene

    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    raw = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/ipt.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(N.SIGNATURES[name][1]), name
        assert args[0] == "void *scene" and args[1] == "const ipt_params_t *p" and "int n_tangents" in args
        assert hasattr(raw, name) and hasattr(N.lib(), name)
    dev = re.search(r"ipt_tangent_mat_dev\s*\(([^;]*)\)", header).group(1)
    assert "double *tan_dev" in dev and dev.strip().endswith("void *stream")
    assert N.lib().ipt_abi_version() == 6 == N.ABI_VERSION
    assert callable(Scene.tangent_materials) and callable(torch_ops.tangent_materials)
    assert callable(optimize.gauss_newton_materials) and hasattr(torch_ops._MaterialsFn, "jvp")


def _many_triangles(path, n):
    """An OBJ of n triangles (a strip over a row of vertices)."""
    with open(path, "w") as fh:
        for i in range(n + 2):
            fh.write("v %g %g 5\n" % (i * 1e-4, (i & 1) * 1e-4))
        for i in range(n):
            fh.write("f %d %d %d\n" % (i + 1, i + 2, i + 3))
    return path


def test_refusals(scene):
    """Each refusal returns non-zero with its message, before anything is allocated or enqueued: all of them reach
    a host-only scene, which reports itself last."""
    from inverse_path_tracer_amd import NativeError
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    par = N.make_params(8, 8, 2, 3)
    nT = scene.nT
    t = np.ones((16, nT, 3), np.float32)
    out = np.zeros((16, 8, 8, 3))
    tp, tf, od = t.ctypes.data, t.ctypes.data_as(N.fp), out.ctypes.data_as(N.dp)

    def dev(p=par, K=1, tkd=tp, tks=None, tke=None, o=out.ctypes.data, s=scene):
        return L.ipt_tangent_mat_dev(s.handle if s else None, C.byref(p) if p else None, None, None, None, K, tkd, tks,
                                     tke, o, None)

    def host(p=par, K=1, tkd=tf, tks=None, tke=None, o=od, s=scene):
        return L.ipt_tangent_mat_host(s.handle if s else None, C.byref(p) if p else None, K, tkd, tks, tke, o)

    def refused(rc, what):
        assert rc == -1 and what in N.last_error(), (rc, what, N.last_error())
        L.ipt_clear_error()

    L.ipt_clear_error()
    for call in (dev, host):
        refused(call(s=None), "null scene")
        refused(call(p=None), "bad arguments")
        refused(call(o=None), "bad arguments")
        for K in (0, -1, 17):
            refused(call(K=K), "n_tangents must be in 1..16")
        refused(call(tkd=None), "at least one of the tangent arrays")
        for mb in (None, 63):
            refused(call(p=N.make_params(8, 8, 2, mb)), "max_bounces in 0..62")
        refused(call(p=N.make_params(8, 8, 0, 3)), "invalid render parameters")
        # 62 bounces: 63 records x 5 fields x 256 lanes x 4 B of LDS alone
        refused(call(p=N.make_params(8, 8, 2, 62), K=16), "LDS footprint")
        # what passes every check of the call meets the scene: host-only
        refused(call(), "host-only")
        refused(call(K=16, tkd=None, tke=tp if call is dev else tf), "host-only")
    assert np.all(out == 0)
    with pytest.raises(NativeError, match="host-only"):
        scene.tangent_materials(t[0], None, None, 8, 8, 2, 3)
    with pytest.raises(NativeError, match="at least one"):
        scene.tangent_materials(None, None, None, 8, 8, 2, 3)
    with pytest.raises(ValueError):
        scene.tangent_materials(t[:2], t[:3], None, 8, 8, 2, 3)


@pytest.mark.slow
def test_refuses_more_than_65535_triangles(tmp_path):
    """(Loading 65536 triangles host-only takes most of a minute on the CPU: tri and et share one 32-bit record field.)"""
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    par = N.make_params(8, 8, 2, 3)
    big = product_scene([((0, 0, 0), (0, 0, 0), (1, 1, 1), _many_triangles(str(tmp_path / "strip.obj"), 65536),
                          "*Kd 0.5 0.5 0.5*")], device=False)
    try:
        assert big.nT == 65536
        tb = np.zeros((1, big.nT, 3), np.float32)
        out = np.zeros((1, 8, 8, 3))
        L.ipt_clear_error()
        assert L.ipt_tangent_mat_dev(big.handle, C.byref(par), None, None, None, 1, tb.ctypes.data, None, None,
                                     out.ctypes.data, None) == -1
        assert "at most 65535 triangles" in N.last_error()
        L.ipt_clear_error()
        assert L.ipt_tangent_mat_host(big.handle, C.byref(par), 1, tb.ctypes.data_as(N.fp), None, None,
                                      out.ctypes.data_as(N.dp)) == -1
        assert "at most 65535 triangles" in N.last_error()
        L.ipt_clear_error()
    finally:
        big.close()


# ------------------------------------------------------------------ 2. the reference itself
_SCENES = {}


@pytest.mark.parametrize("name,f,K", GPU_FRAMES, ids=["%s-%s-K%d" % (n, OM.frame_id(f), k) for n, f, k in GPU_FRAMES])
def test_reference_coverage_and_linearity(oracle, tmp_path_factory, name, f, K):
    """On every frame the GPU file compares: A_ref > 0 in at least 85% of the entries (the comparison is scaled by
    A_ref, so an entry with A_ref = 0 checks only an exact zero), the reference of K tangents is the K
    single-tangent references, and the masked rows' junk reaches nothing."""
    if name not in _SCENES:
        _SCENES[name] = oracle.OracleScene(records(tmp_path_factory.mktemp("tan_" + name), name))
        _SCENES[name].set_material_params(*OM.draw_values(_SCENES[name], 1)[0])
    Q = _SCENES[name]
    tang = draw_tangents(Q, K)
    t0 = time.time()
    T, A = reference(Q, name, f, tang)
    dt = time.time() - t0
    print("reference %s %s K=%d: %.2f s, coverage %.1f%%, max|T| %.3e, min |T|/A %.1e" %
          (name, OM.frame_id(f), K, dt, 100 * coverage(A), np.abs(T).max(), (np.abs(T)[A > 0] / A[A > 0]).min()))
    assert coverage(A) >= COVERAGE, coverage(A)
    assert np.all(np.abs(T) <= A * (1 + 1e-12)) and np.any(T != 0)
    if name == "sphere":  # one sweep of 6.5 s is enough: linearity is checked on the small scenes
        assert (Q.lobe_mask & ~OM.hot_set(Q)).any()
        return
    clean = [t.copy() for t in tang]
    clean[1][:, ~Q.lobe_mask] = 0
    clean[2][:, ~Q.emitter_mask] = 0
    Tc, Ac = reference(Q, name, f, clean)
    assert np.array_equal(Tc, T) and np.array_equal(Ac, A)
    for k in sorted({0, K - 1}):
        T1, A1 = reference(Q, name, f, [t[k:k + 1] for t in tang])
        assert np.array_equal(T1[0], T[k]) and np.array_equal(A1[0], A[k])


# ------------------------------------------------------------------ 3. the code object
TAN = re.compile(r"_ZN3ipt16trace_tan_kernelILb([01])ELb([01])EE")
TWIN = "_ZN3ipt16trace_mat_kernelILb%dELb%dEE"
# (SPEC, BVH) -> VGPRs.  The twins trace_mat_kernel<SPEC, BVH>: 95 / 96 brute force, 119 / 124 BVH, no scratch.
VGPR = {(0, 0): 96, (1, 0): 96, (0, 1): 121, (1, 1): 127}


def test_code_object():
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from code_object_resources import resources

    r = resources()
    mine = {tuple(int(x) for x in TAN.match(k).groups()): v for k, v in r.items() if TAN.match(k)}
    assert sorted(mine) == sorted(VGPR), "exactly four instances of trace_tan_kernel"
    assert sum(1 for k in r if "trace_tan_kernel" in k) == 4
    for key, v in mine.items():
        twin = [t for k, t in r.items() if k.startswith(TWIN % key)]
        assert len(twin) == 1
        print("trace_tan_kernel<%d,%d>: %s; twin %s" % (key + (v, twin[0])))
        assert v["static_lds_bytes"] == 0
        assert v["vgpr"] == VGPR[key] and v["vgpr_spill"] == 0
        assert v["scratch_bytes_per_lane"] == 0 and v["scratch_bytes_per_lane"] <= twin[0]["scratch_bytes_per_lane"]
