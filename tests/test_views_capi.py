"""Views on the host side (no GPU): ipt_camera_look_at, ipt_views_create's
validation on a host-only scene, the origin bound, and the entry points'
refusals of dead handles and of bounce limits the views' adjoint does not take.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import SCENE0, product_scene
from inverse_path_tracer_amd import _native as N
from inverse_path_tracer_amd.scene import camera_at, camera_look_at


@pytest.fixture(scope="module")
def scene():
    s = product_scene(SCENE0, device=False)
    yield s
    s.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def create(scene, cams):
    """(rc, handle, message) of ipt_views_create on raw float32 matrices."""
    cams = np.ascontiguousarray(cams, np.float32)
    n = cams.size // 16
    h = C.c_void_p(0xDEAD)
    N.lib().ipt_clear_error()
    rc = N.lib().ipt_views_create(scene.handle, n, cams.ctypes.data_as(N.fp), C.byref(h))
    return rc, h, N.last_error()


def test_look_at_defaults_are_the_scene_camera_bit_for_bit(scene):
    cam = camera_look_at((0, 0, 0), (0, 0, 1), (0, 1, 0))
    assert cam.shape == (4, 4) and cam.dtype == np.float32
    assert np.array_equal(bits(cam), bits(scene.camera()))
    # the arguments are live: another direction, angle and aspect give another matrix
    side = camera_look_at((0, 0, 0), (1, 0, 1), (0, 1, 0), fov_deg=60, aspect=1.5)
    assert np.isfinite(side).all() and not np.array_equal(side, cam)
    t60 = np.float32(np.tan(np.float32(np.pi * 60.0 / 360.0)))
    assert abs(float(np.linalg.norm(side[0, :3])) - float(t60)) < 1e-6  # row 0 of S * V^T: tan(ha) * (s.x, u.x, f.x)


def test_views_accepts_the_scene_camera_on_a_host_only_scene(scene):
    v = scene.views(scene.camera()[None])
    assert len(v) == 1 and N.lib().ipt_views_count(v.handle) == 1
    assert np.array_equal(bits(v.cams[0]), bits(scene.camera()))
    three = scene.views(np.stack([scene.camera()] * 3))
    assert len(three) == 3 and N.lib().ipt_views_count(three.handle) == 3
    three.close()
    v.close()
    v.close()  # idempotent


def test_views_refusals_each_with_a_message(scene):
    cam = scene.camera()
    # n_views < 1 and > 65535
    for n in (0, -3, 65536):
        h = C.c_void_p(0xDEAD)
        N.lib().ipt_clear_error()
        buf = np.tile(cam.reshape(-1), max(1, n))
        assert N.lib().ipt_views_create(scene.handle, n, buf.ctypes.data_as(N.fp), C.byref(h)) == -1
        assert h.value is None and "n_views" in N.last_error()
    # a non-finite entry in rows 0..2 (a non-finite entry in row 3 is not read by any ray)
    for r, c, bad in ((0, 0, np.nan), (1, 2, np.inf), (2, 3, -np.inf)):
        m = cam.copy()
        m[r, c] = bad
        rc, h, msg = create(scene, np.stack([cam, m]))
        assert rc == -1 and h.value is None and "view 1" in msg and "non-finite" in msg, msg
    m = cam.copy()
    m[3, :] = np.nan
    rc, h, msg = create(scene, m)
    assert rc == 0 and h.value, msg
    N.lib().ipt_views_free(h)
    # a singular 3x3 part
    for m in (np.zeros((4, 4), np.float32), camera_at(np.ones((4, 4), np.float32), (0, 0, 0))):
        rc, h, msg = create(scene, m)
        assert rc == -1 and h.value is None and "determinant" in msg, msg
    # an origin outside the bound
    rc, h, msg = create(scene, camera_at(cam, (0, 1e6, 0)))
    assert rc == -1 and h.value is None and "origin" in msg and "bound" in msg, msg
    with pytest.raises(N.NativeError, match="origin"):
        scene.views(camera_at(cam, (-1e6, 0, 0))[None])


def test_origin_bound_is_exactly_the_coordinate_bound_minus_one(scene):
    # scene_coord_bound = 1 + the largest |coordinate| of a vertex or of the scene's own origin (bvh.cpp)
    tri = scene.triangles()
    want = np.float32(max(np.abs(tri[:, :9]).max(), np.abs(scene.camera()[:3, 3]).max()))
    bound = np.float32(scene.camera_bound)
    assert bound == want, (bound, want)
    up = np.nextafter(bound, np.float32(np.inf))
    cam = scene.camera()
    for axis in range(3):
        for sign in (1.0, -1.0):
            o = np.zeros(3, np.float32)
            o[axis] = sign * bound
            rc, h, msg = create(scene, camera_at(cam, o))
            assert rc == 0 and h.value, (axis, sign, msg)
            N.lib().ipt_views_free(h)
            o[axis] = sign * up
            rc, h, msg = create(scene, camera_at(cam, o))
            assert rc == -1 and h.value is None and "origin" in msg, (axis, sign, msg)


def entry_points(scene, handle, max_bounces=3):
    """rc and message of every views entry point on `handle` (none may reach a kernel)."""
    L = N.lib()
    p = N.make_params(8, 8, 2, max_bounces, 1)
    hdr = np.zeros((8, 8, 3), np.float32)
    grad = np.zeros((3, scene.nT, 3), np.float64)
    idx = np.zeros(1, np.int64)
    o = np.zeros(3, np.float32)
    calls = {
        "render_dev": lambda: L.ipt_render_views_dev(scene.handle, handle, C.byref(p), 128, None, None, None,
                                                     hdr.ctypes.data, None),
        "adjoint_dev": lambda: L.ipt_adjoint_views_dev(scene.handle, handle, C.byref(p), 128, None, None, None,
                                                       hdr.ctypes.data, grad.ctypes.data, None),
        "render_host": lambda: L.ipt_render_views_host(scene.handle, handle, C.byref(p), 128, hdr.ctypes.data_as(N.fp)),
        "adjoint_host": lambda: L.ipt_adjoint_views_host(scene.handle, handle, C.byref(p), 128,
                                                         hdr.ctypes.data_as(N.fp), grad.ctypes.data_as(N.dp)),
        "rays": lambda: L.ipt_views_rays_host(scene.handle, handle, 0, C.byref(p), 1,
                                              idx.ctypes.data_as(C.POINTER(C.c_int64)), o.ctypes.data_as(N.fp),
                                              o.ctypes.data_as(N.fp)),
        "count": lambda: L.ipt_views_count(handle),
    }
    out = {}
    for name, f in calls.items():
        L.ipt_clear_error()
        out[name] = (f(), N.last_error())
    return out


def test_dead_handles_are_refused_with_a_message(scene):
    for name, (rc, msg) in entry_points(scene, None).items():
        assert rc == -1 and "null views handle" in msg, (name, rc, msg)
    v = scene.views(scene.camera()[None])
    raw = C.c_void_p(v.handle.value)
    v.close()
    for name, (rc, msg) in entry_points(scene, raw).items():
        assert rc == -1 and "not live" in msg, (name, rc, msg)
    N.lib().ipt_views_free(raw)  # a second free of a dead handle is ignored
    N.lib().ipt_views_free(None)


def test_views_adjoint_takes_the_bounded_estimator_only(scene):
    v = scene.views(scene.camera()[None])
    for mb in (-1, 63):
        got = entry_points(scene, v.handle, mb)
        for name in ("adjoint_dev", "adjoint_host"):
            rc, msg = got[name]
            assert rc == -1 and "0..62" in msg, (mb, name, rc, msg)
    # and a host-only scene is refused by every launch, with the loader's message
    for name, (rc, msg) in entry_points(scene, v.handle).items():
        if name != "count":
            assert rc == -1 and "host-only" in msg, (name, rc, msg)
    v.close()
