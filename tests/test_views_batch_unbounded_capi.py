"""Views x material sets at no bounce cap on the host side (no GPU; DESIGN.md
§21): the argument refusals of ipt_render_views_batch_unbounded_dev /
ipt_adjoint_views_batch_unbounded_dev through ctypes on a host-only scene --
each with its message, none reaching a kernel -- and the symbols themselves.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import CORNELL, SCENE0, product_scene
from inverse_path_tracer_amd import _native as N

NAMES = ("ipt_render_views_batch_unbounded_dev", "ipt_adjoint_views_batch_unbounded_dev")


@pytest.fixture(scope="module")
def scene():
    s = product_scene(SCENE0, device=False)
    yield s
    s.close()


def entry_points(scene, handle, n_sets=2, max_bounces=None, spp=2):
    """(rc, message) of both entry points; the buffers are host memory no kernel may reach."""
    L = N.lib()
    p = N.make_params(8, 8, spp, max_bounces, 1)
    hdr = np.zeros((4, 3, 8, 8, 3), np.float32)
    grad = np.zeros((4, 3, scene.nT, 3), np.float64)
    calls = {
        "render": lambda: L.ipt_render_views_batch_unbounded_dev(scene.handle, handle, C.byref(p), n_sets, 128, None,
                                                                 None, None, hdr.ctypes.data, None),
        "adjoint": lambda: L.ipt_adjoint_views_batch_unbounded_dev(scene.handle, handle, C.byref(p), n_sets, 128, None,
                                                                   None, None, hdr.ctypes.data, grad.ctypes.data, None),
    }
    out = {}
    for name, f in calls.items():
        L.ipt_clear_error()
        out[name] = (f(), N.last_error())
    assert not hdr.any() and not grad.any()
    return out


def refused(scene, handle, text, **kw):
    for name, (rc, msg) in entry_points(scene, handle, **kw).items():
        assert rc == -1 and text in msg, (name, kw, rc, msg)


def test_symbols_are_additive_and_the_abi_is_current():
    L = N.lib()
    assert L.ipt_abi_version() == 6 and N.ABI_VERSION == 6
    header = open(N.HEADER_PATH).read()
    for name in NAMES:
        assert name in N.SIGNATURES and callable(getattr(L, name))
        assert "int %s(" % name in header
    # the bounded pair is still there, with its own signature
    for name in ("ipt_render_views_batch_dev", "ipt_adjoint_views_batch_dev", "ipt_adjoint_mat_unbounded_dev"):
        assert name in N.SIGNATURES and callable(getattr(L, name))
    assert N.SIGNATURES[NAMES[0]] == N.SIGNATURES["ipt_render_views_batch_dev"]
    assert N.SIGNATURES[NAMES[1]] == N.SIGNATURES["ipt_adjoint_views_batch_dev"]


def test_dead_and_foreign_handles_are_refused(scene):
    refused(scene, None, "null views handle")
    v = scene.views(scene.camera()[None])
    raw = C.c_void_p(v.handle.value)
    v.close()
    refused(scene, raw, "not live")
    other = product_scene(CORNELL, device=False)
    ov = other.views(other.camera()[None])
    refused(scene, ov.handle, "another scene")
    ov.close()
    other.close()


def test_argument_refusals_report_on_a_host_only_scene(scene):
    v = scene.views(np.stack([scene.camera()] * 3))
    # a bounce cap belongs to the bounded pair, which the message names
    for mb in (0, 4, 62, 63):
        refused(scene, v.handle, "max_bounces must be -1", max_bounces=mb)
        refused(scene, v.handle, "ipt_adjoint_views_batch_dev", max_bounces=mb)
    for n in (0, -2):
        refused(scene, v.handle, "n_sets must be >= 1", n_sets=n)
    refused(scene, v.handle, "65535 (material set, view) pairs", n_sets=21846)  # 21846 * 3 = 65538 pairs
    # 65535 pairs pass the argument checks: the scene reports itself last
    refused(scene, v.handle, "host-only", n_sets=21845)
    refused(scene, v.handle, "host-only", spp=0)  # (the render parameters are the device path's check)
    # the cap's refusal comes before the others
    refused(scene, v.handle, "max_bounces must be -1", max_bounces=4, n_sets=0)
    # required pointers
    p = N.make_params(8, 8, 2, None, 1)
    L = N.lib()
    L.ipt_clear_error()
    assert L.ipt_render_views_batch_unbounded_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None, None,
                                                  None) == -1 and "hdr_dev" in N.last_error()
    L.ipt_clear_error()
    assert L.ipt_adjoint_views_batch_unbounded_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None, None,
                                                   None, None) == -1 and "grad_dev" in N.last_error()
    L.ipt_clear_error()
    assert L.ipt_render_views_batch_unbounded_dev(scene.handle, v.handle, None, 2, 128, None, None, None, None,
                                                  None) == -1 and "params" in N.last_error()
    # well-formed arguments on a host-only scene: the loader's message
    refused(scene, v.handle, "host-only")
    v.close()


def test_the_bounded_entry_points_keep_refusing_no_cap(scene):
    """Every existing refusal stays word for word: the bounded pair does not start taking -1."""
    v = scene.views(scene.camera()[None])
    L = N.lib()
    p = N.make_params(8, 8, 2, None, 1)
    buf = np.zeros((2, 1, 8, 8, 3), np.float32)
    grad = np.zeros((2, 3, scene.nT, 3), np.float64)
    L.ipt_clear_error()
    assert L.ipt_render_views_batch_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None, buf.ctypes.data,
                                        None) == -1
    assert "views batch: give max_bounces in 0..62 (the unbounded estimator is not supported)" in N.last_error()
    L.ipt_clear_error()
    assert L.ipt_adjoint_views_batch_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None,
                                         buf.ctypes.data, grad.ctypes.data, None) == -1
    assert "views batch: give max_bounces in 0..62 (the unbounded estimator is not supported)" in N.last_error()
    v.close()
