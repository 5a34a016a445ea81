"""Views x material sets on the host side (no GPU): the argument
refusals of ipt_render_views_batch_dev / ipt_adjoint_views_batch_dev through
ctypes on a host-only scene -- each with its message, none reaching a kernel --
and MaterialOptimizer's refusal of tie_shared together with views.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import CORNELL, SCENE0, product_scene
from inverse_path_tracer_amd import _native as N


@pytest.fixture(scope="module")
def scene():
    s = product_scene(SCENE0, device=False)
    yield s
    s.close()


def entry_points(scene, handle, n_sets=2, max_bounces=3):
    """(rc, message) of both entry points; the buffers are host memory no kernel may reach."""
    L = N.lib()
    p = N.make_params(8, 8, 2, max_bounces, 1)
    hdr = np.zeros((4, 3, 8, 8, 3), np.float32)
    grad = np.zeros((4, 3, scene.nT, 3), np.float64)
    calls = {
        "render": lambda: L.ipt_render_views_batch_dev(scene.handle, handle, C.byref(p), n_sets, 128, None, None,
                                                       None, hdr.ctypes.data, None),
        "adjoint": lambda: L.ipt_adjoint_views_batch_dev(scene.handle, handle, C.byref(p), n_sets, 128, None, None,
                                                         None, hdr.ctypes.data, grad.ctypes.data, None),
    }
    out = {}
    for name, f in calls.items():
        L.ipt_clear_error()
        out[name] = (f(), N.last_error())
    return out


def refused(scene, handle, text, **kw):
    for name, (rc, msg) in entry_points(scene, handle, **kw).items():
        assert rc == -1 and text in msg, (name, kw, rc, msg)


def test_symbols_are_additive_and_the_abi_is_current():
    assert N.lib().ipt_abi_version() == 6
    assert "ipt_render_views_batch_dev" in N.SIGNATURES and "ipt_adjoint_views_batch_dev" in N.SIGNATURES


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
    for n in (0, -2):
        refused(scene, v.handle, "n_sets", n_sets=n)
    refused(scene, v.handle, "65535", n_sets=21846)        # 21846 * 3 = 65538 pairs
    refused(scene, v.handle, "host-only", n_sets=21845)    # 65535 pairs pass the argument checks
    for mb in (-1, 63):
        refused(scene, v.handle, "0..62", max_bounces=mb)
    # required pointers
    p = N.make_params(8, 8, 2, 3, 1)
    N.lib().ipt_clear_error()
    assert N.lib().ipt_render_views_batch_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None, None,
                                              None) == -1 and "hdr_dev" in N.last_error()
    N.lib().ipt_clear_error()
    assert N.lib().ipt_adjoint_views_batch_dev(scene.handle, v.handle, C.byref(p), 2, 128, None, None, None, None,
                                               None, None) == -1 and "grad_dev" in N.last_error()
    # well-formed arguments on a host-only scene: the loader's message, as ipt_adjoint_views_dev
    refused(scene, v.handle, "host-only")
    v.close()


def test_tie_shared_together_with_views_raises():
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    cams = np.eye(4, dtype=np.float32)[None]
    with pytest.raises(ValueError, match="tie_shared"):
        MaterialOptimizer([], 8, 8, 1, 3, tie_shared=18, views=cams)
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError, match="views"):
            MaterialOptimizer([], 8, 8, 1, 3, views=bad)
        with pytest.raises(ValueError, match="views"):
            build_tasks([], 8, 8, 1, 3, 0.5, None, views=bad)
    assert MaterialOptimizer([], 8, 8, 1, 3, views=cams).cams.shape == (1, 4, 4)
