"""The unbounded material adjoint's entry points through the C ABI, without a
GPU: ipt_adjoint_mat_unbounded_dev / ipt_adjoint_mat_unbounded_host are
declared, exported and bound, the ABI version did not move, and bad arguments,
a bounce cap and a host-only scene are refused with their messages (as
test_materials_capi.py and test_materials_batch_capi.py check the bounded
calls).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, product_scene

SCENE_A = CORNELL + [((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1), os.path.join(ASSETS, "phong", "cube_phong.obj"),
                      os.path.join(ASSETS, "phong", "cube_phong.mtl"))]
NAMES = ("ipt_adjoint_mat_unbounded_dev", "ipt_adjoint_mat_unbounded_host")


@pytest.fixture(scope="module")
def scene():
    S = product_scene(SCENE_A, device=False)
    yield S
    S.close()


def test_declared_exported_and_bound():
    from inverse_path_tracer_amd import _native as N
    from inverse_path_tracer_amd.scene import Scene

    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    raw = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/ipt.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(N.SIGNATURES[name][1]), name
        assert args[0] == "void *scene" and args[1] == "const ipt_params_t *p"
        assert hasattr(raw, name) and hasattr(N.lib(), name)
    # the device call has ipt_adjoint_mat_dev's signature, the host call ipt_adjoint_mat_host's
    assert N.SIGNATURES[NAMES[0]] == N.SIGNATURES["ipt_adjoint_mat_dev"]
    assert N.SIGNATURES[NAMES[1]] == N.SIGNATURES["ipt_adjoint_mat_host"]
    dev = re.search(r"ipt_adjoint_mat_unbounded_dev\s*\(([^;]*)\)", header).group(1)
    assert "double *grad_dev" in dev and dev.strip().endswith("void *stream")
    assert N.lib().ipt_abi_version() == 6 == N.ABI_VERSION
    assert callable(getattr(Scene, "adjoint_materials_unbounded"))


def test_bad_arguments_bounce_cap_and_host_only_scene(scene):
    from inverse_path_tracer_amd import NativeError
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    unb = N.make_params(8, 8, 1, None)
    assert unb.max_bounces == -1
    # any non-null addresses: every call below must be refused before it looks at them
    adj = np.zeros((8, 8, 3), np.float32)
    g = np.zeros((3, scene.nT, 3))
    a, gp = adj.ctypes.data, g.ctypes.data
    af, gd = adj.ctypes.data_as(N.fp), g.ctypes.data_as(N.dp)

    def refused(rc, what):
        assert rc == -1 and what in N.last_error(), (rc, N.last_error())
        L.ipt_clear_error()

    L.ipt_clear_error()
    refused(L.ipt_adjoint_mat_unbounded_dev(None, C.byref(unb), None, None, None, a, gp, None), "null scene")
    refused(L.ipt_adjoint_mat_unbounded_host(None, C.byref(unb), af, gd), "null scene")
    refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, None, None, None, None, a, gp, None), "bad arguments")
    refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, C.byref(unb), None, None, None, None, gp, None),
            "bad arguments")
    refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, C.byref(unb), None, None, None, a, None, None),
            "bad arguments")
    refused(L.ipt_adjoint_mat_unbounded_host(scene.handle, None, af, gd), "bad arguments")
    refused(L.ipt_adjoint_mat_unbounded_host(scene.handle, C.byref(unb), None, gd), "bad arguments")
    refused(L.ipt_adjoint_mat_unbounded_host(scene.handle, C.byref(unb), af, None), "bad arguments")
    # a bounce cap belongs to the bounded call, which the message names
    for mb in (0, 3, 62, 63):
        capped = N.make_params(8, 8, 1, mb)
        refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, C.byref(capped), None, None, None, a, gp, None),
                "ipt_adjoint_mat_dev")
        refused(L.ipt_adjoint_mat_unbounded_host(scene.handle, C.byref(capped), af, gd), "ipt_adjoint_mat_dev")
    # a host-only scene cannot be traced
    refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, C.byref(unb), None, None, None, a, gp, None), "host-only")
    refused(L.ipt_adjoint_mat_unbounded_host(scene.handle, C.byref(unb), af, gd), "host-only")
    with pytest.raises(NativeError, match="host-only"):
        scene.adjoint_materials_unbounded(adj, 8, 8, 1)
    # on a host-only scene that refusal comes before the frame's own checks (spp = 0 here)
    bad = N.make_params(8, 8, 0, None)
    refused(L.ipt_adjoint_mat_unbounded_dev(scene.handle, C.byref(bad), None, None, None, a, gp, None), "host-only")
    assert np.all(g == 0)
