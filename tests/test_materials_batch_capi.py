"""The batched material entry points through the C ABI, without a GPU:
ipt_render_mat_batch_dev / ipt_adjoint_mat_batch_dev are declared, exported and
bound, the ABI version did not move, and bad arguments or a host-only scene are
refused with a message (as test_materials_capi.py checks the single-set calls).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, product_scene

SCENE_A = CORNELL + [((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1), os.path.join(ASSETS, "phong", "cube_phong.obj"),
                      os.path.join(ASSETS, "phong", "cube_phong.mtl"))]
NAMES = ("ipt_render_mat_batch_dev", "ipt_adjoint_mat_batch_dev")


@pytest.fixture(scope="module")
def scene():
    S = product_scene(SCENE_A, device=False)
    yield S
    S.close()


def test_declared_exported_and_bound():
    from inverse_path_tracer_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    raw = C.CDLL(N.LIB_PATH)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, "%s is not declared in include/ipt.h" % name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(N.SIGNATURES[name][1]), name
        assert args[2] == "int n_scenes" and args[3] == "uint64_t seed_stride" and args[-1] == "void *stream"
        assert hasattr(raw, name) and hasattr(N.lib(), name)
    assert "double *grad_dev" in re.search(r"ipt_adjoint_mat_batch_dev\s*\(([^;]*)\)", header).group(1)
    assert N.lib().ipt_abi_version() == 6 == N.ABI_VERSION


def test_bad_arguments_and_host_only_scene(scene):
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    par = N.make_params(8, 8, 1, 2)
    # any non-null addresses: every call below must be refused before it looks at them
    hdr = np.zeros((2, 8, 8, 3), np.float32)
    adj = np.zeros((2, 8, 8, 3), np.float32)
    g = np.zeros((2, 3, scene.nT, 3))
    h, a, gp = hdr.ctypes.data, adj.ctypes.data, g.ctypes.data

    def refused(rc, what):
        assert rc == -1 and what in N.last_error(), (rc, N.last_error())
        L.ipt_clear_error()

    L.ipt_clear_error()
    refused(L.ipt_render_mat_batch_dev(None, C.byref(par), 2, 64, None, None, None, h, None), "null scene")
    refused(L.ipt_adjoint_mat_batch_dev(None, C.byref(par), 2, 64, None, None, None, a, gp, None), "null scene")
    refused(L.ipt_render_mat_batch_dev(scene.handle, None, 2, 64, None, None, None, h, None), "bad arguments")
    refused(L.ipt_adjoint_mat_batch_dev(scene.handle, None, 2, 64, None, None, None, a, gp, None), "bad arguments")
    refused(L.ipt_render_mat_batch_dev(scene.handle, C.byref(par), 2, 64, None, None, None, None, None),
            "bad arguments")
    refused(L.ipt_adjoint_mat_batch_dev(scene.handle, C.byref(par), 2, 64, None, None, None, None, gp, None),
            "bad arguments")
    refused(L.ipt_adjoint_mat_batch_dev(scene.handle, C.byref(par), 2, 64, None, None, None, a, None, None),
            "bad arguments")
    for n in (0, -3):
        refused(L.ipt_render_mat_batch_dev(scene.handle, C.byref(par), n, 64, None, None, None, h, None), "n_scenes")
        refused(L.ipt_adjoint_mat_batch_dev(scene.handle, C.byref(par), n, 64, None, None, None, a, gp, None),
                "n_scenes")
    # a host-only scene cannot be traced, with one set or several
    for n in (1, 2):
        refused(L.ipt_render_mat_batch_dev(scene.handle, C.byref(par), n, 64, None, None, None, h, None), "host-only")
        refused(L.ipt_adjoint_mat_batch_dev(scene.handle, C.byref(par), n, 64, None, None, None, a, gp, None),
                "host-only")
    assert np.all(g == 0) and np.all(hdr == 0)
