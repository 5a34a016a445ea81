"""The views' kernels in the built library (no GPU needed):
exactly eight trace_fwd_views_kernel<FWD | FWDM, SPEC, BVH> and four
trace_mat_views_kernel<SPEC, BVH> instances exist under their own __global__
names, and the view's 19 floats -- read from the table through the constant
address space at every loop iteration -- cost no register, spill or scratch
over their twins, trace_fwd_mat_kernel and trace_mat_kernel.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
FWD = re.compile(r"_ZN3ipt22trace_fwd_views_kernelILi([04])ELb([01])ELb([01])EE")
MAT = re.compile(r"_ZN3ipt22trace_mat_views_kernelILb([01])ELb([01])EE")
FWD_TWIN = "_ZN3ipt20trace_fwd_mat_kernelILi%dELb%dELb%dEE"
MAT_TWIN = "_ZN3ipt16trace_mat_kernelILb%dELb%dEE"

# Scratch bytes per lane this build measured, per (MODE, SPEC, BVH) / (SPEC, BVH).  Only the two SPEC BVH
# forwards use scratch, 16 B like their twins (4 and 5 spilled VGPRs, the twins' counts); every other
# instance, and all four adjoints, use none.  VGPRs equal the twins' everywhere (96 in the forwards, 95 / 119
# / 96 / 124 in the adjoints); SGPR spills are BELOW the twins' in all twelve (no per-set offsets to carry).
FWD_SCRATCH = {(0, 0, 0): 0, (0, 0, 1): 0, (0, 1, 0): 0, (0, 1, 1): 16,
               (4, 0, 0): 0, (4, 0, 1): 0, (4, 1, 0): 0, (4, 1, 1): 16}
MAT_SCRATCH = {(0, 0): 0, (0, 1): 0, (1, 0): 0, (1, 1): 0}


def find(r, rx, prefix):
    found = {}
    for k, v in r.items():
        m = rx.match(k)
        if m:
            key = tuple(int(g) for g in m.groups())
            assert key not in found, k
            found[key] = v
    return found


def twin_of(r, fmt, key):
    hits = [v for k, v in r.items() if k.startswith(fmt % key)]
    assert len(hits) == 1, (fmt % key, len(hits))
    return hits[0]


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_view_kernels_present_and_no_heavier_than_their_twins():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    fwd, mat = find(r, FWD, "fwd"), find(r, MAT, "mat")
    assert set(fwd) == set(FWD_SCRATCH) and len(fwd) == 8, sorted(fwd)
    assert set(mat) == set(MAT_SCRATCH) and len(mat) == 4, sorted(mat)
    for found, caps, fmt in ((fwd, FWD_SCRATCH, FWD_TWIN), (mat, MAT_SCRATCH, MAT_TWIN)):
        for key, cap in caps.items():
            v, t = found[key], twin_of(r, fmt, key)
            print(key, v, "twin", t)
            assert v["scratch_bytes_per_lane"] <= cap, (key, v)
            assert v["scratch_bytes_per_lane"] <= t["scratch_bytes_per_lane"], (key, v, t)
            assert v["vgpr_spill"] <= t["vgpr_spill"], (key, v, t)
            assert v["vgpr"] <= t["vgpr"], (key, v, t)
            assert v["static_lds_bytes"] == 0
    # the other entry points' instance counts did not move
    assert sum(1 for k in r if k.startswith("ipt::trace_kernel<")) == 21
    assert sum(1 for k in r if k.startswith("_ZN3ipt16trace_mat_kernelI")) == 4
    assert sum(1 for k in r if k.startswith("_ZN3ipt20trace_fwd_mat_kernelI")) == 8
    assert sum(1 for k in r if k.startswith("_ZN3ipt17trace_matu_kernelI")) == 4
