"""The views x material sets kernels in the built library (no GPU needed;
DESIGN.md §20): exactly eight trace_fwd_views_batch_kernel<FWD | FWDM, SPEC,
BVH> and four trace_mat_views_batch_kernel<SPEC, BVH> instances exist under
their own __global__ names, and the (set, view) decomposition costs no VGPR,
VGPR spill or scratch over their §18 twins, trace_fwd_views_kernel and
trace_mat_views_kernel.  The other families' instance counts are unmoved.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
FWD = re.compile(r"_ZN3ipt28trace_fwd_views_batch_kernelILi([04])ELb([01])ELb([01])EE")
MAT = re.compile(r"_ZN3ipt28trace_mat_views_batch_kernelILb([01])ELb([01])EE")
FWD_TWIN = "_ZN3ipt22trace_fwd_views_kernelILi%dELb%dELb%dEE"
MAT_TWIN = "_ZN3ipt22trace_mat_views_kernelILb%dELb%dEE"
FWD_KEYS = {(m, s, b) for m in (0, 4) for s in (0, 1) for b in (0, 1)}
MAT_KEYS = {(s, b) for s in (0, 1) for b in (0, 1)}


def find(r, rx):
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
def test_view_set_kernels_present_and_no_heavier_than_the_view_kernels():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    fwd, mat = find(r, FWD), find(r, MAT)
    assert set(fwd) == FWD_KEYS and len(fwd) == 8, sorted(fwd)
    assert set(mat) == MAT_KEYS and len(mat) == 4, sorted(mat)
    for found, fmt in ((fwd, FWD_TWIN), (mat, MAT_TWIN)):
        for key in sorted(found):
            v, t = found[key], twin_of(r, fmt, key)
            print(key, v, "twin", t)
            assert v["vgpr"] <= t["vgpr"], (key, v, t)
            assert v["vgpr_spill"] <= t["vgpr_spill"], (key, v, t)
            assert v["scratch_bytes_per_lane"] <= t["scratch_bytes_per_lane"], (key, v, t)
            assert v["static_lds_bytes"] == 0, (key, v)
    # the other entry points' instance counts did not move
    assert sum(1 for k in r if k.startswith("ipt::trace_kernel<")) == 21
    assert sum(1 for k in r if k.startswith("_ZN3ipt16trace_mat_kernelI")) == 4
    assert sum(1 for k in r if k.startswith("_ZN3ipt20trace_fwd_mat_kernelI")) == 8
    assert sum(1 for k in r if k.startswith("_ZN3ipt17trace_matu_kernelI")) == 4
    assert sum(1 for k in r if k.startswith("_ZN3ipt22trace_fwd_views_kernelI")) == 8
    assert sum(1 for k in r if k.startswith("_ZN3ipt22trace_mat_views_kernelI")) == 4
