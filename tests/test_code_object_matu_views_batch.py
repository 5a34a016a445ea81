"""The unbounded material adjoint over (material set, view) pairs in the built
library (no GPU needed): exactly four
trace_matu_views_batch_kernel<SPEC, BVH> instances exist under their own
__global__ name, with the registers, VGPR spills and scratch the build gives --
those of their twins trace_matu_kernel<SPEC, BVH>: the view sets' keying costs
scalar registers only -- and no static LDS.  The other families' instance
counts are unmoved.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
NEW = re.compile(r"_ZN3ipt29trace_matu_views_batch_kernelILb([01])ELb([01])EE")
TWIN = "_ZN3ipt17trace_matu_kernelILb%dELb%dEE"
# (SPEC, BVH) -> (VGPRs, VGPR spills, scratch bytes per lane), as built; the twins' figures
PINNED = {(0, 0): (96, 0, 0), (0, 1): (122, 0, 0), (1, 0): (96, 1, 16), (1, 1): (126, 0, 0)}
# the other families: prefix -> instances
FAMILIES = {
    "ipt::trace_kernel<": 21,
    "_ZN3ipt16trace_mat_kernelI": 4,
    "_ZN3ipt20trace_fwd_mat_kernelI": 8,
    "_ZN3ipt17trace_matu_kernelI": 4,
    "_ZN3ipt22trace_fwd_views_kernelI": 8,
    "_ZN3ipt22trace_mat_views_kernelI": 4,
    "_ZN3ipt28trace_fwd_views_batch_kernelI": 8,
    "_ZN3ipt28trace_mat_views_batch_kernelI": 4,
}


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_four_instances_with_their_twins_registers_and_no_static_lds():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    found = {}
    for k, v in r.items():
        m = NEW.match(k)
        if m:
            key = tuple(int(g) for g in m.groups())
            assert key not in found, k
            found[key] = v
    assert set(found) == set(PINNED) and len(found) == 4, sorted(found)
    for key in sorted(found):
        v = found[key]
        twins = [t for k, t in r.items() if k.startswith(TWIN % key)]
        assert len(twins) == 1, key
        t = twins[0]
        print(key, v, "twin", t)
        assert (v["vgpr"], v["vgpr_spill"], v["scratch_bytes_per_lane"]) == PINNED[key], (key, v)
        assert v["vgpr"] <= t["vgpr"], (key, v, t)
        assert v["vgpr_spill"] <= t["vgpr_spill"], (key, v, t)
        assert v["scratch_bytes_per_lane"] <= t["scratch_bytes_per_lane"], (key, v, t)
        assert v["static_lds_bytes"] == 0, (key, v)
    for prefix, n in FAMILIES.items():
        assert sum(1 for k in r if k.startswith(prefix)) == n, prefix
    # no count by prefix of another family sees the new name
    assert not any(k.startswith(p) for p in FAMILIES for k in r if NEW.match(k))
