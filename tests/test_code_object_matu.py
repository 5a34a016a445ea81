"""The unbounded material adjoint's kernels in the built library (no GPU
needed): exactly four trace_matu_kernel<SPEC, BVH> instances exist under their
own __global__ name -- they are instances neither of trace_kernel, whose count
tests/test_code_object.py pins, nor of trace_mat_kernel, which
tests/test_code_object_matgrad.py pins -- and they spill no more than their
twins, the Kd-only unbounded adjoints trace_kernel<3, SPEC, BVH>.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
MANGLED = re.compile(r"_ZN3ipt17trace_matu_kernelILb([01])ELb([01])EE")

# (SPEC, BVH) -> scratch bytes per lane of this build, with the VGPRs it was measured at:
# 96 / 122 / 96 / 126 (the twins: 96 / 124 / 96 / 128 VGPRs and 12 / 0 / 32 / 0 B; VGPR spills 0 / 0 / 1 / 0
# against the twins' 2 / 0 / 4 / 0).  None is above its twin.  The brute-force instances sit at the unbounded
# adjoint's 5 waves per SIMD; their owner lanes' carried state lives in LDS words, which is
# why they need less scratch than their twins.
SCRATCH = {(False, False): 0, (False, True): 0, (True, False): 16, (True, True): 0}
VGPRS = {(False, False): 96, (False, True): 122, (True, False): 96, (True, True): 126}


def twin(spec, bvh):
    return "ipt::trace_kernel<3, %s, %s>" % ("true" if spec else "false", "true" if bvh else "false")


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_unbounded_material_adjoint_kernels_present_and_spill_no_more_than_their_twins():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    found = {}
    for k, v in r.items():
        m = MANGLED.match(k)
        if m:
            key = (m.group(1) == "1", m.group(2) == "1")
            assert key not in found, k
            found[key] = v
    assert set(found) == set(SCRATCH) and len(found) == 4, sorted(found)
    for key, scratch in SCRATCH.items():
        t = r[twin(*key)]
        print(key, found[key], "twin", t)
        assert found[key]["vgpr_spill"] <= t["vgpr_spill"], (key, found[key], t)
        # pinned: a change of allocation in either direction should be looked at (and DESIGN §16.2 updated)
        assert found[key]["scratch_bytes_per_lane"] == scratch, (key, found[key])
        assert found[key]["vgpr"] == VGPRS[key] <= t["vgpr"], (key, found[key], t)
    # the other entry points' instance counts did not move
    assert sum(1 for k in r if k.startswith("ipt::trace_kernel<")) == 21
    assert sum(1 for k in r if k.startswith("_ZN3ipt16trace_mat_kernelI")) == 4
