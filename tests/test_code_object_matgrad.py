"""The material adjoint's kernels in the built library (no GPU needed): the
four trace_mat_kernel<SPEC, BVH> instances exist under their own __global__
name -- they are NOT instances of trace_kernel, whose count
tests/test_code_object.py pins -- and stay within their scratch budget.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
MANGLED = re.compile(r"_ZN3ipt16trace_mat_kernelILb([01])ELb([01])EE")

# (SPEC, BVH) -> max scratch bytes per lane: the values of this build (all 0, so
# none needs the DESIGN sentence asked of anything above 32 B/lane), with the
# VGPRs it was measured at: 95 / 119 / 96 / 124 -- the bounded adjoint's own
# 5 (brute force) and 2 (BVH) waves per SIMD.
BUDGET = {(False, False): 0, (False, True): 0, (True, False): 0, (True, True): 0}


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_material_adjoint_kernels_present_and_within_scratch_budget():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    found = {}
    for k, v in r.items():
        m = MANGLED.match(k)
        if m:
            found[(m.group(1) == "1", m.group(2) == "1")] = v
    assert set(found) == set(BUDGET), sorted(found)
    for key, cap in BUDGET.items():
        assert found[key]["scratch_bytes_per_lane"] <= cap, (key, found[key])
        assert found[key]["vgpr_spill"] == 0, (key, found[key])
    # brute-force instances hold the bounded adjoint's 5 waves/SIMD (<= 96 VGPRs)
    assert found[(False, False)]["vgpr"] <= 96 and found[(True, False)]["vgpr"] <= 96
    assert any("pack_mat_kernel" in k for k in r)
