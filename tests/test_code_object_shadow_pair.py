"""The one-pair shadow cast (ipt_device.h, shadow_hit_pairs_small) must
not cost the C2 headline's kernels registers or occupancy (no GPU needed): the
fused render trace_kernel<4, false, false> stays at <= 96 VGPRs (5 waves/SIMD)
without scratch, the 6-wave adjoint trace_kernel<5, false, false> at <= 80
VGPRs (6 waves/SIMD) -- the values before the change, read from the built
library's code object metadata.
"""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")

# gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves
WAVES = lambda vgpr: min(8, 512 // (8 * ((vgpr + 7) // 8)))  # noqa: E731

# kernel -> (max VGPRs, min waves/SIMD, max scratch bytes per lane)
BEFORE = {
    "ipt::trace_kernel<4, false, false>": (96, 5, 0),
    "ipt::trace_kernel<5, false, false>": (80, 6, 8),
}


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_headline_kernels_keep_their_registers_and_occupancy():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    for k, (vgpr, waves, scratch) in BEFORE.items():
        assert k in r, k
        print(k, r[k], "waves/SIMD", WAVES(r[k]["vgpr"]))
        assert r[k]["vgpr"] <= vgpr, (k, r[k])
        assert WAVES(r[k]["vgpr"]) >= waves, (k, r[k])
        assert r[k]["scratch_bytes_per_lane"] <= scratch, (k, r[k])
