"""The small-scene shading tables (scene_layout.h TriShade / EmitShade,
DESIGN.md §23) must not cost the C2 headline's kernels registers or occupancy
(no GPU needed).  The launches that take the tables run instances of their own,
trace_shade_kernel<MODE, SPEC, false>; the fused render (MODE 4) stays at <= 96
VGPRs (5 waves/SIMD) without scratch and the six-wave adjoint (MODE 5) at <= 80
VGPRs (6 waves/SIMD) with at most 8 B of scratch per lane, in both the old
instances trace_kernel<4 | 5, false, false>, which serve every other scene, and
the new ones -- read from the built library's code object metadata.
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


def shade_name(mode, spec):
    """trace_shade_kernel<mode, spec, false>'s symbol prefix (the tool demangles trace_kernel only)."""
    return "_ZN3ipt18trace_shade_kernelILi%dELb%dELb0EEE" % (mode, int(spec))


# kernel -> (max VGPRs, min waves/SIMD, max scratch bytes per lane)
BUDGET = {
    "ipt::trace_kernel<4, false, false>": (96, 5, 0),
    "ipt::trace_kernel<5, false, false>": (80, 6, 8),
    shade_name(4, False): (96, 5, 0),
    shade_name(5, False): (80, 6, 8),
    # the other instances that take the tables: 5 waves/SIMD and the scratch budget
    # that test_code_object.py sets for their trace_kernel twin
    shade_name(0, False): (96, 5, 0),
    shade_name(1, False): (96, 5, 0),
    shade_name(0, True): (96, 5, 0),
    shade_name(1, True): (96, 5, 0),
    shade_name(4, True): (96, 5, 32),
}


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_headline_kernels_keep_their_budgets_with_the_shade_tables():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    for want, (vgpr, waves, scratch) in BUDGET.items():
        found = [k for k in r if k.startswith(want)]
        assert len(found) == 1, (want, found)
        k = found[0]
        print(want, r[k], "waves/SIMD", WAVES(r[k]["vgpr"]))
        assert r[k]["vgpr"] <= vgpr, (want, r[k])
        assert WAVES(r[k]["vgpr"]) >= waves, (want, r[k])
        assert r[k]["scratch_bytes_per_lane"] <= scratch, (want, r[k])
    # seven instances: FWD, ADJ and FWDM with and without a Phong lobe, the six-wave adjoint without
    assert sum(1 for k in r if "trace_shade_kernel" in k) == 7
