"""The kernels of the material batch in the built library (no GPU needed,
DESIGN.md §15): the batched forward with per-set TriMat tables has eight
instances of its own, trace_fwd_mat_kernel<MODE, SPEC, BVH> for the two forward
modes -- they are NOT instances of trace_kernel, whose count
tests/test_code_object.py pins -- and each uses what its trace_kernel
counterpart uses: the same body plus one pointer offset ahead of the loop.
"""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_object_resources as COR  # noqa: E402

LIB = os.path.join(ROOT, "inverse_path_tracer_amd", "lib", "libipt_amd.so")
MANGLED = re.compile(r"_ZN3ipt20trace_fwd_mat_kernelILi(\d+)ELb([01])ELb([01])EE")
FWD, FWDM = 0, 4  # the forward modes (ipt_hip.hip MODE_FWD, MODE_FWDM)


@pytest.mark.skipif(not os.path.exists(COR.READELF), reason="llvm-readelf absent")
def test_batch_forward_instances_match_their_trace_kernel_counterparts():
    assert os.path.exists(LIB), "run __graft_entry__.build()"
    r = COR.resources(LIB)
    found = {}
    for k, v in r.items():
        m = MANGLED.match(k)
        if m:
            found[(int(m.group(1)), m.group(2) == "1", m.group(3) == "1")] = v
    assert set(found) == {(mode, s, b) for mode in (FWD, FWDM) for s in (False, True) for b in (False, True)}
    for (mode, spec, bvh), v in found.items():
        twin = r["ipt::trace_kernel<%d, %s, %s>" % (mode, str(spec).lower(), str(bvh).lower())]
        for key in ("vgpr", "vgpr_spill", "scratch_bytes_per_lane", "static_lds_bytes"):
            assert v[key] <= twin[key], (mode, spec, bvh, key, v, twin)
    assert any("pack_mat_kernel" in k for k in r) and any("replicate_kernel" in k for k in r)
