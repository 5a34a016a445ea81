"""Cost of the material adjoint (ipt_adjoint_mat_dev: dL/dKd, dL/dKs, dL/dKe)
against the Kd-only bounded adjoint (ipt_adjoint_dev) on the same scenes:

    python tools/matgrad_cost.py [--launches 30] [--warmup 5] [--size 512] [--spp 64] > matgrad_cost.json

HIP events around each launch on one stream, the two kernels alternated so
that clock and thermal drift hit both alike; medians and the ratio per scene
(c3_phong: the SPEC instances; cornell: the diffuse ones).

    python tools/matgrad_cost.py --unbounded > matgrad_cost_unbounded.json

times the unbounded pair instead (max_bounces = -1): ipt_adjoint_mat_unbounded_dev
against ipt_adjoint_dev.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from inverse_path_tracer_amd import _native as N  # noqa: E402
from inverse_path_tracer_amd.scene import ObjectSpec, Scene  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
CORNELL = [ObjectSpec(os.path.join(ASSETS, "CornellBox", "CornellBox-Empty-CO.obj"),
                      os.path.join(ASSETS, "CornellBox", "CornellBox-Empty-CO.mtl"), (0, 0, 4), (0, 0, 0), (2, 2, 2))]
SCENES = {
    "c3_phong": CORNELL + [ObjectSpec(os.path.join(ASSETS, "phong", "cube_phong.obj"),
                                      os.path.join(ASSETS, "phong", "cube_phong.mtl"), (0, -1.5, 4), (0, 0, 0),
                                      (1, 1, 1))],
    "cornell": CORNELL,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--unbounded", action="store_true", help="the unbounded pair (max_bounces = -1)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    mb = None if a.unbounded else a.bounces
    mat_name = "adjoint_mat_unbounded_dev" if a.unbounded else "adjoint_mat_dev"
    mat_fn = L.ipt_adjoint_mat_unbounded_dev if a.unbounded else L.ipt_adjoint_mat_dev
    out = {"size": a.size, "spp": a.spp, "max_bounces": -1 if a.unbounded else a.bounces, "launches": a.launches, "warmup": a.warmup,
           "timer": "HIP events per launch, kernels alternated on one stream", "scenes": {}}
    for name, objs in SCENES.items():
        S = Scene(objs)
        p = N.make_params(a.size, a.size, a.spp, mb, 0)
        adj = torch.rand((a.size, a.size, 3), device="cuda") + 0.5
        g1 = torch.zeros((S.nT, 3), device="cuda", dtype=torch.float64)
        g3 = torch.zeros((3, S.nT, 3), device="cuda", dtype=torch.float64)

        def kd_only():
            N.check(L.ipt_adjoint_dev(S.handle, C.byref(p), None, adj.data_ptr(), g1.data_ptr(), stream), "adjoint")

        def materials():
            N.check(mat_fn(S.handle, C.byref(p), None, None, None, adj.data_ptr(), g3.data_ptr(), stream), mat_name)

        times = {"adjoint_dev": [], mat_name: []}
        for i in range(a.warmup + a.launches):
            for key, fn in (("adjoint_dev", kd_only), (mat_name, materials)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times[key].append(e0.elapsed_time(e1))
        n = a.launches
        # both accumulate: the Kd blocks must agree (the same paths, another fp64 order)
        kd_rel = float(((g3[0] - g1).abs().max() / g1.abs().max()).item())
        med = {k: statistics.median(v) for k, v in times.items()}
        out["scenes"][name] = {
            "nT": S.nT, "nE": S.nE,
            "adjoint_dev_ms": {"median": med["adjoint_dev"], "min": min(times["adjoint_dev"]),
                               "max": max(times["adjoint_dev"])},
            mat_name + "_ms": {"median": med[mat_name], "min": min(times[mat_name]), "max": max(times[mat_name])},
            "ratio_of_medians": med[mat_name] / med["adjoint_dev"],
            "kd_block_max_rel_diff": kd_rel, "launches": n,
        }
        S.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
