"""Cost of the tangent launch (ipt_tangent_mat_dev: K tangent images, the
paths traced once) against the launch it is built from, the
bounded material adjoint (ipt_adjoint_mat_dev), in one process:

    python tools/tangent_cost.py [--ks 1 4 16] [--size 512] [--spp 64] [--launches 20] [--warmup 3]

writes profiles/tangent/tangent_cost.json (--out).  HIP events around each
launch on one stream, the variants alternated so that clock and thermal drift
hit all alike; medians and ratios per scene (c3_phong: the SPEC instances;
cornell: the diffuse ones).

    python tools/tangent_cost.py --phases inverse_path_tracer_amd/lib/variants/libipt_phase.so

writes profiles/tangent/phase_split.json instead: the loop's phases in wave
cycles for the same launches, from an IPT_PHASE_TIMING build.  The tangents are random in all three blocks; the
tangent images accumulate like the gradient does, so neither output is zeroed
between launches.
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


PHASES = ["refill", "path_cast", "shade", "shadow_cast", "emitter_eval", "finalise_and_sweep"]


def phase_split(a):
    """--phases: summed wave cycles per phase of the loop (tools/phase_timing.py's
    counters) of one adjoint launch and one tangent launch per K, from a library
    built with -DIPT_PHASE_TIMING (make variant V=phase DEFS=-DIPT_PHASE_TIMING).
    The sweep is part of the last phase."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import variant_bench as VB

    L = VB.load(a.phases)
    L.ipt_debug_phase_cycles.argtypes = [C.POINTER(C.c_ulonglong)]
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    p = N.make_params(a.size, a.size, a.spp, a.bounces, 0)
    out = {"size": a.size, "spp": a.spp, "max_bounces": a.bounces,
           "unit": "wave cycles summed over the launch's waves (instrumented build: slower than the shipped one)",
           "scenes": {}}
    for name, objs in SCENES.items():
        h = VB.scene(L, [(o.obj_file, o.mtl_file, o.pos, o.ori, o.scl) for o in objs])
        nT = L.ipt_scene_num_triangles(h)
        adj = torch.ones((a.size, a.size, 3), device="cuda")
        grad = torch.zeros((3, nT, 3), device="cuda", dtype=torch.float64)
        tang = torch.rand((max(a.ks), nT, 3), device="cuda") * 2 - 1
        tan = torch.zeros((max(a.ks), a.size, a.size, 3), device="cuda", dtype=torch.float64)
        cyc = (C.c_ulonglong * 26)()
        res = {}
        for key, K in [("adjoint_mat_dev", 0)] + [("tangent_mat_dev_K%d" % K, K) for K in a.ks]:
            for rep in range(2):  # the second launch is kept
                L.ipt_debug_phase_cycles(cyc)
                if K == 0:
                    rc = L.ipt_adjoint_mat_dev(h, C.byref(p), None, None, None, adj.data_ptr(), grad.data_ptr(), st)
                else:
                    rc = L.ipt_tangent_mat_dev(h, C.byref(p), None, None, None, K, tang.data_ptr(), tang.data_ptr(),
                                               tang.data_ptr(), tan.data_ptr(), st)
                assert rc == 0, N.last_error()
                torch.cuda.synchronize()
                L.ipt_debug_phase_cycles(cyc)
            v = list(cyc)
            res[key] = {"cycles_total": sum(v[:6]), **{n: v[i] for i, n in enumerate(PHASES)},
                        "sweep_rounds": v[21], "sweep_tasks": v[20]}
        out["scenes"][name] = res
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phases", metavar="LIB", help="phase split from an IPT_PHASE_TIMING build instead of the timing")
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tangent", "tangent_cost.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=4)
    a = ap.parse_args()
    if a.phases:
        if a.out.endswith("tangent_cost.json"):
            a.out = os.path.join(os.path.dirname(a.out), "phase_split.json")
        return phase_split(a)
    torch.cuda.set_device(0)
    L = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    out = {"size": a.size, "spp": a.spp, "max_bounces": a.bounces, "launches": a.launches, "warmup": a.warmup,
           "timer": "HIP events per launch, the variants alternated on one stream", "scenes": {}}
    for name, objs in SCENES.items():
        S = Scene(objs)
        p = N.make_params(a.size, a.size, a.spp, a.bounces, 0)
        gen = torch.Generator(device="cuda").manual_seed(1)
        adj = torch.rand((a.size, a.size, 3), device="cuda", generator=gen) + 0.5
        grad = torch.zeros((3, S.nT, 3), device="cuda", dtype=torch.float64)
        kmax = max(a.ks)
        tang = [torch.rand((kmax, S.nT, 3), device="cuda", generator=gen) * 2 - 1 for _ in range(3)]
        tan = torch.zeros((kmax, a.size, a.size, 3), device="cuda", dtype=torch.float64)

        def adjoint():
            N.check(L.ipt_adjoint_mat_dev(S.handle, C.byref(p), None, None, None, adj.data_ptr(), grad.data_ptr(),
                                          stream), "adjoint_mat_dev")

        def tangent(K):
            def run():
                N.check(L.ipt_tangent_mat_dev(S.handle, C.byref(p), None, None, None, K, tang[0].data_ptr(),
                                              tang[1].data_ptr(), tang[2].data_ptr(), tan.data_ptr(), stream),
                        "tangent_mat_dev")
            return run

        variants = [("adjoint_mat_dev", adjoint)] + [("tangent_mat_dev_K%d" % K, tangent(K)) for K in a.ks]
        times = {k: [] for k, _ in variants}
        for i in range(a.warmup + a.launches):
            for key, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    times[key].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        out["scenes"][name] = {
            "nT": S.nT, "nE": S.nE,
            **{k + "_ms": {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
            **{"tangent_K%d_over_adjoint" % K: med["tangent_mat_dev_K%d" % K] / med["adjoint_mat_dev"] for K in a.ks},
        }
        S.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
