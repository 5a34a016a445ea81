"""Cost of the batched material adjoint (ipt_adjoint_mat_batch_dev: dL/dKd,
dL/dKs, dL/dKe of S material sets in one launch) against the two ways the
same work ran before it: S consecutive ipt_adjoint_mat_dev launches, and the
Kd-only batch ipt_adjoint_batch_dev (which returns a third of the gradient):

    python tools/matbatch_cost.py [--sets 13] [--size 256] [--spp 32] [--launches 30] [--warmup 5] > matbatch_cost.json

HIP events around each variant on one stream, the three alternated so that
clock and thermal drift hit all alike; medians and ratios per scene (scene_a:
Cornell + the Phong cube, the SPEC instances; cornell: the diffuse ones).  The
default shape is C5's: 13 sets at 256 x 256 x 32, 4 bounces.
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
    "scene_a": CORNELL + [ObjectSpec(os.path.join(ASSETS, "phong", "cube_phong.obj"),
                                     os.path.join(ASSETS, "phong", "cube_phong.mtl"), (0, -1.5, 4), (0, 0.3, 0),
                                     (1, 1, 1))],
    "cornell": CORNELL,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=13)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    S, frame = a.sets, a.size * a.size * a.spp
    out = {"sets": S, "size": a.size, "spp": a.spp, "max_bounces": a.bounces, "launches": a.launches,
           "warmup": a.warmup, "timer": "HIP events per variant, the variants alternated on one stream",
           "scenes": {}}
    for name, objs in SCENES.items():
        sc = Scene(objs)
        nT = sc.nT
        kd0, ks0, ke0, _ = sc.material_params()
        gen = torch.Generator(device="cuda").manual_seed(1)
        # per-set values around the scene's own, inside the masks
        jit = [torch.rand((S, nT, 3), device="cuda", generator=gen) * 0.2 + 0.9 for _ in range(3)]
        kd, ks, ke = ((torch.tensor(v, device="cuda")[None] * j).clamp(0, None).contiguous()
                      for v, j in zip((kd0, ks0, ke0), jit))
        kd.clamp_(0, 1)
        ks.clamp_(0, 1)
        adj = torch.rand((S, a.size, a.size, 3), device="cuda", generator=gen) + 0.5
        g_kd = torch.zeros((S, nT, 3), device="cuda", dtype=torch.float64)
        g_mb = torch.zeros((S, 3, nT, 3), device="cuda", dtype=torch.float64)
        g_ms = torch.zeros((S, 3, nT, 3), device="cuda", dtype=torch.float64)
        p = N.make_params(a.size, a.size, a.spp, a.bounces, 0)
        ps = [N.make_params(a.size, a.size, a.spp, a.bounces, b * frame) for b in range(S)]

        def kd_batch():
            N.check(L.ipt_adjoint_batch_dev(sc.handle, C.byref(p), S, frame, kd.data_ptr(), adj.data_ptr(),
                                            g_kd.data_ptr(), stream), "adjoint_batch")

        def mat_batch():
            N.check(L.ipt_adjoint_mat_batch_dev(sc.handle, C.byref(p), S, frame, kd.data_ptr(), ks.data_ptr(),
                                                ke.data_ptr(), adj.data_ptr(), g_mb.data_ptr(), stream),
                    "adjoint_mat_batch")

        def mat_singles():
            for b in range(S):
                N.check(L.ipt_adjoint_mat_dev(sc.handle, C.byref(ps[b]), kd[b].data_ptr(), ks[b].data_ptr(),
                                              ke[b].data_ptr(), adj[b].data_ptr(), g_ms[b].data_ptr(), stream),
                        "adjoint_mat")

        # untimed: with the scene's own Ks and Ke (NULL arrays) the Kd block is the Kd-only batch's
        N.check(L.ipt_adjoint_mat_batch_dev(sc.handle, C.byref(p), S, frame, kd.data_ptr(), None, None,
                                            adj.data_ptr(), g_mb.data_ptr(), stream), "adjoint_mat_batch")
        kd_batch()
        kd_rel = float(((g_mb[:, 0] - g_kd).abs().max() / g_kd.abs().max()).item())
        g_mb.zero_()
        g_kd.zero_()

        variants = (("adjoint_batch_dev", kd_batch), ("adjoint_mat_batch_dev", mat_batch),
                    ("adjoint_mat_dev_x_sets", mat_singles))
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
        # both accumulated the same number of launches over the same paths: the gradients must agree
        out["scenes"][name] = {
            "nT": nT, "nE": sc.nE,
            **{k + "_ms": {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
            "batch_over_single_launches": med["adjoint_mat_batch_dev"] / med["adjoint_mat_dev_x_sets"],
            "batch_over_kd_only_batch": med["adjoint_mat_batch_dev"] / med["adjoint_batch_dev"],
            "max_rel_diff_batch_vs_single_launches": float(((g_mb - g_ms).abs().max() / g_ms.abs().max()).item()),
            "max_rel_diff_kd_block_vs_kd_only_batch": kd_rel,
        }
        sc.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
