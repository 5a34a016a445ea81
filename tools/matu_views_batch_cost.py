"""Cost of the unbounded views x material sets launches
(ipt_render_views_batch_unbounded_dev / ipt_adjoint_views_batch_unbounded_dev:
S material sets through V cameras in ONE launch at max_bounces = -1, DESIGN.md
§21) against what could run the same number of (set, view) pairs before them:

  * S * V single launches through the scene's own camera, ipt_render_mat_dev at
    -1 / ipt_adjoint_mat_unbounded_dev (the only unbounded material adjoint
    there was: one set, one launch, the scene's camera);
  * for rendering through the views, S launches of ipt_render_views_dev at -1;
  * as a floor, ONE unbounded Kd-only batch of S * V sets
    (ipt_render_batch_dev / ipt_adjoint_batch_dev: no Ks or Ke blocks, the
    scene's own camera).

    python tools/matu_views_batch_cost.py [--shapes 4x3 13x3] [--size 256] [--spp 32] [--launches 30] [--warmup 5]

writes profiles/matu_views_batch/cost.json (--out).  HIP events around each
variant on one stream, the variants alternated so that clock and thermal drift
hit all alike; medians and ratios per scene (scene_a: Cornell + the Phong cube,
the SPEC instances; cornell: the diffuse ones) and (S, V).  The views are
tools/views_cost.py's; every set carries the scene's own values.
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
from inverse_path_tracer_amd.scene import Scene  # noqa: E402
from tools.views_batch_cost import SCENES, cameras  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4x3", "13x3"], help="SxV: material sets x views")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matu_views_batch", "cost.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    frame = a.size * a.size * a.spp
    out = {"size": a.size, "spp": a.spp, "max_bounces": -1, "launches": a.launches, "warmup": a.warmup,
           "timer": "HIP events per variant, the variants alternated on one stream", "scenes": {}}
    for name, objs in SCENES.items():
        sc = Scene(objs)
        nT = sc.nT
        out["scenes"][name] = {"nT": nT, "nE": sc.nE}
        for shape in a.shapes:
            S, V = (int(x) for x in shape.split("x"))
            n = S * V
            views = sc.views(cameras(sc, V))
            gen = torch.Generator(device="cuda").manual_seed(1)
            adj = torch.rand((S, V, a.size, a.size, 3), device="cuda", generator=gen) + 0.5
            hdr = torch.empty((S, V, a.size, a.size, 3), device="cuda")
            kd = torch.tensor(sc.materials, device="cuda")[None].repeat(n, 1, 1).contiguous()
            g_p = torch.zeros((S, 3, nT, 3), device="cuda", dtype=torch.float64)
            g_o = torch.zeros((n, 3, nT, 3), device="cuda", dtype=torch.float64)
            g_k = torch.zeros((n, nT, 3), device="cuda", dtype=torch.float64)
            p = N.make_params(a.size, a.size, a.spp, None, 0)
            pp = [N.make_params(a.size, a.size, a.spp, None, i * frame) for i in range(n)]
            flat_h, flat_a = hdr.view(n, a.size, a.size, 3), adj.view(n, a.size, a.size, 3)

            def render_pairs():
                N.check(L.ipt_render_views_batch_unbounded_dev(sc.handle, views.handle, C.byref(p), S, frame, None,
                                                               None, None, hdr.data_ptr(), stream), "render pairs")

            def render_own():
                for i in range(n):
                    N.check(L.ipt_render_mat_dev(sc.handle, C.byref(pp[i]), None, None, None, flat_h[i].data_ptr(),
                                                 None, stream), "render_mat")

            def render_views():
                for s in range(S):
                    N.check(L.ipt_render_views_dev(sc.handle, views.handle, C.byref(pp[s * V]), frame, None, None,
                                                   None, hdr[s].data_ptr(), stream), "render_views")

            def render_kd_batch():
                N.check(L.ipt_render_batch_dev(sc.handle, C.byref(p), n, frame, kd.data_ptr(), hdr.data_ptr(),
                                               stream), "render_batch")

            def adjoint_pairs():
                N.check(L.ipt_adjoint_views_batch_unbounded_dev(sc.handle, views.handle, C.byref(p), S, frame, None,
                                                                None, None, adj.data_ptr(), g_p.data_ptr(), stream),
                        "adjoint pairs")

            def adjoint_own():
                for i in range(n):
                    N.check(L.ipt_adjoint_mat_unbounded_dev(sc.handle, C.byref(pp[i]), None, None, None,
                                                            flat_a[i].data_ptr(), g_o[i].data_ptr(), stream),
                            "adjoint_mat_unbounded")

            def adjoint_kd_batch():
                N.check(L.ipt_adjoint_batch_dev(sc.handle, C.byref(p), n, frame, kd.data_ptr(), adj.data_ptr(),
                                                g_k.data_ptr(), stream), "adjoint_batch")

            variants = (("render_views_batch_unbounded_dev", render_pairs), ("render_mat_dev_x_pairs", render_own),
                        ("render_views_dev_x_sets", render_views), ("render_batch_dev_kd_only", render_kd_batch),
                        ("adjoint_views_batch_unbounded_dev", adjoint_pairs),
                        ("adjoint_mat_unbounded_dev_x_pairs", adjoint_own),
                        ("adjoint_batch_dev_kd_only", adjoint_kd_batch))
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
            new_r, new_a = med["render_views_batch_unbounded_dev"], med["adjoint_views_batch_unbounded_dev"]
            out["scenes"][name]["S=%d,V=%d" % (S, V)] = {
                **{k + "_ms": {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                "render_pairs_over_single_launches": new_r / med["render_mat_dev_x_pairs"],
                "render_pairs_over_views_launches": new_r / med["render_views_dev_x_sets"],
                "render_pairs_over_kd_batch": new_r / med["render_batch_dev_kd_only"],
                "adjoint_pairs_over_single_launches": new_a / med["adjoint_mat_unbounded_dev_x_pairs"],
                "adjoint_pairs_over_kd_batch": new_a / med["adjoint_batch_dev_kd_only"],
            }
            views.close()
        sc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
