"""Cost of the views x material sets launches (ipt_render_views_batch_dev /
ipt_adjoint_views_batch_dev: S material sets through V cameras in ONE launch,
DESIGN.md §20) against what could run the same (set, view) pairs before: S
consecutive views launches (ipt_render_views_dev / ipt_adjoint_views_dev, one
material set each), and ONE material-batch launch of S * V sets
(ipt_render_mat_batch_dev / ipt_adjoint_mat_batch_dev: the same sample count
through the scene's own camera, the natural yardstick):

    python tools/views_batch_cost.py [--shapes 4x3 13x3] [--size 256] [--spp 32] [--launches 30] [--warmup 5]

writes profiles/views_batch/views_batch_cost.json (--out).  HIP events around
each variant on one stream, the variants alternated so that clock and thermal
drift hit all alike; medians and ratios per scene (scene_a: Cornell + the Phong
cube, the SPEC instances; cornell: the diffuse ones) and (S, V).  The views are
tools/views_cost.py's; every set carries the scene's own values (NULL arrays: the
launch still replicates kd per set, as the material batch does).
"""

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from inverse_path_tracer_amd import _native as N  # noqa: E402
from inverse_path_tracer_amd.scene import ObjectSpec, Scene, camera_at, camera_look_at  # noqa: E402

ASSETS = os.path.join(ROOT, "assets")
CORNELL = [ObjectSpec(os.path.join(ASSETS, "CornellBox", "CornellBox-Empty-CO.obj"),
                      os.path.join(ASSETS, "CornellBox", "CornellBox-Empty-CO.mtl"), (0, 0, 4), (0, 0, 0), (2, 2, 2))]
SCENES = {
    "scene_a": CORNELL + [ObjectSpec(os.path.join(ASSETS, "phong", "cube_phong.obj"),
                                     os.path.join(ASSETS, "phong", "cube_phong.mtl"), (0, -1.5, 4), (0, 0, 0),
                                     (1, 1, 1))],
    "cornell": CORNELL,
}


def cameras(sc, V):
    """View 0: the scene's own; view b: moved on a small circle and turned towards the room's middle."""
    cams = [sc.camera()]
    for b in range(1, V):
        t = 2 * np.pi * b / V
        eye = np.array([0.8 * np.cos(t), 0.5 * np.sin(t), 0.3 * (b % 3)], np.float32)
        cams.append(camera_at(camera_look_at((0, 0, 0), np.array([0, 0, 4], np.float32) - eye, (0, 1, 0)), eye))
    return np.stack(cams)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4x3", "13x3"], help="SxV: material sets x views")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_batch", "views_batch_cost.json"))
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--bounces", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = N.lib()
    stream = torch.cuda.current_stream().cuda_stream
    frame = a.size * a.size * a.spp
    out = {"size": a.size, "spp": a.spp, "max_bounces": a.bounces, "launches": a.launches, "warmup": a.warmup,
           "timer": "HIP events per variant, the variants alternated on one stream", "scenes": {}}
    for name, objs in SCENES.items():
        sc = Scene(objs)
        nT = sc.nT
        out["scenes"][name] = {"nT": nT, "nE": sc.nE}
        for shape in a.shapes:
            S, V = (int(x) for x in shape.split("x"))
            views = sc.views(cameras(sc, V))
            gen = torch.Generator(device="cuda").manual_seed(1)
            adj = torch.rand((S, V, a.size, a.size, 3), device="cuda", generator=gen) + 0.5
            hdr = torch.empty((S, V, a.size, a.size, 3), device="cuda")
            g_p = torch.zeros((S, 3, nT, 3), device="cuda", dtype=torch.float64)
            g_v = torch.zeros((S, 3, nT, 3), device="cuda", dtype=torch.float64)
            g_b = torch.zeros((S * V, 3, nT, 3), device="cuda", dtype=torch.float64)
            p = N.make_params(a.size, a.size, a.spp, a.bounces, 0)
            ps = [N.make_params(a.size, a.size, a.spp, a.bounces, s * V * frame) for s in range(S)]

            def render_pairs():
                N.check(L.ipt_render_views_batch_dev(sc.handle, views.handle, C.byref(p), S, frame, None, None, None,
                                                     hdr.data_ptr(), stream), "render_views_batch")

            def render_views():
                for s in range(S):
                    N.check(L.ipt_render_views_dev(sc.handle, views.handle, C.byref(ps[s]), frame, None, None, None,
                                                   hdr[s].data_ptr(), stream), "render_views")

            def render_batch():
                N.check(L.ipt_render_mat_batch_dev(sc.handle, C.byref(p), S * V, frame, None, None, None,
                                                   hdr.data_ptr(), stream), "render_mat_batch")

            def adjoint_pairs():
                N.check(L.ipt_adjoint_views_batch_dev(sc.handle, views.handle, C.byref(p), S, frame, None, None, None,
                                                      adj.data_ptr(), g_p.data_ptr(), stream), "adjoint_views_batch")

            def adjoint_views():
                for s in range(S):
                    N.check(L.ipt_adjoint_views_dev(sc.handle, views.handle, C.byref(ps[s]), frame, None, None, None,
                                                    adj[s].data_ptr(), g_v[s].data_ptr(), stream), "adjoint_views")

            def adjoint_batch():
                N.check(L.ipt_adjoint_mat_batch_dev(sc.handle, C.byref(p), S * V, frame, None, None, None,
                                                    adj.data_ptr(), g_b.data_ptr(), stream), "adjoint_mat_batch")

            variants = (("render_views_batch_dev", render_pairs), ("render_views_dev_x_sets", render_views),
                        ("render_mat_batch_dev", render_batch), ("adjoint_views_batch_dev", adjoint_pairs),
                        ("adjoint_views_dev_x_sets", adjoint_views), ("adjoint_mat_batch_dev", adjoint_batch))
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
            out["scenes"][name]["S=%d,V=%d" % (S, V)] = {
                **{k + "_ms": {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
                "render_pairs_over_views_launches": med["render_views_batch_dev"] / med["render_views_dev_x_sets"],
                "render_pairs_over_mat_batch": med["render_views_batch_dev"] / med["render_mat_batch_dev"],
                "adjoint_pairs_over_views_launches": med["adjoint_views_batch_dev"] / med["adjoint_views_dev_x_sets"],
                "adjoint_pairs_over_mat_batch": med["adjoint_views_batch_dev"] / med["adjoint_mat_batch_dev"],
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
