"""In-process interleaved A/B of whole libraries at C2's shape (512x512, 64 spp):
    python tools/ab_libs.py ROUNDS name=path/to/libipt_*.so ...
Each library loads its own copy of the Cornell box and scenes/0; the first
named library is the base.  A frame of every library is compared bit for bit
with the base's, then ROUNDS rounds run, in each of them every library and
every kind in turn (render = fused, 4 bounces; adj = bounded adjoint;
renderu / adju = no bounce cap), four launches per timing.  Prints per scene,
kind and library the median, min and max of the per-round means (ms) and one
JSON line.  (tools/variant_bench.py does the same for lib/variants by name,
with fewer rounds and more kinds.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import variant_bench as VB  # noqa: E402

N = VB.N


def main():
    rounds = int(sys.argv[1])
    libs = {}
    for spec in sys.argv[2:]:
        n, p = spec.split("=")
        libs[n] = VB.load(os.path.join(ROOT, p))
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for sname, recs in VB.SCENES.items():
        hs = {n: VB.scene(L, recs) for n, L in libs.items()}
        p = N.make_params(512, 512, 64, 4, 0)
        pu = N.make_params(512, 512, 64, None, 0)
        hdr = torch.empty((512 * 512, 3), device=dev)
        adj = torch.ones((512, 512, 3), device=dev)
        g = torch.zeros((8192, 3), dtype=torch.float64, device=dev)
        ref = None
        for n, L in libs.items():  # bitwise equal frames
            assert L.ipt_render_dev(hs[n], C.byref(p), None, hdr.data_ptr(), None, st) == 0
            torch.cuda.synchronize()
            h = hdr.cpu().numpy().view(np.uint32)
            if ref is None:
                ref = h.copy()
            print(sname, n, "frame", "bit-exact" if np.array_equal(h, ref) else "MISMATCH", flush=True)
        kinds = ("render", "adj", "renderu", "adju")
        times = {n: {k: [] for k in kinds} for n in libs}
        for rnd in range(rounds + 1):
            for n, L in libs.items():
                for kind in kinds:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(4):
                        if kind.startswith("render"):
                            assert L.ipt_render_dev(hs[n], C.byref(pu if kind == "renderu" else p), None, hdr.data_ptr(), None, st) == 0
                        else:
                            assert L.ipt_adjoint_dev(hs[n], C.byref(pu if kind == "adju" else p), None, adj.data_ptr(), g.data_ptr(), st) == 0
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd > 0:
                        times[n][kind].append(e0.elapsed_time(e1) / 4)
        for kind in kinds:
            base = float(np.median(times[list(libs)[0]][kind]))
            for n in libs:
                t = np.array(times[n][kind])
                out["%s:%s:%s" % (sname, kind, n)] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                                                    "max_ms": round(float(t.max()), 4)}
                print("%-8s %-8s %-8s median %.4f  min %.4f  max %.4f  vs %s %+.2f%%" % (
                    sname, kind, n, np.median(t), t.min(), t.max(), list(libs)[0], 100 * (np.median(t) / base - 1)), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
