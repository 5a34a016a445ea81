#!/usr/bin/env python3
"""Record what the Python layer asks of the native library, and what comes back.

Runs one fixed scenario through the public surface of torch_ops, Scene and
optimize with ``_native.lib()`` answering through a recording proxy, and writes
one JSON file:

  trace    every ipt_* call in order: the symbol, every field of a Params
           argument, every scalar argument, and for each pointer whether it
           is null;
  images   SHA-256 of every forward image (bit-exact from run to run);
  numbers  every gradient and every parameter after the optimizer's steps.

Two runs of one tree give the same trace and images, and numbers that differ
by the order of the fp64 atomics alone.  ``--compare A B [--margin M]`` reports
whether two files agree: traces and images exactly, numbers to the relative
margin (default: exactly).  A run's file is some hundred KiB, so what is kept
is ``--summary PARENT PARENT_2 BRANCH``: digests of each run, the spread of the
two parent runs, the margin (twice that spread) and how the branch compares.

Uses public names only, so the same file runs against any tree of the project:
    python tools/bindings_trace.py --out trace.json [--package-root DIR]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

W = H = 8
SPP, MB, S, V = 4, 2, 2, 3
BANDS = {"full": (0, None, 1), "rows-2-4-6": (2, 8, 2), "rows-3-to-6": (3, 7, 1)}
PARAM_FIELDS = ("width", "height", "spp", "max_bounces", "seed", "row_begin", "row_end", "row_step")


def describe(arg, kind, N):
    if kind is N.pp:
        p = arg._obj
        return {f: int(getattr(p, f)) for f in PARAM_FIELDS}
    if kind in (C.c_int, C.c_int32, C.c_int64, C.c_uint64):
        return int(arg)
    if kind is C.c_float:
        return float(arg)
    value = getattr(arg, "value", arg)  # c_void_p handles, integers from data_ptr(), byref(), arrays, None
    return "null" if value is None or (isinstance(value, int) and value == 0) else "ptr"


class Recorder:
    """Stands in for the loaded library: ipt_* calls are noted, then made."""

    def __init__(self, lib, N):
        self._lib, self._N, self.trace = lib, N, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("ipt_"):
            return f
        kinds = self._N.SIGNATURES[name][1]

        def call(*args):
            self.trace.append([name] + [describe(a, k, self._N) for a, k in zip(args, kinds)])
            return f(*args)
        return call


def sha(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def nums(t):
    """The values as JSON numbers that read back exactly (9 digits carry a float32, 17 a float64)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    fmt = "%.9g" if a.dtype == np.float32 else "%.17g"
    return [float(fmt % x) for x in a.reshape(-1)]


def scenario(root, tmp):
    import torch

    from inverse_path_tracer_amd import _native as N
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks
    from inverse_path_tracer_amd.scene import Scene, camera_at, camera_look_at, format_object_block

    rec = Recorder(N.lib(), N)
    N.lib = lambda: rec
    images, numbers = {}, {}
    torch.cuda.set_device(0)
    assets = os.path.join(root, "assets")
    P = Scene.from_file(os.path.join(assets, "phong", "scene0_phong.txt"))
    own = P.camera()
    side = camera_at(camera_look_at((0, 0, 0), (0.5, -0.2, 1.0), (0, 1, 0), fov_deg=60), (-0.8, 0.3, 0.5))
    cams = np.stack([own, camera_at(own, (0.3, 0.1, -0.2)), side])
    views = P.views(cams)
    kd0, ks0, ke0, _ = P.material_params()
    rs = np.random.RandomState(3)
    sets = [np.stack([m, (m * rs.uniform(0.4, 0.9, m.shape)).astype(np.float32)]) for m in (kd0, ks0, ke0)]
    one = (kd0, ks0, ke0)

    def adj_of(shape):
        return rs.uniform(0.5, 1.5, shape).astype(np.float32)

    def leaves(arrays, mode):
        """all: three leaves; mixed: kd None, ks a leaf, ke given without a gradient."""
        t = [torch.tensor(a, device="cuda") for a in arrays]
        if mode == "all":
            return [x.requires_grad_(True) for x in t]
        return [None, t[1].requires_grad_(True), t[2]]

    def run_op(tag, fn, arrays, mode, **kw):
        t = leaves(arrays, mode)
        img = fn(t, **kw)
        images[tag] = sha(img)
        (img * torch.tensor(adj_of(tuple(img.shape)), device="cuda")).sum().backward()
        for name, x in zip(("kd", "ks", "ke"), t):
            if x is not None and x.grad is not None:
                numbers["%s/d%s" % (tag, name)] = nums(x.grad)

    # ---- torch_ops: the eight public ops, forward and backward
    for mode, extra in (("all", {}), ("mixed", {"adjoint_seed": 12345})):
        for band, (rb, re_, rstep) in BANDS.items():
            rows = dict(row_begin=rb, row_end=re_, row_step=rstep)
            if mode == "all":
                run_op("render/%s" % band, lambda t, **kw: torch_ops.render(P, t[0], W, H, SPP, MB, seed=9, **kw),
                       one, mode, **rows)
            run_op("render_materials/%s/%s" % (mode, band),
                   lambda t, **kw: torch_ops.render_materials(P, t[0], t[1], t[2], W, H, SPP, MB, seed=9, **kw),
                   one, mode, **rows, **extra)
            run_op("render_materials_unbounded/%s/%s" % (mode, band),
                   lambda t, **kw: torch_ops.render_materials_unbounded(P, t[0], t[1], t[2], W, H, SPP, seed=9, **kw),
                   one, mode, **rows, **extra)
        if mode == "all":
            run_op("render_batch", lambda t, **kw: torch_ops.render_batch(P, t[0], W, H, SPP, MB, seed=9, **kw),
                   sets, mode, adjoint_seed=777)
        run_op("render_materials_batch/%s" % mode,
               lambda t, **kw: torch_ops.render_materials_batch(P, t[0], t[1], t[2], W, H, SPP, MB, seed=9, **kw),
               sets, mode, **extra)
        run_op("render_views/%s" % mode,
               lambda t, **kw: torch_ops.render_views(P, views, t[0], t[1], t[2], W, H, SPP, MB, seed=9, **kw),
               one, mode, **extra)
        run_op("render_views_batch/%s" % mode,
               lambda t, **kw: torch_ops.render_views_batch(P, views, t[0], t[1], t[2], W, H, SPP, MB, seed=9, **kw),
               sets, mode, **extra)
        run_op("render_views_batch_unbounded/%s" % mode,
               lambda t, **kw: torch_ops.render_views_batch_unbounded(P, views, t[0], t[1], t[2], W, H, SPP, seed=9,
                                                                      **kw), sets, mode, **extra)
    run_op("render_views_batch/stride",
           lambda t, **kw: torch_ops.render_views_batch(P, views, t[0], t[1], t[2], W, H, SPP, MB, seed=9, **kw),
           sets, "all", seed_stride=1000)

    # ---- Scene: the host-array methods of the material and view launches
    aS, aV, aSV = adj_of((S, H, W, 3)), adj_of((V, H, W, 3)), adj_of((S, V, H, W, 3))
    for band, (rb, re_, rstep) in BANDS.items():
        rows = dict(row_begin=rb, row_end=re_, row_step=rstep)
        for tag, m, m1 in (("sets", sets, one), ("own", (None, None, None), (None, None, None)),
                           ("ks", (None, sets[1], None), (None, ks0, None))):
            key = "scene/%s/%s/" % (tag, band)
            numbers[key + "adjoint_materials_batch"] = nums(
                P.adjoint_materials_batch(aS, m[0], m[1], m[2], W, H, SPP, MB, 9, **rows))
            images[key + "render_views"] = sha(P.render_views(views, W, H, SPP, MB, 9, None, *m1, **rows))
            numbers[key + "adjoint_views"] = nums(P.adjoint_views(views, aV, W, H, SPP, MB, 9, None, *m1, **rows))
            n = dict(n_sets=S) if tag == "own" else {}
            images[key + "render_views_batch"] = sha(
                P.render_views_batch(views, m[0], m[1], m[2], W, H, SPP, MB, 9, **rows, **n))
            numbers[key + "adjoint_views_batch"] = nums(np.stack(
                P.adjoint_views_batch(views, aSV, m[0], m[1], m[2], W, H, SPP, MB, 9, **rows)))
            images[key + "render_views_batch_unbounded"] = sha(
                P.render_views_batch_unbounded(views, m[0], m[1], m[2], W, H, SPP, 9, **rows, **n))
            numbers[key + "adjoint_views_batch_unbounded"] = nums(np.stack(
                P.adjoint_views_batch_unbounded(views, aSV, m[0], m[1], m[2], W, H, SPP, 9, **rows)))
    numbers["scene/stride/adjoint_views_batch"] = nums(np.stack(
        P.adjoint_views_batch(views, aSV, *sets, W, H, SPP, MB, 9, seed_stride=1000)))
    views.close()

    # ---- optimize: targets and two steps on each route
    kd = [float(x) for x in open(os.path.join(assets, "phong", "cube_phong.mtl")).read().split("Kd")[1].split()[:3]]
    files = []
    cornell = os.path.join(assets, "CornellBox", "CornellBox-Empty-CO")
    for i, c in enumerate((kd, [kd[2], kd[0], kd[1]])):
        mtl = os.path.join(tmp, "phong_%d.mtl" % i)
        with open(mtl, "w") as f:
            f.write("newmtl phong\nKd %r %r %r\nKs 0.5 0.5 0.5\nNs 20\n" % tuple(c))
        files.append(os.path.join(tmp, "a_%d.txt" % i))
        with open(files[-1], "w") as f:
            f.write("OBJECT\n" + format_object_block(cornell + ".obj", cornell + ".mtl", (0, 0, 4), (0, 0, 0),
                                                     (2, 2, 2)))
            f.write("OBJECT\n" + format_object_block(os.path.join(assets, "phong", "cube_phong.obj"), mtl,
                                                     (0, -1.5, 4), (0, 0, 0), (1, 1, 1)))
    dev = torch.device("cuda")
    mats = ("kd", "ks", "ke")
    routes = [("1-kd", ("kd",), None, MB, {}), ("1-kd-unbounded", ("kd",), None, None, {}),
              ("1-kd-tied", ("kd",), None, MB, {"tie_shared": 2}),
              ("2-unbounded-own", mats, None, None, {}), ("2-unbounded-views", mats, cams, None, {}),
              ("2-unbounded-views-kd", ("kd",), cams, -1, {}),
              ("3-views", mats, cams, MB, {}), ("3-views-kd", ("kd",), cams, MB, {}),
              ("4-materials", ("ks", "ke"), None, MB, {}),
              ("4-materials-same-stream", mats, None, MB, {"decorrelate": False})]
    for tag, learn, vw, mb, kw in routes:
        tasks = build_tasks(files, W, H, 2 * SPP, mb, 0.5, dev, seed=7, first_index=1, learn=learn, views=vw)
        for i, t in enumerate(tasks):
            images["optimize/%s/target%d" % (tag, i)] = sha(t.target)
        opt = MaterialOptimizer(tasks, W, H, SPP, mb, lr=0.02, seed=40, n_total=4, learn=learn, views=vw, **kw)
        for step in range(2):
            opt.step()
            for j, q in enumerate(opt.params):
                numbers["optimize/%s/step%d/grad%d" % (tag, step, j)] = nums(q.grad)
        for j, q in enumerate(opt.params):
            numbers["optimize/%s/param%d" % (tag, j)] = nums(q)
        opt.run(0)
        for i, t in enumerate(tasks):
            numbers["optimize/%s/history%d" % (tag, i)] = [float(x) for x in t.history]
        for h in [t.views for t in tasks] + list(opt.view_handles):  # the handles first, then their scenes
            if h is not None:
                h.close()
        for sc in {id(t.scene): t.scene for t in tasks}.values():
            sc.close()
    P.close()
    torch.cuda.synchronize()
    return {"trace": rec.trace, "images": images, "numbers": numbers}


def spread(a, b):
    """Largest element-wise relative difference |x - y| / max(|x|, |y|) of the numbers of two runs."""
    worst, where = 0.0, None
    assert a["numbers"].keys() == b["numbers"].keys()
    for k in a["numbers"]:
        x, y = np.asarray(a["numbers"][k], np.float64), np.asarray(b["numbers"][k], np.float64)
        assert x.shape == y.shape, k
        scale = np.maximum(np.abs(x), np.abs(y))
        rel = np.where(scale > 0, np.abs(x - y) / np.where(scale > 0, scale, 1), 0.0)
        if rel.size and rel.max() > worst:
            worst, where = float(rel.max()), k
    return worst, where


def digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def summary(parent, parent_2, branch):
    """What is kept of three runs: per run, the size and SHA-256 of its trace (canonical JSON, so equal
    digests are equal traces, call for call and in order), of its image hashes and of its numbers; the
    parent's run-to-run spread, the margin, and the branch against each parent run."""
    runs = {"parent": parent, "parent_2": parent_2, "branch": branch}
    out = {"runs": {}}
    for name, r in runs.items():
        calls = {}
        for c in r["trace"]:
            calls[c[0]] = calls.get(c[0], 0) + 1
        out["runs"][name] = {"calls": len(r["trace"]), "trace_sha256": digest(r["trace"]), "calls_per_symbol": calls,
                             "images": len(r["images"]), "images_sha256": digest(r["images"]),
                             "number_arrays": len(r["numbers"]),
                             "numbers": sum(len(v) for v in r["numbers"].values()),
                             "numbers_sha256": digest(r["numbers"])}

    def against(a, b):
        worst, where = spread(a, b)
        return {"traces_identical": a["trace"] == b["trace"], "images_identical": a["images"] == b["images"],
                "largest_relative_difference": worst, "where": where,
                "arrays_that_differ": sorted(k for k in a["numbers"] if a["numbers"][k] != b["numbers"].get(k))}
    out["parent_vs_parent_2"] = against(parent, parent_2)
    out["margin"] = 2 * out["parent_vs_parent_2"]["largest_relative_difference"]
    for name in ("parent", "parent_2"):
        out["branch_vs_" + name] = against(runs[name], branch)
    out["equivalent"] = all(out[k]["traces_identical"] and out[k]["images_identical"] for k in out if "_vs_" in k) and \
        all(out["branch_vs_" + n]["largest_relative_difference"] <= out["margin"] for n in ("parent", "parent_2"))
    return out


def compare(a, b, margin):
    ok = True
    if a["trace"] != b["trace"]:
        ok = False
        first = next((i for i, (x, y) in enumerate(zip(a["trace"], b["trace"])) if x != y),
                     min(len(a["trace"]), len(b["trace"])))
        print("traces differ at call %d (%d and %d calls)" % (first, len(a["trace"]), len(b["trace"])))
        for t in (a["trace"], b["trace"]):
            print("   ", t[first] if first < len(t) else None)
    else:
        print("traces identical: %d calls" % len(a["trace"]))
    if a["images"] != b["images"]:
        ok = False
        print("images differ:", sorted(k for k in set(a["images"]) | set(b["images"])
                                       if a["images"].get(k) != b["images"].get(k)))
    else:
        print("image hashes identical: %d images" % len(a["images"]))
    worst, where = spread(a, b)
    n = sum(len(v) for v in a["numbers"].values())
    print("numbers: %d in %d arrays, largest relative difference %.3e (%s), margin %.3e" % (
        n, len(a["numbers"]), worst, where, margin))
    return ok and worst <= margin


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose inverse_path_tracer_amd package and assets are used")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--summary", nargs=3, metavar=("PARENT", "PARENT_2", "BRANCH"))
    ap.add_argument("--margin", type=float, default=0.0)
    args = ap.parse_args()
    if args.summary:
        out = summary(*(json.load(open(p)) for p in args.summary))
        print(json.dumps(out, indent=1))
        return 0 if out["equivalent"] else 1
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        return 0 if compare(a, b, args.margin) else 1
    root = os.path.abspath(args.package_root)
    sys.path.insert(0, root)
    with tempfile.TemporaryDirectory() as tmp:
        out = scenario(root, tmp)
    with open(args.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%d calls, %d images, %d number arrays -> %s" % (len(out["trace"]), len(out["images"]),
                                                            len(out["numbers"]), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
