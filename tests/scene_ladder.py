"""Generated mid-size scenes for the tests: the Cornell box plus `n_tri` free-floating triangles ("shards").

The hand-made test scenes have 18..43 or 1298+ triangles and at most 2 emitters past 43.  The host code picks another
kernel instance or another LDS layout at 32/33 triangles (unrolled pair loop, shading tables), 16/17 emitters (shading
tables; the BVH instances' emitter records), 39/40 (graph bins in LDS), 63/64 (brute force / BVH), 512/513 (Kd and
tangent tables, gradient bins all in LDS) and 128 wide BVH nodes (the tree staged in LDS).  RUNGS puts one scene on
either side of each; tests/test_scene_ladder.py checks them on the CPU, tests/test_gpu_scene_ladder.py runs them.

A plain helper module (no fixtures): shards() writes the files, records() builds a rung by name.
"""
import collections
import os

import numpy as np

from conftest import CORNELL

# where the shards' centres fall: inside the Cornell box (|x|, |y| < 2, 2 < z < 6 at scale 2 around (0, 0, 4)),
# lower than the ceiling light
BOX_LO, BOX_HI = (-1.5, -1.7, 2.6), (1.5, 1.5, 5.4)
MTL = ("newmtl plain\nKd 0.6 0.7 0.5\n\n"
       "newmtl glow\nKd 0.4 0.5 0.6\nKe 3 2 1\n\n"
       "newmtl shiny\nKd 0.5 0.3 0.3\nKs 0.4 0.4 0.4\nNs 20\n")


def shards(tmp, name, n_tri, seed, n_glow=0, n_shiny=0, size=(0.25, 0.8)):
    """Writes <tmp>/<name>.obj and .mtl: n_tri triangles, each with its centre uniform in the box above and two edge
    vectors of random direction and length uniform in `size`; the first n_glow are emitters (Ke 3 2 1), the next
    n_shiny carry a Phong lobe (Ks 0.4, Ns 20), the rest are diffuse.  Returns the scene's object records: the
    Cornell box, then the shards -- nT = 18 + n_tri, nE = 2 + n_glow, lobe_mask.sum() == n_shiny."""
    assert n_glow + n_shiny <= n_tri
    rs = np.random.RandomState(seed)
    centre = rs.uniform(BOX_LO, BOX_HI, (n_tri, 3))
    edges = rs.normal(size=(n_tri, 2, 3))
    edges *= (rs.uniform(size[0], size[1], (n_tri, 2)) / np.linalg.norm(edges, axis=2))[:, :, None]
    v0 = centre - edges.sum(1) / 3
    obj, mtl = os.path.join(str(tmp), name + ".obj"), os.path.join(str(tmp), name + ".mtl")
    with open(mtl, "w") as f:
        f.write(MTL)
    with open(obj, "w") as f:
        f.write("mtllib %s.mtl\n" % name)
        for v in np.stack([v0, v0 + edges[:, 0], v0 + edges[:, 1]], axis=1).reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % tuple(v))
        for i in range(n_tri):
            f.write("usemtl %s\n" % ("glow" if i < n_glow else "shiny" if i < n_glow + n_shiny else "plain"))
            f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return CORNELL + [((0, 0, 0), (0, 0, 0), (1, 1, 1), obj, mtl)]


# nT, nE and lobe triangles of the whole scene; the generator's seed and size
Rung = collections.namedtuple("Rung", "nT nE lobes seed size")


def R(nT, nE, lobes, seed=None, size=(0.25, 0.8)):
    return Rung(nT, nE, lobes, 100 + nT if seed is None else seed, size)


RUNGS = {
    "31-2-0": R(31, 2, 0),        # the last odd count of the unrolled pair loop; shading tables
    "32-16-0": R(32, 16, 0),      # both limits of the shading tables, the last unrolled count
    "33-17-0": R(33, 17, 0),      # one past all three
    "32-2-8": R(32, 2, 8),        # the SPEC shading instance at the limit
    "39-2-0": R(39, 2, 0),        # graph bins: the last count in LDS at 2 emitters ...
    "40-2-0": R(40, 2, 0),        # ... and the first in global memory
    "63-2-0": R(63, 2, 0),        # the last brute-force scene in auto mode
    "64-2-0": R(64, 2, 0),        # the first BVH scene
    "64-16-0": R(64, 16, 0),      # BVH, the emitters' records in LDS at their limit
    "65-17-8": R(65, 17, 8),      # BVH x SPEC, the emitters' records read from global memory
    # the middle of the band: BVH + Kd tables + all gradient bins in LDS, SPEC (seed 400 leaves 0.47 of the lobe rows
    # with a gradient on the bounded material frame, 403 leaves 0.59)
    "300-22-100": R(300, 22, 100, seed=403),
    "512-2-0": R(512, 2, 0),      # the last count with Kd tables and all bins in LDS
    "513-2-0": R(513, 2, 0),      # the first with the hot set and Kd from global memory
    # the same limit with SPEC; smaller shards, so that half of the lobe rows get a gradient on the smallest frame
    "512-8-256": R(512, 8, 256, size=(0.15, 0.5)),
    "513-32-200": R(513, 32, 200, size=(0.15, 0.5)),
    "450-2-300": R(450, 2, 300),  # host-only: the tangent launch's LDS limit (test_scene_ladder.py)
    # the wide tree on either side of 128 nodes (32 KiB of LDS); smaller shards keep the box from going dark
    "tree-fits": R(3000, 2, 0, size=(0.08, 0.25)),
    "tree-global": R(3400, 2, 0, size=(0.08, 0.25)),
}
KD_TABLE_TRIS = 512   # kMaxTableTris (ipt_hip.hip)
BVH_MIN_TRIS = 64     # IPT_BVH_MIN_TRIS
WIDE_LDS_NODES = 128  # kBvhLdsNodeBytes / sizeof(WideNode)


def records(tmp, name):
    r = RUNGS[name]
    return shards(tmp, "ladder_" + name, r.nT - 18, r.seed, r.nE - 2, r.lobes, r.size)


def named(tmp, name, known):
    """Object records by name for tests parametrised over scenes: "ladder:<rung>" is a generated scene written under
    tmp, every other name is looked up in `known`."""
    return records(tmp, name[len("ladder:"):]) if name.startswith("ladder:") else known[name]


# ipt_debug_last_launch (include/ipt.h), by name
LAUNCH_FIELDS = ("launches", "mode", "spec", "bvh", "kind", "kd_tables", "small_pairs", "grad_slots", "bvh_wide_lds",
                 "rec_lds", "lds_edges", "lds_bytes", "rec_cap", "bvh_big_lds", "emit_lds", "grid", "nT", "nE")
MODE_FWD, MODE_ADJ, MODE_GRAPH, MODE_ADJU, MODE_FWDM, MODE_ADJW = range(6)
KIND_TRACE, KIND_MATG, KIND_FWDB, KIND_VFWD, KIND_VMAT, KIND_VBFWD, KIND_VBMAT, KIND_SHADE, KIND_TANG = range(9)


def last_launch():
    """The fields of the process's last trace launch as a dict."""
    import ctypes as C

    from inverse_path_tracer_amd import _native as N

    out = (C.c_int32 * len(LAUNCH_FIELDS))()
    assert N.lib().ipt_debug_last_launch(out, len(LAUNCH_FIELDS)) == len(LAUNCH_FIELDS)
    return dict(zip(LAUNCH_FIELDS, out))


# ---------------------------------------------------------------- the frames of the GPU module
# (W, H, spp, max_bounces, seed): small and odd; None = the unbounded estimator
FRAME_4 = (24, 16, 4, 4, 31)
FRAME_U = (33, 17, 5, None, 32)
FRAME_20 = (20, 12, 3, 20, 33)
# The two tree rungs have 3000 and 3400 triangles: the 1536 paths of FRAME_4 (720 of FRAME_20) reach a fifth of
# them, short of the 0.4 of the Kd rows that test_scene_ladder.py asks of every frame.  Their bounded frames are
# larger.  The 20-bounce one is the launch that stages a 105-node tree: with 21 vertex records per lane one
# workgroup fits a CU with or without the 26.9 KiB of nodes, so the stage costs no residency (launch_bvh_pick).
TREE_FRAME_4 = (49, 33, 5, 4, 31)
TREE_FRAME_20 = (49, 33, 5, 20, 33)
TREE_RUNGS = ("tree-fits", "tree-global")
BAND = (1, 16, 3)  # rows of FRAME_4 on the two banded rungs: (begin, end, step)
BAND_RUNGS = ("33-17-0", "65-17-8")
GPU_RUNGS = tuple(n for n in RUNGS if n != "450-2-300")


def frames(name):
    """[(frame, rows or None)]: what the forward and the Kd adjoint of a rung run."""
    if name in TREE_RUNGS:
        return [(TREE_FRAME_4, None), (FRAME_U, None), (TREE_FRAME_20, None)]
    return [(FRAME_4, None), (FRAME_U, None), (FRAME_20, None)] + ([(FRAME_4, BAND)] if name in BAND_RUNGS else [])


GRAPH_RUNGS = ("39-2-0", "40-2-0", "63-2-0", "64-2-0", "300-22-100")
# the material adjoint (Kd, Ks, Ke) runs where there are glow or shiny shards, under OM.draw_values
MAT_RUNGS = tuple(n for n in GPU_RUNGS if RUNGS[n].nE > 2 or RUNGS[n].lobes)
# Under the drawn values one triangle of the ceiling light is dark, and FRAME_4 leaves 0.39 / 0.36 of the 256 / 200
# lobe rows of the two largest SPEC rungs with a gradient -- test_scene_ladder.py asks for half.  Their bounded
# material frame has the unbounded frame's 2805 paths (0.58 / 0.60).
MAT_FRAME_4_WIDE = (33, 17, 5, 4, 31)


def mat_frames(name):
    """(bounded, unbounded) frame of a rung's material adjoint."""
    return (MAT_FRAME_4_WIDE if name in ("512-8-256", "513-32-200") else FRAME_4), FRAME_U


MAT_BATCH_RUNGS = ("65-17-8", "300-22-100")
# tangents: rung -> (K, frame, tangent tables in LDS); the reference costs one oracle adjoint per pixel.  K = 16
# at 300 triangles fits the LDS with 3 vertex records per lane (147 KiB of tables and records); at 512 triangles
# it does not fit at any bounce count, and the launch reads the tangents from global memory, like 513 triangles do.
TAN_FRAME = (12, 8, 8, 4, 34)
TAN_FRAME_2 = (12, 8, 8, 2, 34)
TANGENTS = {"32-2-8": (3, TAN_FRAME, 1), "65-17-8": (3, TAN_FRAME, 1), "300-22-100": (16, TAN_FRAME_2, 1),
            "512-8-256": (16, TAN_FRAME, 0), "513-32-200": (2, TAN_FRAME, 0)}
RAY_RUNGS = ("64-2-0", "300-22-100", "513-2-0", "tree-fits", "tree-global")
