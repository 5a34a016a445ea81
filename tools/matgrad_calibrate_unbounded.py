"""Reference-only calibration of the tolerances in
tests/test_gpu_materials_unbounded.py (CPU oracle alone, no GPU):

    python tools/matgrad_calibrate_unbounded.py

tools/matgrad_calibrate.py at max_bounces = None (the reference's own
estimator).  Paths are long there, so the five-point stencil is no longer
exact; how far it is off is measured on the one gradient the oracle has,
dL/dKd, with the test's frames, adjoint image, step and directions:

  TOL_KS_MATERIAL: the stencil on the cube's Kd (all channels, then each
      channel) against the oracle's unbounded Kd adjoint; scene A, 32x32x8.
  TOL_KS_ENTRY: the same for the single (triangle, channel) entries of the
      cube that the test perturbs.
  REL_KE: scene B, the derivative of F = sum(adj * I) along t -> t * Kd_A at
      t = 1 (the same stencil) against sum(Kd_A * gKd_A), per object A, as a
      fraction of |F|.

The tests use 8x these figures.
"""
import os
import tempfile

import numpy as np

import matgrad_calibrate as MC

ENTRIES = [(0, 0), (3, 1), (5, 2), (6, 0), (8, 1), (11, 2)]  # (index into the cube's triangles, channel)


def main():
    oracle_lib = MC.oracle_lib
    oracle_lib.build()
    mb = None
    Q = oracle_lib.OracleScene(MC.SCENE_A)
    kd0 = Q.get_materials()
    g = Q.adjoint(MC.W, MC.H, MC.SPP, mb, MC.SEED, MC.ADJ)
    cube = list(range(18, Q.nT))
    worst_mat = worst_ent = 0.0
    for d in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        def f(t):
            kd = kd0.copy()
            kd[cube] += np.float32(t) * np.float32(d)
            return MC.with_kd(Q, kd0, kd, mb)
        want = float((g[cube] * np.float64(d)).sum())
        err = abs(MC.stencil(f) - want)
        print("cube Kd direction %s: adjoint %.9g, stencil off by %.3e" % (d, want, err))
        worst_mat = max(worst_mat, err)
    for i, c in ENTRIES:
        ti = cube[i]

        def f(t):
            kd = kd0.copy()
            kd[ti, c] += np.float32(t)
            return MC.with_kd(Q, kd0, kd, mb)
        err = abs(MC.stencil(f) - g[ti, c])
        print("Kd entry (%d, %d): adjoint %.9g, stencil off by %.3e" % (ti, c, g[ti, c], err))
        worst_ent = max(worst_ent, err)
    print("unbounded Kd stencil vs oracle adjoint, worst absolute discrepancy: cube material %.3e, single entries %.3e"
          % (worst_mat, worst_ent))

    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "glow.mtl"), "w") as fh:
        fh.write("newmtl glow\nKd 0.4 0.4 0.4\nKe 3 2 1\n")
    src = open(MC.CUBE_OBJ).read()
    i = src.index("\nf ") + 1
    with open(os.path.join(tmp, "glow.obj"), "w") as fh:
        fh.write(src[:i] + "mtllib glow.mtl\nusemtl glow\n" + src[i:])
    B = MC.SCENE_A + [((1.0, 0.5, 4.5), (0, 0.5, 0), (0.3, 0.3, 0.3), os.path.join(tmp, "glow.obj"),
                       os.path.join(tmp, "glow.mtl"))]
    QB = oracle_lib.OracleScene(B)
    kdb = QB.get_materials()
    g = QB.adjoint(MC.W, MC.H, MC.SPP, mb, MC.SEED, MC.ADJ)
    F = MC.loss(QB, mb)
    worst = 0.0
    for idx in MC.materials(kdb):
        def f(t):
            kd = kdb.copy()
            kd[idx] = (kd[idx].astype(np.float64) * (1 + t)).astype(np.float32)
            return MC.with_kd(QB, kdb, kd, mb)
        worst = max(worst, abs(MC.stencil(f) - float((kdb[idx].astype(np.float64) * g[idx]).sum())) / abs(F))
    print("unbounded sum(Kd_A * gKd_A) vs the stencil along Kd_A, worst discrepancy: %.3e of |F| (F = %.6g)"
          % (worst, F))


if __name__ == "__main__":
    main()
