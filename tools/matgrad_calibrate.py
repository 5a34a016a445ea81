"""Reference-only calibration of the tolerances in tests/test_gpu_materials.py
(CPU oracle alone, no GPU):

    python tools/matgrad_calibrate.py

The tests check the Ks and Ke gradients by identities between the adjoint
and the forward (a five-point stencil, homogeneity in Ke).  How far such an
identity is off by rounding alone is measured here on the one gradient the
oracle has, dL/dKd, with the same frames, adjoint image and step:

  TOL_KS_MATERIAL / TOL_KS_ENTRY: the identical stencil on Kd against the
      oracle's Kd adjoint -- per material (all channels, then each channel)
      and for six single (triangle, channel) entries of the cube; scene A,
      32x32x8, mb 1..3.  Worst absolute discrepancy of each kind.
  REL_KE: scene B (scene A + a small emissive cube), mb 3: the derivative of
      F = sum(adj * I) along t -> t * Kd_A at t = 1 (the same stencil)
      against sum(Kd_A * gKd_A), per object A, as a fraction of |F|.

The tests use 8x these figures.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib  # noqa: E402
from conftest import ASSETS, CORNELL, CUBE_OBJ  # noqa: E402

W = H = 32
SPP, SEED, STEP = 8, 11, 0.125
ADJ = np.random.RandomState(7).uniform(0.5, 1.5, (H, W, 3)).astype(np.float32)
PHONG = (os.path.join(ASSETS, "phong", "cube_phong.obj"), os.path.join(ASSETS, "phong", "cube_phong.mtl"))
SCENE_A = CORNELL + [((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1)) + PHONG]


def loss(Q, mb):
    s, _ = Q.render_samples(W, H, SPP, mb, SEED)
    hdr, _ = oracle_lib.pixel_mean(s, W * H, SPP)
    return float((ADJ.reshape(-1, 3).astype(np.float64) * hdr.astype(np.float64)).sum())


def stencil(f, h=STEP):
    return (8 * (f(h) - f(-h)) - (f(2 * h) - f(-2 * h))) / (12 * h)


def with_kd(Q, kd0, kd, mb):
    Q.set_materials(kd)
    v = loss(Q, mb)
    Q.set_materials(kd0)
    return v


def materials(kd):
    groups = {}
    for i, k in enumerate(tuple(r) for r in kd):
        groups.setdefault(k, []).append(i)
    return list(groups.values())


def main():
    oracle_lib.build()
    Q = oracle_lib.OracleScene(SCENE_A)
    kd0 = Q.get_materials()
    worst_mat = worst_ent = 0.0
    for mb in (1, 2, 3):
        g = Q.adjoint(W, H, SPP, mb, SEED, ADJ)
        for idx in materials(kd0):
            for d in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                def f(t):
                    kd = kd0.copy()
                    kd[idx] += np.float32(t) * np.float32(d)
                    return with_kd(Q, kd0, kd, mb)
                worst_mat = max(worst_mat, abs(stencil(f) - float((g[idx] * np.float64(d)).sum())))
        cube = list(range(18, Q.nT))
        for ti, c in [(cube[0], 0), (cube[3], 1), (cube[5], 2), (cube[6], 0), (cube[8], 1), (cube[11], 2)]:
            def f(t):
                kd = kd0.copy()
                kd[ti, c] += np.float32(t)
                return with_kd(Q, kd0, kd, mb)
            worst_ent = max(worst_ent, abs(stencil(f) - g[ti, c]))
    print("Kd stencil vs oracle adjoint, worst absolute discrepancy: per material %.3e, single entries %.3e"
          % (worst_mat, worst_ent))

    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "glow.mtl"), "w") as fh:
        fh.write("newmtl glow\nKd 0.4 0.4 0.4\nKe 3 2 1\n")
    src = open(CUBE_OBJ).read()
    i = src.index("\nf ") + 1
    with open(os.path.join(tmp, "glow.obj"), "w") as fh:
        fh.write(src[:i] + "mtllib glow.mtl\nusemtl glow\n" + src[i:])
    B = SCENE_A + [((1.0, 0.5, 4.5), (0, 0.5, 0), (0.3, 0.3, 0.3), os.path.join(tmp, "glow.obj"),
                    os.path.join(tmp, "glow.mtl"))]
    QB = oracle_lib.OracleScene(B)
    kdb = QB.get_materials()
    g = QB.adjoint(W, H, SPP, 3, SEED, ADJ)
    F = loss(QB, 3)
    worst = 0.0
    for idx in materials(kdb):
        def f(t):
            kd = kdb.copy()
            kd[idx] = (kd[idx].astype(np.float64) * (1 + t)).astype(np.float32)
            return with_kd(QB, kdb, kd, 3)
        worst = max(worst, abs(stencil(f) - float((kdb[idx].astype(np.float64) * g[idx]).sum())) / abs(F))
    print("sum(Kd_A * gKd_A) vs the stencil along Kd_A, worst discrepancy: %.3e of |F| (F = %.6g)" % (worst, F))


if __name__ == "__main__":
    main()
