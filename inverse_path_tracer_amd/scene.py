"""Scene: the reference's scene-file format and a handle on the native scene.

Scene text format (ipt_cuda.py:17-59, 91-107): blocks introduced by a line
``OBJECT``, each with optional ``POS x y z``, ``ORI x y z`` (axis*angle),
``SCL x y z`` and mandatory ``OBJ path`` and ``MTL path-or-*Kd r g b*``.
Paths are resolved like the reference (relative to the current directory);
``Scene.from_file`` also accepts a ``root`` to resolve them against.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N


@dataclass
class ObjectSpec:
    """One OBJECT block (the fields of ipt_cuda.ObjParams, ipt_cuda.py:61-78)."""

    obj_file: str
    mtl_file: str
    pos: Sequence[float] = (0.0, 0.0, 0.0)
    ori: Sequence[float] = (0.0, 0.0, 0.0)
    scl: Sequence[float] = (1.0, 1.0, 1.0)


def parse_object_block(text: str) -> ObjectSpec:
    """from_string (ipt_cuda.py:39-59): later keys win, defaults 0/0/1."""
    pos = ori = scl = obj = mtl = None
    for line in text.split("\n"):
        items = line.strip().split(" ")
        token, values = items[0], items[1:]
        if token == "POS":
            pos = [float(x) for x in values]
        elif token == "ORI":
            ori = [float(x) for x in values]
        elif token == "SCL":
            scl = [float(x) for x in values]
        elif token == "OBJ":
            obj = values[0]
        elif token == "MTL":
            mtl = " ".join(values)
    if obj is None or mtl is None:
        raise ValueError("OBJECT block without OBJ/MTL: %r" % text)
    return ObjectSpec(obj, mtl, pos if pos is not None else [0.0] * 3, ori if ori is not None else [0.0] * 3,
                      scl if scl is not None else [1.0] * 3)


def format_object_block(obj_file: str, mtl_file: str, pos=None, ori=None, scl=None) -> str:
    """Inverse of parse_object_block in the reference's spelling (ipt_cuda.py:17-37
    to_string): optional POS/ORI/SCL lines with each value printed by str(),
    then OBJ and MTL."""
    keys = (("POS", pos), ("ORI", ori), ("SCL", scl))
    head = "".join("%s %s\n" % (k, " ".join(str(x) for x in v[:3])) for k, v in keys if v is not None)
    return head + "OBJ %s\nMTL %s\n" % (obj_file, mtl_file)


def inline_kd(kd: Sequence[float]) -> str:
    """The inline material string ``*Kd r g b*`` (ipt_cuda.py:14-15)."""
    return "*Kd %s*" % " ".join(str(x) for x in kd)


def parse_scene_text(text: str) -> List[ObjectSpec]:
    """load_params (ipt_cuda.py:91-107)."""
    objects, cur = [], ""
    for line in text.splitlines(True):
        line = line.strip()
        if line == "OBJECT":
            if len(cur) > 0:
                objects.append(parse_object_block(cur))
            cur = ""
        else:
            cur += line + "\n"
    objects.append(parse_object_block(cur))
    return objects


def _resolve(path: str, roots: Sequence[str]) -> str:
    if path.startswith("*") or os.path.isabs(path):
        return path
    for r in roots:
        cand = os.path.normpath(os.path.join(r, path))
        if os.path.exists(cand):
            return cand
    return path


class Scene:
    """A scene loaded on the current HIP device (loadScene, scene.h:177-193)."""

    def __init__(self, objects: Sequence[ObjectSpec], device: bool = True):
        L = N.lib()
        n = len(objects)
        self.objects = list(objects)
        pos = np.array([o.pos for o in objects], np.float32).reshape(n, 3)
        ori = np.array([o.ori for o in objects], np.float32).reshape(n, 3)
        scl = np.array([o.scl for o in objects], np.float32).reshape(n, 3)
        objs = (C.c_char_p * n)(*[o.obj_file.encode() for o in objects])
        mtls = (C.c_char_p * n)(*[o.mtl_file.encode() for o in objects])
        h = C.c_void_p(0)
        load = L.ipt_load_scene if device else L.ipt_load_scene_host
        nT = load(n, pos.ctypes.data_as(N.fp), ori.ctypes.data_as(N.fp), scl.ctypes.data_as(N.fp),
                              objs, mtls, C.byref(h))
        if nT < 0:
            raise N.NativeError("loadScene failed: %s" % N.last_error())
        self.handle = h
        self.nT = nT
        self.nE = L.ipt_scene_num_emissives(h)
        # the lobe flags are fixed here, from the MTL values (a later set_material_params may zero a lobe's Ks)
        self._lobe_mask = (self.material_params()[1] != 0).any(axis=1)

    @classmethod
    def from_file(cls, path: str, root: Optional[str] = None, device: bool = True) -> "Scene":
        with open(path) as f:
            objects = parse_scene_text(f.read())
        roots = [root] if root else []
        roots += [os.getcwd(), os.path.dirname(os.path.dirname(os.path.abspath(path))),
                  os.path.dirname(os.path.abspath(path))]
        for o in objects:
            o.obj_file = _resolve(o.obj_file, roots)
            o.mtl_file = _resolve(o.mtl_file, roots)
        return cls(objects, device=device)

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            N.lib().freeScene(self.handle)
            self.handle = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------- materials
    @property
    def materials(self) -> np.ndarray:
        """Per-triangle diffuse Kd, (nT, 3) float32 (getMaterials)."""
        out = np.zeros((self.nT, 3), np.float32)
        N.check(N.lib().ipt_scene_get_materials(self.handle, out.ctypes.data_as(N.fp)), "getMaterials")
        return out

    @materials.setter
    def materials(self, kd):
        kd = np.ascontiguousarray(np.asarray(kd, np.float32).reshape(self.nT, 3))
        N.check(N.lib().ipt_scene_set_materials(self.handle, kd.ctypes.data_as(N.fp)), "setMaterials")

    def material_params(self):
        """(kd, ks, ke, ns): per-triangle diffuse, specular and emitted colour,
        (nT, 3) float32 each, and the Phong exponent (nT,)."""
        kd, ks, ke = (np.zeros((self.nT, 3), np.float32) for _ in range(3))
        ns = np.zeros(self.nT, np.float32)
        N.check(N.lib().ipt_scene_get_material_params(self.handle, kd.ctypes.data_as(N.fp), ks.ctypes.data_as(N.fp),
                                                      ke.ctypes.data_as(N.fp), ns.ctypes.data_as(N.fp)),
                "get_material_params")
        return kd, ks, ke, ns

    def set_material_params(self, kd=None, ks=None, ke=None):
        """Replace material VALUES (None: keep).  Structure is frozen at load:
        ke rows outside emitter_mask and ks rows outside lobe_mask are ignored
        and stay 0."""
        arrs = [None if v is None else np.ascontiguousarray(np.asarray(v, np.float32).reshape(self.nT, 3))
                for v in (kd, ks, ke)]
        ptrs = [None if a is None else a.ctypes.data_as(N.fp) for a in arrs]
        N.check(N.lib().ipt_scene_set_material_params(self.handle, *ptrs), "set_material_params")

    @property
    def emitter_mask(self) -> np.ndarray:
        """bool (nT,): the triangles on the emitter list built at load (the only rows Ke acts on)."""
        return self.triangles()[:, 56] >= 0

    @property
    def lobe_mask(self) -> np.ndarray:
        """bool (nT,): the triangles that carried a Phong lobe (Ks != 0) at load (the only rows Ks acts on)."""
        return self._lobe_mask.copy()

    def triangles(self) -> np.ndarray:
        out = np.zeros((self.nT, N.TRI_EXPORT_STRIDE), np.float32)
        N.check(N.lib().ipt_scene_export_triangles(self.handle, out.ctypes.data_as(N.fp)), "export")
        return out

    def camera(self) -> np.ndarray:
        out = np.zeros(16, np.float32)
        N.check(N.lib().ipt_scene_camera(self.handle, out.ctypes.data_as(N.fp)), "camera")
        return out.reshape(4, 4)

    # ---------------------------------------------------------- acceleration
    def set_accel(self, mode: int):
        """IPT_ACCEL_AUTO / _BRUTE / _BVH (N.ACCEL_*): which closest-hit loop
        the kernels run.  Results are identical; only speed differs."""
        N.check(N.lib().ipt_scene_set_accel(self.handle, int(mode)), "set_accel")

    def bvh_info(self) -> dict:
        info = (C.c_int32 * 8)()
        has = N.lib().ipt_scene_bvh_info(self.handle, info)
        N.check(has, "bvh_info")
        return {"has_bvh": bool(has), "nodes": info[0], "pairs": info[1], "depth": info[2], "big_pairs": info[4],
                "wide_nodes": info[5], "wide_depth": info[6], "wide_tris": info[7],
                "accel": {N.ACCEL_BRUTE: "brute", N.ACCEL_BVH: "bvh"}.get(info[3], "?"),
                "status": "ok" if has else N.last_error()}

    def export_bvh(self):
        """(nodes[n,16] float32, pairs[m,40] float32, big_idx[2k] int32) --
        BvhNode / BvhPair records (scene_layout.h; child links and indices are
        int32 bits) and the large triangles tested before the traversal."""
        i = self.bvh_info()
        nodes = np.zeros((i["nodes"], 16), np.float32)
        pairs = np.zeros((i["pairs"], 40), np.float32)
        big = np.zeros(2 * i["big_pairs"], np.int32)
        N.check(N.lib().ipt_scene_export_bvh(self.handle, nodes.ctypes.data_as(N.fp), pairs.ctypes.data_as(N.fp),
                                             big.ctypes.data_as(C.POINTER(C.c_int32))), "export_bvh")
        return nodes, pairs, big

    def export_wide(self):
        """wide[n,8,8] float32: the cooperative traversal's 8-wide nodes
        (WideNode, scene_layout.h; child refs are int32 bits)."""
        n = self.bvh_info()["wide_nodes"]
        wide = np.zeros((n, 8, 8), np.float32)
        N.check(N.lib().ipt_scene_export_wide(self.handle, wide.ctypes.data_as(N.fp)), "export_wide")
        return wide

    def closest_hit(self, origins, dirs, targets=None):
        """The kernels' cast on caller rays: (t float32[n], idx int32[n])."""
        o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        n = o.shape[0]
        t = np.zeros(n, np.float32)
        idx = np.zeros(n, np.int32)
        tg = None
        if targets is not None:
            tg = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(n))
        ip = C.POINTER(C.c_int32)
        N.check(N.lib().ipt_closest_hit_host(self.handle, n, o.ctypes.data_as(N.fp), d.ctypes.data_as(N.fp),
                                             tg.ctypes.data_as(ip) if tg is not None else None,
                                             t.ctypes.data_as(N.fp), idx.ctypes.data_as(ip)), "closest_hit")
        return t, idx

    def shadow_masks(self):
        """uint32[nT, max(nE, 1)]: the shadow rays' potential-occluder pair masks."""
        m = np.zeros((self.nT, max(1, self.nE)), np.uint32)
        N.check(N.lib().ipt_scene_shadow_masks(self.handle, m.ctypes.data_as(C.POINTER(C.c_uint32))), "shadow_masks")
        return m

    def shadow_hit(self, origins, dirs, targets, sources):
        """Shadow rays as the megakernel casts them from a vertex on triangle
        sources[i] (< 0: unknown) towards emitter triangle targets[i]."""
        o = np.ascontiguousarray(np.asarray(origins, np.float32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
        n = o.shape[0]
        t = np.zeros(n, np.float32)
        idx = np.zeros(n, np.int32)
        tg = np.ascontiguousarray(np.asarray(targets, np.int32).reshape(n))
        sr = np.ascontiguousarray(np.asarray(sources, np.int32).reshape(n))
        ip = C.POINTER(C.c_int32)
        N.check(N.lib().ipt_shadow_hit_host(self.handle, n, o.ctypes.data_as(N.fp), d.ctypes.data_as(N.fp),
                                            tg.ctypes.data_as(ip), sr.ctypes.data_as(ip), t.ctypes.data_as(N.fp),
                                            idx.ctypes.data_as(ip)), "shadow_hit")
        return t, idx

    # ---------------------------------------------------------- host-memory renders
    def render_samples(self, width, height, spp, max_bounces=None, seed=0, row_begin=0, row_end=None, row_step=1):
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        out = np.zeros((p.rows * width * spp, 3), np.float32)
        N.check(N.lib().ipt_render_samples_host(self.handle, C.byref(p), out.ctypes.data_as(N.fp)), "render_samples")
        return out

    def render(self, width, height, spp, max_bounces=None, seed=0, row_begin=0, row_end=None, ldr=False, row_step=1):
        """HDR image (rows, W, 3) = per-pixel mean of the samples (+ 8-bit tonemap)."""
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        rows = p.rows
        hdr = np.zeros((rows, width, 3), np.float32)
        u8 = np.zeros((rows, width, 3), np.uint8) if ldr else None
        N.check(N.lib().ipt_render_host(self.handle, C.byref(p), hdr.ctypes.data_as(N.fp),
                                        u8.ctypes.data_as(N.u8p) if ldr else None), "render")
        return (hdr, u8) if ldr else hdr

    def adjoint(self, adj, width, height, spp, max_bounces, seed=0, row_begin=0, row_end=None, row_step=1):
        """d(sum(adj * I))/dKd as (nT, 3) float64; adj is (H, W, 3)."""
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        adj = np.ascontiguousarray(np.asarray(adj, np.float32).reshape(height, width, 3))
        g = np.zeros((self.nT, 3), np.float64)
        N.check(N.lib().ipt_adjoint_host(self.handle, C.byref(p), adj.ctypes.data_as(N.fp),
                                         g.ctypes.data_as(N.dp)), "adjoint")
        return g

    def adjoint_materials(self, adj, width, height, spp, max_bounces, seed=0, row_begin=0, row_end=None, row_step=1):
        """d(sum(adj * I))/d(Kd, Ks, Ke) as three (nT, 3) float64 arrays, from
        one launch of the material adjoint (bounded estimator only:
        max_bounces None is refused).  Rows of Ks outside lobe_mask and of Ke
        outside emitter_mask are exactly 0."""
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        adj = np.ascontiguousarray(np.asarray(adj, np.float32).reshape(height, width, 3))
        g = np.zeros((3, self.nT, 3), np.float64)
        N.check(N.lib().ipt_adjoint_mat_host(self.handle, C.byref(p), adj.ctypes.data_as(N.fp),
                                             g.ctypes.data_as(N.dp)), "adjoint_materials")
        return g[0], g[1], g[2]

    def tangent_materials(self, tkd, tks, tke, width, height, spp, max_bounces, seed=0, row_begin=0, row_end=None,
                          row_step=1):
        """Forward-mode derivatives of the HDR image along K directions in
        material space, from ONE launch (ipt_tangent_mat_host; the paths are
        traced once): tkd, tks, tke are (K, nT, 3) host arrays -- (nT, 3) means
        K = 1 -- or None (zero; at least one is given), 1 <= K <= 16.  Returns
        (K, rows, W, 3) float64: entry [k, p, c] is <``adjoint_materials`` under
        the one-hot adjoint image at p, tangent k> in channel c, to fp64
        summation order.  The scene's own material values; bounded estimator
        only.  tks rows outside lobe_mask and tke rows outside emitter_mask are
        ignored."""
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        t, K = [], None
        for name, v in (("tkd", tkd), ("tks", tks), ("tke", tke)):
            if v is not None:
                v = np.ascontiguousarray(np.asarray(v, np.float32))
                if v.ndim == 2:
                    v = v[None]
                if v.ndim != 3 or v.shape[1:] != (self.nT, 3) or (K is not None and v.shape[0] != K):
                    raise ValueError("%s must be (K, nT=%d, 3) with one K for all, got %s" % (name, self.nT, v.shape))
                K = v.shape[0]
            t.append(v)
        if K is None:
            raise N.NativeError("material tangents: give at least one of the tangent arrays tkd, tks, tke")
        out = np.zeros((K, p.rows, width, 3), np.float64)
        N.check(N.lib().ipt_tangent_mat_host(self.handle, C.byref(p), K,
                                             *[v.ctypes.data_as(N.fp) if v is not None else None for v in t],
                                             out.ctypes.data_as(N.dp)), "tangent_materials")
        return out

    def adjoint_materials_unbounded(self, adj, width, height, spp, seed=0, row_begin=0, row_end=None, row_step=1):
        """``adjoint_materials`` for the reference's own estimator (no bounce
        cap, paths end by Russian roulette or a miss): three (nT, 3) float64
        arrays from one launch of the unbounded material adjoint
        (ipt_adjoint_mat_unbounded_host).  The Kd block equals
        ``adjoint(..., max_bounces=None)``; masks as in ``adjoint_materials``."""
        p = N.make_params(width, height, spp, None, seed, row_begin, row_end, row_step)
        adj = np.ascontiguousarray(np.asarray(adj, np.float32).reshape(height, width, 3))
        g = np.zeros((3, self.nT, 3), np.float64)
        N.check(N.lib().ipt_adjoint_mat_unbounded_host(self.handle, C.byref(p), adj.ctypes.data_as(N.fp),
                                                       g.ctypes.data_as(N.dp)), "adjoint_materials_unbounded")
        return g[0], g[1], g[2]

    def adjoint_materials_batch(self, adj, kd, ks, ke, width, height, spp, max_bounces, seed=0, seed_stride=None,
                                row_begin=0, row_end=None, row_step=1):
        """``adjoint_materials`` for S material sets in ONE batched launch
        (ipt_adjoint_mat_batch_dev): adj is (S, H, W, 3) full frames, kd / ks /
        ke are (S, nT, 3) host arrays or None (the scene's own values in every
        set); set b traces seed + b * seed_stride (default: one frame of
        samples).  Returns (S, 3, nT, 3) float64, [set][Kd | Ks | Ke].  torch
        only provides the device memory."""
        adj = np.ascontiguousarray(np.asarray(adj, np.float32))
        if adj.ndim != 4 or adj.shape[1:] != (height, width, 3):
            raise ValueError("adj must be (S, H=%d, W=%d, 3), got %s" % (height, width, adj.shape))
        mats = self._materials_dev(None, kd, ks, ke, adj.shape[0])
        return self._launch("adjoint_materials_batch", "render_materials_batch", None, mats, width, height, spp,
                            max_bounces, seed, seed_stride, (row_begin, row_end, row_step), adj)

    # ---------------------------------------------------------- views (caller-supplied cameras)
    @property
    def camera_bound(self) -> float:
        """The largest |component| a view's origin may have: the acceleration
        structures are exact only inside the coordinate bound fixed at load
        (ipt_scene_camera_bound); ``views`` refuses an origin beyond it."""
        b = C.c_float(0)
        N.check(N.lib().ipt_scene_camera_bound(self.handle, C.byref(b)), "camera_bound")
        return float(b.value)

    def views(self, cams) -> "Views":
        """A handle on V cameras over this scene: cams is (V, 4, 4) float32 in
        ``camera()``'s layout (``camera_look_at``, ``camera_at``).  Validated
        once (NativeError: a non-finite or singular matrix, an origin beyond
        ``camera_bound``); works on a host-only scene too (validation only)."""
        return Views(self, cams)

    def _materials_dev(self, views, kd, ks, ke, n_sets=None, sets=True):
        """(S, device copies of the kd / ks / ke host arrays; None stays None),
        each checked against (S, nT, 3) -- S is n_sets, else the arrays' first
        extent, 1 when all are None -- or, for one set (sets False, S None),
        against (nT, 3)."""
        import torch

        if views is not None and views.scene is not self:
            raise ValueError("the views belong to another scene")
        host = [None if v is None else np.ascontiguousarray(np.asarray(v, np.float32)) for v in (kd, ks, ke)]
        S, want, text = None, (self.nT, 3), "%s must be (nT=%d, 3), got %s"
        if sets:
            given = [v for v in host if v is not None]
            S = int(n_sets) if n_sets is not None else (given[0].shape[0] if given and given[0].ndim == 3 else 1)
            want, text = (S, self.nT, 3), "%s must be (S=%d, nT=%d, 3), got %s"
        for name, v in zip(("kd", "ks", "ke"), host):
            if v is not None and v.shape != want:
                raise ValueError(text % ((name,) + want[:-1] + (v.shape,)))
        return S, [None if v is None else torch.from_numpy(v).cuda() for v in host]

    def _launch(self, what, op, views, mats, width, height, spp, max_bounces, seed, seed_stride, rows, adj=None):
        """The launch every material and view method ends in, through the route
        of torch_ops' `op` on torch's current stream: the render (V frames per
        set) or, with the host array `adj`, the adjoint (3 blocks per set), as
        a host array.  torch only provides the device memory."""
        import torch

        from . import torch_ops

        route, (S, dev) = torch_ops._ROUTES[op], mats
        p = N.make_params(width, height, spp, max_bounces, seed, *rows)
        stride = width * height * spp if seed_stride is None else int(seed_stride)
        lead = (max(S, 0),) if route.n_sets else ()
        if adj is None:
            out = torch.zeros(lead + (len(views), p.rows, width, 3), device="cuda", dtype=torch.float32)
            symbol, tail = route.render, (out.data_ptr(),)
        else:
            a = torch.from_numpy(adj).cuda()
            out = torch.zeros(lead + (3, self.nT, 3), device=a.device, dtype=torch.float64)
            symbol, tail = route.adjoint, (a.data_ptr(), out.data_ptr())
        torch_ops._launch(route, symbol, self, views, p, S, stride, dev, tail, out.device, what)
        return out.cpu().numpy()

    def render_views(self, views, width, height, spp, max_bounces=None, seed=0, seed_stride=None, kd=None, ks=None,
                     ke=None, row_begin=0, row_end=None, row_step=1):
        """HDR images (V, rows, W, 3) of every view from ONE launch
        (ipt_render_views_dev) with one material set: kd / ks / ke are (nT, 3)
        host arrays or None (the scene's own).  View b traces seed + b *
        seed_stride (default: one frame of samples, W*H*spp) and equals the
        single-camera render through its camera bit for bit.  torch only
        provides the device memory."""
        mats = self._materials_dev(views, kd, ks, ke, sets=False)
        return self._launch("render_views", "render_views", views, mats, width, height, spp, max_bounces, seed,
                            seed_stride, (row_begin, row_end, row_step))

    def adjoint_views(self, views, adj, width, height, spp, max_bounces, seed=0, seed_stride=None, kd=None, ks=None,
                      ke=None, row_begin=0, row_end=None, row_step=1):
        """d(sum over views of sum(adj[b] * I[b]))/d(Kd, Ks, Ke) as ONE
        (3, nT, 3) float64 array from one launch (ipt_adjoint_views_dev); adj
        is (V, H, W, 3) full frames.  Bounded estimator only."""
        adj = np.ascontiguousarray(np.asarray(adj, np.float32))
        if adj.shape != (len(views), height, width, 3):
            raise ValueError("adj must be (V=%d, H=%d, W=%d, 3), got %s" % (len(views), height, width, adj.shape))
        mats = self._materials_dev(views, kd, ks, ke, sets=False)
        return self._launch("adjoint_views", "render_views", views, mats, width, height, spp, max_bounces, seed,
                            seed_stride, (row_begin, row_end, row_step), adj)

    def render_views_batch(self, views, kd=None, ks=None, ke=None, width=0, height=0, spp=1, max_bounces=4, seed=0,
                           seed_stride=None, row_begin=0, row_end=None, row_step=1, n_sets=None):
        """HDR images (S, V, rows, W, 3) of S material sets through every view
        from ONE launch (ipt_render_views_batch_dev): kd / ks / ke are
        (S, nT, 3) host arrays or None (the scene's own values in every set;
        all None: give n_sets).  Pair (s, b) traces seed + (s * V + b) *
        seed_stride (default: one frame of samples) and equals view b of
        ``render_views`` with set s's arrays at that seed bit for bit.
        Bounded estimator only (max_bounces 0..62).  torch only provides the
        device memory."""
        mats = self._materials_dev(views, kd, ks, ke, n_sets)
        return self._launch("render_views_batch", "render_views_batch", views, mats, width, height, spp, max_bounces,
                            seed, seed_stride, (row_begin, row_end, row_step))

    def adjoint_views_batch(self, views, adj, kd=None, ks=None, ke=None, width=0, height=0, spp=1, max_bounces=4,
                            seed=0, seed_stride=None, row_begin=0, row_end=None, row_step=1):
        """Per material set s, d(sum over views of sum(adj[s, b] * I[s, b]))/
        d(Kd, Ks, Ke): three (S, nT, 3) float64 blocks from ONE launch
        (ipt_adjoint_views_batch_dev); adj is (S, V, H, W, 3) full frames,
        kd / ks / ke as in ``render_views_batch``.  ``out[k][s]`` equals block
        k of ``adjoint_views`` with set s's arrays at seed + s * V *
        seed_stride, to the order of the fp64 atomics."""
        adj = np.ascontiguousarray(np.asarray(adj, np.float32))
        if adj.ndim != 5 or adj.shape[1:] != (len(views), height, width, 3):
            raise ValueError("adj must be (S, V=%d, H=%d, W=%d, 3), got %s" % (len(views), height, width, adj.shape))
        mats = self._materials_dev(views, kd, ks, ke, adj.shape[0])
        g = self._launch("adjoint_views_batch", "render_views_batch", views, mats, width, height, spp, max_bounces,
                         seed, seed_stride, (row_begin, row_end, row_step), adj)
        return g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()

    def render_views_batch_unbounded(self, views, kd=None, ks=None, ke=None, width=0, height=0, spp=1, seed=0,
                                     seed_stride=None, row_begin=0, row_end=None, row_step=1, n_sets=None):
        """``render_views_batch`` for the reference's own estimator (no bounce
        cap): (S, V, rows, W, 3) from ONE launch
        (ipt_render_views_batch_unbounded_dev).  Pair (s, b) equals view b of
        ``render_views`` at ``max_bounces=None`` with set s's arrays at seed +
        (s * V + b) * seed_stride bit for bit."""
        mats = self._materials_dev(views, kd, ks, ke, n_sets)
        return self._launch("render_views_batch_unbounded", "render_views_batch_unbounded", views, mats, width, height,
                            spp, None, seed, seed_stride, (row_begin, row_end, row_step))

    def adjoint_views_batch_unbounded(self, views, adj, kd=None, ks=None, ke=None, width=0, height=0, spp=1, seed=0,
                                      seed_stride=None, row_begin=0, row_end=None, row_step=1):
        """``adjoint_views_batch`` for the reference's own estimator (no bounce
        cap): three (S, nT, 3) float64 blocks from ONE launch of the unbounded
        material adjoint over (set, view) pairs
        (ipt_adjoint_views_batch_unbounded_dev); adj is (S, V, H, W, 3) full
        frames.  With the scene's own camera as the one view, ``out[k][s]``
        equals block k of ``adjoint_materials_unbounded`` with set s's
        materials at seed + s * seed_stride, to the order of the fp64 atomics."""
        adj = np.ascontiguousarray(np.asarray(adj, np.float32))
        if adj.ndim != 5 or adj.shape[1:] != (len(views), height, width, 3):
            raise ValueError("adj must be (S, V=%d, H=%d, W=%d, 3), got %s" % (len(views), height, width, adj.shape))
        mats = self._materials_dev(views, kd, ks, ke, adj.shape[0])
        g = self._launch("adjoint_views_batch_unbounded", "render_views_batch_unbounded", views, mats, width, height,
                         spp, None, seed, seed_stride, (row_begin, row_end, row_step), adj)
        return g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()

    def view_rays(self, views, view, width, height, spp, seed, sample_index):
        """(origins, directions), (n, 3) float32 each: the camera rays of view
        `view` for the global sample indices (pixel * spp + sample), from the
        trace kernels' own generator and camera code (ipt_views_rays_host)."""
        idx = np.ascontiguousarray(np.asarray(sample_index, np.int64).reshape(-1))
        p = N.make_params(width, height, spp, 0, seed)
        org = np.zeros((idx.size, 3), np.float32)
        d = np.zeros((idx.size, 3), np.float32)
        N.check(N.lib().ipt_views_rays_host(self.handle, views.handle, int(view), C.byref(p), idx.size,
                                            idx.ctypes.data_as(C.POINTER(C.c_int64)), org.ctypes.data_as(N.fp),
                                            d.ctypes.data_as(N.fp)), "view_rays")
        return org, d

    def graph(self, target, width, height, spp, max_bounces=None, seed=0, row_begin=0, row_end=None, row_step=1):
        """createGraph: returns (acc[(nT+1)*nT, 8] float64, data[(nT+1)*nT*7] float32)."""
        p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
        target = np.ascontiguousarray(np.asarray(target, np.uint8).reshape(height, width, 3))
        acc = np.zeros(((self.nT + 1) * self.nT, N.ACC_WIDTH), np.float64)
        data = np.zeros((self.nT + 1) * self.nT * 7, np.float32)
        N.check(N.lib().ipt_graph_host(self.handle, C.byref(p), target.ctypes.data_as(N.u8p),
                                       acc.ctypes.data_as(N.dp), data.ctypes.data_as(N.fp)), "graph")
        return acc, data


def camera_look_at(eye, look, up, fov_deg=90.0, aspect=1.0) -> np.ndarray:
    """The reference's camera matrix for (eye, look direction, up, height
    angle in degrees, aspect ratio) as (4, 4) float32 (ipt_camera_look_at);
    the defaults' matrix is ``Scene.camera()`` bit for bit.  As in the
    reference the eye lands in row 3, which rays never read -- ``camera_at``
    places a camera."""
    v = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(3)) for a in (eye, look, up)]
    out = np.zeros(16, np.float32)
    N.check(N.lib().ipt_camera_look_at(v[0].ctypes.data_as(N.fp), v[1].ctypes.data_as(N.fp),
                                       v[2].ctypes.data_as(N.fp), float(fov_deg), float(aspect),
                                       out.ctypes.data_as(N.fp)), "camera_look_at")
    return out.reshape(4, 4)


def camera_at(cam, origin) -> np.ndarray:
    """A copy of the (4, 4) camera matrix whose rays start at `origin` (column
    3 of rows 0..2, the position Ray::transform reads)."""
    out = np.array(cam, np.float32).reshape(4, 4).copy()
    out[:3, 3] = np.asarray(origin, np.float32).reshape(3)
    return out


class Views:
    """V cameras over one scene (ipt_views_create): ``len()``, ``.cams``
    ((V, 4, 4) float32, a copy), ``close()``."""

    def __init__(self, scene: "Scene", cams):
        cams = np.ascontiguousarray(np.asarray(cams, np.float32))
        if cams.ndim == 2:
            cams = cams[None]
        if cams.ndim != 3 or cams.shape[1:] != (4, 4):
            raise ValueError("cams must be (V, 4, 4), got %s" % (cams.shape,))
        h = C.c_void_p(0)
        N.check(N.lib().ipt_views_create(scene.handle, cams.shape[0], cams.ctypes.data_as(N.fp), C.byref(h)),
                "views")
        self.handle, self.scene, self.cams = h, scene, cams.copy()

    def __len__(self):
        return self.cams.shape[0]

    def close(self):
        if getattr(self, "handle", None) and self.handle.value:
            N.lib().ipt_views_free(self.handle)
            self.handle = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def compress(nT: int, acc: np.ndarray) -> np.ndarray:
    """DataWrapper::compress (inv_scene.h:87-115) of fp64 bins."""
    acc = np.ascontiguousarray(acc, np.float64)
    data = np.zeros((nT + 1) * nT * 7, np.float32)
    N.check(N.lib().ipt_compress(nT, acc.ctypes.data_as(N.dp), data.ctypes.data_as(N.fp)), "compress")
    return data


def unpack_graph(nT: int, data: np.ndarray):
    """Split createGraph output like generate_data (ipt_cuda.py:153-163)."""
    size = (nT + 1) * nT
    data = np.asarray(data).astype(np.float64)
    w = data[:size].reshape(nT + 1, nT)
    pixel = data[size:size * 4].reshape(nT + 1, nT, 3)
    light = data[size * 4:].reshape(nT + 1, nT, 3)
    return w, pixel, light


def png_write(path: str, rgb: np.ndarray):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    N.check(N.lib().ipt_png_write(path.encode(), W, H, rgb.ctypes.data_as(N.u8p)), "png_write")


def png_read(path: str) -> np.ndarray:
    w, h = C.c_int(0), C.c_int(0)
    N.check(N.lib().ipt_png_read(path.encode(), C.byref(w), C.byref(h), None, 0), "png_read")
    out = np.zeros((h.value, w.value, 3), np.uint8)
    N.check(N.lib().ipt_png_read(path.encode(), C.byref(w), C.byref(h), out.ctypes.data_as(N.u8p), out.size),
            "png_read")
    return out
