"""PyTorch-ROCm autograd op over the HIP kernels.

``render(scene, kd, ...)`` returns the HDR image (rows, W, 3) rendered with
per-triangle diffuse albedo ``kd`` (nT, 3) on the GPU; its backward runs the
adjoint kernel (path replay under common random numbers) and
returns dLoss/dkd.  PyTorch only provides device memory and the stream; all
compute is libipt_amd.so (there is no fallback).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _native as N
from .scene import Scene


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def render_into(scene: Scene, params: N.Params, kd: torch.Tensor, hdr: torch.Tensor):
    """Forward kernels on torch's current stream, into a preallocated image."""
    N.check(N.lib().ipt_render_dev(scene.handle, C.byref(params), kd.data_ptr() if kd is not None else None,
                                   hdr.data_ptr(), None, _stream(hdr.device)), "ipt_render_dev")
    return hdr


def adjoint_into(scene: Scene, params: N.Params, kd: torch.Tensor, adj_full: torch.Tensor, grad: torch.Tensor):
    """Accumulate d(sum adj*I)/dkd (fp64, nT*3) for rows [row_begin,row_end).
    ``adj_full`` is indexed by global pixel: pass the full (H, W, 3) image or a
    band pointer offset by row_begin*W*3 (see adjoint_band)."""
    N.check(N.lib().ipt_adjoint_dev(scene.handle, C.byref(params), kd.data_ptr() if kd is not None else None,
                                    adj_full, grad.data_ptr(), _stream(grad.device)), "ipt_adjoint_dev")
    return grad


def adjoint_band(scene: Scene, params: N.Params, kd, adj_band: torch.Tensor, grad: torch.Tensor):
    """Adjoint for a launch whose adjoint image holds only its own rows."""
    base, frame = _adjoint_base(adj_band.contiguous(), params)  # frame: referenced until the call has returned
    return adjoint_into(scene, params, kd, base, grad)


def _adjoint_base(adj: torch.Tensor, p: N.Params):
    """(pointer, its tensor): the launch's own rows `adj` (contiguous float32)
    as the adjoint kernels want them, indexed by global pixel.  The caller
    keeps the tensor until the native call has returned."""
    if p.row_step > 1:  # interleaved rows: scatter into a full-frame image
        full = torch.zeros((p.height, p.width, 3), device=adj.device, dtype=torch.float32)
        full[p.row_begin:p.row_end:p.row_step] = adj
        return full.data_ptr(), full
    return adj.data_ptr() - p.row_begin * p.width * 3 * 4, adj  # a full frame (row_begin 0): adj itself


class _RenderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kd, scene, params, adjoint_seed):
        kd_c = kd.detach().contiguous().float()
        hdr = torch.empty((params.rows, params.width, 3), device=kd.device, dtype=torch.float32)
        render_into(scene, params, kd_c, hdr)
        ctx.scene, ctx.params, ctx.adjoint_seed = scene, params, adjoint_seed
        ctx.save_for_backward(kd_c)
        return hdr

    @staticmethod
    def backward(ctx, grad_hdr):
        (kd_c,) = ctx.saved_tensors
        g = torch.zeros(kd_c.shape, device=kd_c.device, dtype=torch.float64)
        adjoint_band(ctx.scene, _replay_params(ctx.params, ctx.adjoint_seed), kd_c, grad_hdr.float(), g)
        return g.to(kd_c.dtype), None, None, None


def _replay_params(p: N.Params, adjoint_seed):
    """The adjoint's parameters: the forward's (common random numbers: the
    exact derivative of the returned image), or the same configuration on an
    independent sample stream (adjoint_seed: an unbiased estimate of the
    derivative of the expected image, uncorrelated with the forward's noise)."""
    if adjoint_seed is None:
        return p
    return N.Params(p.width, p.height, p.spp, p.max_bounces, int(adjoint_seed) & 0xFFFFFFFFFFFFFFFF, p.row_begin,
                    p.row_end, p.row_step)


def render(scene: Scene, kd: torch.Tensor, width: int, height: int, spp: int, max_bounces=4, seed: int = 0,
           row_begin: int = 0, row_end=None, adjoint_seed=None, row_step: int = 1) -> torch.Tensor:
    """Differentiable render: HDR image of rows row_begin, row_begin + row_step,
    ... < row_end w.r.t. kd.  max_bounces None is the reference's own
    estimator (paths end by Russian roulette or a miss); its adjoint keeps
    the vertex records in an LDS ring and replays long paths chunk by chunk.

    The backward pass replays the forward's paths (adjoint_seed None) or
    traces the same configuration with seed `adjoint_seed`.  The second form
    is what an optimiser of E[loss] wants: with the forward's own samples the
    gradient of (I - T)^2 correlates the residual with the derivative, a bias
    of order 1/spp towards darker albedo.

    Choose `adjoint_seed` so that its samples' seeds (adjoint_seed + global
    sample index) differ from the forward's in the LOW 32 bits, e.g. the
    next frame: seed + W*H*spp.  curand_init's XORWOW set-up hashes the two
    32-bit halves of a seed separately, so seeds equal mod 2^32 share three
    of the five state words and their first draws differ only by a constant
    -- correlated streams (measured: a residual bias of ~14% of the
    same-stream one, tests/test_gpu_full.py)."""
    p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
    return _RenderFn.apply(kd, scene, p, adjoint_seed)


BATCH_REFUSED = ("material adjoint: the scene batch (n_scenes > 1) is not supported by render_materials; "
                 "pass (S, nT, 3) tensors to render_materials_batch")


class _Route(NamedTuple):
    """How one public material op reaches the library: its two symbols, which
    of (views handle, n_sets, seed_stride) the launches take after the scene
    and the params, and its refusals.  N.check's `what` is the symbol."""

    name: str
    render: str
    adjoint: str
    views: bool = False
    n_sets: bool = False
    seed_stride: bool = False
    ldr: bool = False  # the render takes a trailing ldr pointer (the one-set material render alone)
    set_refused: Optional[str] = None  # one-set ops: the NativeError for an (S, nT, 3) tensor (None: a shape like any)
    unbounded_refused: Optional[str] = None  # bounded ops: the NativeError for no bounce cap


_MAT = _Route(
    "render_materials", "ipt_render_mat_dev", "ipt_adjoint_mat_dev", ldr=True, set_refused=BATCH_REFUSED,
    unbounded_refused="material adjoint: the unbounded estimator (max_bounces < 0) is not supported by "
                      "render_materials; give max_bounces in 0..62 or call render_materials_unbounded")
_ROUTES = {r.name: r for r in (
    _MAT,
    _MAT._replace(name="render_materials_unbounded", adjoint="ipt_adjoint_mat_unbounded_dev", unbounded_refused=None,
                  set_refused="unbounded material adjoint: the scene batch (n_scenes > 1) is not supported"),
    _Route("render_materials_batch", "ipt_render_mat_batch_dev", "ipt_adjoint_mat_batch_dev", n_sets=True,
           seed_stride=True,
           unbounded_refused="material adjoint: the unbounded estimator (max_bounces < 0) is not supported by the "
                             "scene batch; give max_bounces in 0..62 (one set: render_materials_unbounded)"),
    _Route("render_views", "ipt_render_views_dev", "ipt_adjoint_views_dev", views=True, seed_stride=True,
           unbounded_refused="views adjoint: the unbounded estimator (max_bounces < 0) is not supported by "
                             "render_views; give max_bounces in 0..62"),
    _Route("render_views_batch", "ipt_render_views_batch_dev", "ipt_adjoint_views_batch_dev", views=True, n_sets=True,
           seed_stride=True,
           unbounded_refused="views batch: the unbounded estimator (max_bounces < 0) is not supported by "
                             "render_views_batch; give max_bounces in 0..62"),
    _Route("render_views_batch_unbounded", "ipt_render_views_batch_unbounded_dev",
           "ipt_adjoint_views_batch_unbounded_dev", views=True, n_sets=True, seed_stride=True),
)}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _launch(route: _Route, symbol: str, scene, views, params: N.Params, n_sets, stride, mats, tail, device,
            what=None):
    """One native call of `route` on torch's current stream: the scene, the
    arguments the route takes, the three material pointers, then `tail`."""
    args = [scene.handle] + ([views.handle] if route.views else []) + [C.byref(params)]
    args += ([n_sets] if route.n_sets else []) + ([stride] if route.seed_stride else [])
    N.check(getattr(N.lib(), symbol)(*args, *[_ptr(t) for t in mats], *tail, _stream(device)), what or symbol)


def _validate(route: _Route, scene, mats, max_bounces):
    given = [t for t in mats if t is not None]
    if not given:
        raise ValueError("%s needs at least one of kd, ks, ke as a device tensor" % route.name)
    for t in given:
        if route.n_sets:
            if t.dim() != 3 or tuple(t.shape[1:]) != (scene.nT, 3):
                raise ValueError("kd, ks, ke must be (S, nT=%d, 3), got %s" % (scene.nT, tuple(t.shape)))
            if t.shape[0] != given[0].shape[0]:
                raise ValueError("kd, ks, ke must hold the same number of sets, got %s" %
                                 [tuple(u.shape) for u in given])
            continue
        if route.set_refused and t.dim() == 3:
            raise N.NativeError(route.set_refused)
        if tuple(t.shape) != (scene.nT, 3):
            raise ValueError("kd, ks, ke must be (nT=%d, 3), got %s" % (scene.nT, tuple(t.shape)))
    if route.unbounded_refused and (max_bounces is None or max_bounces < 0):
        raise N.NativeError(route.unbounded_refused)


class _MaterialsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kd, ks, ke, route, scene, views, params, stride, adjoint_seed):
        first = next(t for t in (kd, ks, ke) if t is not None)
        lead = ((first.shape[0],) if route.n_sets else ()) + ((len(views),) if route.views else ())
        c = [None if t is None else t.detach().contiguous().float() for t in (kd, ks, ke)]
        hdr = torch.empty(lead + (params.rows, params.width, 3), device=first.device, dtype=torch.float32)
        _launch(route, route.render, scene, views, params, lead[0] if route.n_sets else None, stride, c,
                (hdr.data_ptr(),) + ((None,) if route.ldr else ()), first.device)
        ctx.call, ctx.adjoint_seed, ctx.mat = (route, scene, views, params, lead, stride), adjoint_seed, c
        return hdr

    @staticmethod
    def backward(ctx, grad_hdr):
        route, scene, views, params, lead, stride = ctx.call
        p = _replay_params(params, ctx.adjoint_seed)
        sets = lead[:1] if route.n_sets else ()
        g = torch.zeros(sets + (3, scene.nT, 3), device=grad_hdr.device, dtype=torch.float64)
        base, frame = _adjoint_base(grad_hdr.float().contiguous(), p)  # frame: referenced until the call has returned
        _launch(route, route.adjoint, scene, views, p, sets[0] if sets else None, stride, ctx.mat,
                (base, g.data_ptr()), grad_hdr.device)
        out = [g.select(-3, i).float() if (t is not None and ctx.needs_input_grad[i]) else None
               for i, t in enumerate(ctx.mat)]
        return out[0], out[1], out[2], None, None, None, None, None, None

    @staticmethod
    def jvp(ctx, tkd, tks, tke, *_):
        """Forward-mode AD (torch.autograd.forward_ad): ONE tangent launch with
        K = 1 at the forward's own seed, cast once to float32.  Only
        ``render_materials`` has a tangent kernel."""
        route, scene, views, params, lead, stride = ctx.call
        if route.name != "render_materials":
            raise N.NativeError("forward-mode AD is not supported by %s; render_materials (one material set, the "
                                "scene's own camera, max_bounces in 0..62) is the supported op" % route.name)
        first = next(t for t in ctx.mat if t is not None)
        # an input without a tangent, or one that is not given, contributes nothing
        t = [None if (v is None or m is None) else v.detach().contiguous().float()
             for v, m in zip((tkd, tks, tke), ctx.mat)]
        if all(v is None for v in t):
            return torch.zeros((params.rows, params.width, 3), device=first.device, dtype=torch.float32)
        return _tangent_launch(scene, params, ctx.mat, t, 1, first.device)[0].float()


def _tangent_launch(scene, params: N.Params, mats, tangents, K: int, device) -> torch.Tensor:
    """ipt_tangent_mat_dev on torch's current stream: (K, rows, W, 3) float64."""
    out = torch.zeros((K, params.rows, params.width, 3), device=device, dtype=torch.float64)
    N.check(N.lib().ipt_tangent_mat_dev(scene.handle, C.byref(params), *[_ptr(t) for t in mats], K,
                                        *[_ptr(t) for t in tangents], out.data_ptr(), _stream(device)),
            "ipt_tangent_mat_dev")
    return out


def tangent_materials(scene: Scene, kd, ks, ke, tkd, tks, tke, width: int, height: int, spp: int, max_bounces=4,
                      seed: int = 0, row_begin: int = 0, row_end=None, row_step: int = 1) -> torch.Tensor:
    """Tangent images of ``render_materials``: K directions in material space
    -> a float64 CUDA tensor (K, rows, W, 3) from ONE launch
    (ipt_tangent_mat_dev; the paths are traced once, however many directions).
    kd, ks, ke: (nT, 3) CUDA tensors or None (the scene's own values); tkd,
    tks, tke: (K, nT, 3) CUDA tensors -- (nT, 3) means K = 1 -- or None (zero;
    at least one is given), 1 <= K <= 16.  Entry [k, p, c] is the derivative of
    pixel p's channel c of the HDR mean along direction k under the forward's
    own paths: <the material adjoint's gradient under the one-hot adjoint image
    at p, tangent k>, to fp64 summation order.  tks rows outside
    ``scene.lobe_mask`` and tke rows outside ``scene.emitter_mask`` are ignored.
    Runs on torch's current stream; no autograd graph.  Bounded estimator only
    (max_bounces 0..62)."""
    given = [t for t in (tkd, tks, tke) if t is not None]
    if not given:
        raise N.NativeError("material tangents: give at least one of the tangent arrays tkd, tks, tke")
    K = given[0].shape[0] if given[0].dim() == 3 else 1
    for t in given:
        if tuple(t.shape) not in ((K, scene.nT, 3),) + (((scene.nT, 3),) if K == 1 else ()):
            raise ValueError("tkd, tks, tke must be (K=%d, nT=%d, 3), got %s" % (K, scene.nT, tuple(t.shape)))
    for t in (kd, ks, ke):
        if t is not None and tuple(t.shape) != (scene.nT, 3):
            raise ValueError("kd, ks, ke must be (nT=%d, 3), got %s" % (scene.nT, tuple(t.shape)))
    for t in (kd, ks, ke, tkd, tks, tke):  # raw pointers go to the native call: all on one GPU
        if t is not None and (not t.is_cuda or t.device != given[0].device):
            raise ValueError("tangent_materials needs CUDA tensors on one device, got %s and %s" %
                             (t.device, given[0].device))
    if max_bounces is None or max_bounces < 0:
        raise N.NativeError("material tangents: give max_bounces in 0..62 (the unbounded estimator is not supported)")
    p = N.make_params(width, height, spp, max_bounces, seed, row_begin, row_end, row_step)
    c = [None if t is None else t.detach().contiguous().float() for t in (kd, ks, ke, tkd, tks, tke)]
    return _tangent_launch(scene, p, c[:3], c[3:], K, given[0].device)


def _materials(name, scene, views, kd, ks, ke, width, height, spp, max_bounces, seed, seed_stride, adjoint_seed,
               rows=(0, None, 1)):
    """The public material ops: validate, then _MaterialsFn on the op's route."""
    route = _ROUTES[name]
    _validate(route, scene, (kd, ks, ke), max_bounces)
    stride = width * height * spp if seed_stride is None else int(seed_stride)
    p = N.make_params(width, height, spp, max_bounces, seed, *rows)
    return _MaterialsFn.apply(kd, ks, ke, route, scene, views, p, stride, adjoint_seed)


def render_materials(scene: Scene, kd, ks, ke, width: int, height: int, spp: int, max_bounces=4, seed: int = 0,
                     row_begin: int = 0, row_end=None, adjoint_seed=None, row_step: int = 1) -> torch.Tensor:
    """Differentiable render w.r.t. diffuse kd, specular ks and emission ke
    ((nT, 3) CUDA tensors; any may be None = the scene's own values, or not
    require grad).  The forward is ``render``'s with the overrides; the
    backward is ONE launch of the material adjoint.  Structure is frozen at
    load: ke rows outside ``scene.emitter_mask`` and ks rows outside
    ``scene.lobe_mask`` are ignored, and their gradients are exactly 0; the
    Phong exponent is not differentiated.  Refused (NativeError): the
    unbounded estimator (max_bounces None), which
    ``render_materials_unbounded`` takes, and batched inputs (S, nT, 3),
    which ``render_materials_batch`` takes.
    `adjoint_seed` as in ``render``."""
    return _materials("render_materials", scene, None, kd, ks, ke, width, height, spp, max_bounces, seed, None,
                      adjoint_seed, (row_begin, row_end, row_step))


def render_materials_unbounded(scene: Scene, kd, ks, ke, width: int, height: int, spp: int, seed: int = 0,
                               row_begin: int = 0, row_end=None, adjoint_seed=None, row_step: int = 1) -> torch.Tensor:
    """``render_materials`` for the reference's own estimator (no bounce cap;
    paths end by Russian roulette or a miss): the forward is
    ipt_render_mat_dev with max_bounces = -1, the backward ONE launch of the
    unbounded material adjoint (ipt_adjoint_mat_unbounded_dev: the ring and
    replay sweep of ``render(max_bounces=None)``'s adjoint, emitting dL/dKd,
    dL/dKs and dL/dKe).  kd, ks, ke, the masks, None and
    no-grad inputs and `adjoint_seed` as in ``render_materials``; batched
    (S, nT, 3) inputs are refused (NativeError)."""
    return _materials("render_materials_unbounded", scene, None, kd, ks, ke, width, height, spp, None, seed, None,
                      adjoint_seed, (row_begin, row_end, row_step))


def render_materials_batch(scene: Scene, kd, ks, ke, width: int, height: int, spp: int, max_bounces=4,
                           seed: int = 0, seed_stride=None, adjoint_seed=None) -> torch.Tensor:
    """``render_materials`` for S material sets over one geometry: kd, ks, ke
    are (S, nT, 3) CUDA tensors (any may be None = the scene's own values in
    every set, or not require grad; at least one is given and all share S)
    -> HDR images (S, H, W, 3).  ONE batched forward launch
    (ipt_render_mat_batch_dev); the backward is ONE batched launch of the
    material adjoint.  Set b is ``render_materials`` of its rows with seed
    ``seed + b * seed_stride`` bit for bit (default stride: one frame of
    samples, as ``render_batch``).  Masks, refusals and `adjoint_seed` as in
    ``render_materials``."""
    return _materials("render_materials_batch", scene, None, kd, ks, ke, width, height, spp, max_bounces, seed,
                      seed_stride, adjoint_seed)


class _BatchRenderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kd, scene, params, stride, adjoint_seed):
        kd_c = kd.detach().contiguous().float()
        S = kd_c.shape[0]
        hdr = torch.empty((S, params.height, params.width, 3), device=kd.device, dtype=torch.float32)
        N.check(N.lib().ipt_render_batch_dev(scene.handle, C.byref(params), S, stride, kd_c.data_ptr(),
                                             hdr.data_ptr(), _stream(hdr.device)), "ipt_render_batch_dev")
        ctx.scene, ctx.params, ctx.stride, ctx.adjoint_seed = scene, params, stride, adjoint_seed
        ctx.save_for_backward(kd_c)
        return hdr

    @staticmethod
    def backward(ctx, grad_hdr):
        (kd_c,) = ctx.saved_tensors
        g = torch.zeros(kd_c.shape, device=kd_c.device, dtype=torch.float64)
        adj = grad_hdr.float().contiguous()
        p = _replay_params(ctx.params, ctx.adjoint_seed)
        N.check(N.lib().ipt_adjoint_batch_dev(ctx.scene.handle, C.byref(p), kd_c.shape[0], ctx.stride,
                                              kd_c.data_ptr(), adj.data_ptr(), g.data_ptr(), _stream(g.device)),
                "ipt_adjoint_batch_dev")
        return g.to(kd_c.dtype), None, None, None, None


def render_batch(scene: Scene, kd: torch.Tensor, width: int, height: int, spp: int, max_bounces=4, seed: int = 0,
                 seed_stride=None, adjoint_seed=None) -> torch.Tensor:
    """Differentiable render of S material sets over one geometry in one
    launch (ipt_render_batch_dev): kd (S, nT, 3) -> HDR images (S, H, W, 3).
    Set b is ``render(scene, kd[b], ..., seed + b * seed_stride)`` bit for bit
    (default stride: one frame of samples, so the sets' sample streams are
    disjoint); the backward runs ONE batched adjoint launch."""
    if kd.dim() != 3 or kd.shape[1] != scene.nT or kd.shape[2] != 3:
        raise ValueError("kd must be (S, nT=%d, 3), got %s" % (scene.nT, tuple(kd.shape)))
    stride = width * height * spp if seed_stride is None else int(seed_stride)
    p = N.make_params(width, height, spp, max_bounces, seed)
    return _BatchRenderFn.apply(kd, scene, p, stride, adjoint_seed)


def render_views(scene: Scene, views, kd, ks, ke, width: int, height: int, spp: int, max_bounces=4, seed: int = 0,
                 seed_stride=None, adjoint_seed=None) -> torch.Tensor:
    """``render_materials`` through V caller-supplied cameras (``scene.views``)
    with ONE material set: kd, ks, ke are (nT, 3) CUDA tensors (any may be
    None = the scene's own, or not require grad; at least one is given) ->
    HDR images (V, H, W, 3).  ONE forward launch (ipt_render_views_dev): view
    b is ``render_materials`` through camera b at ``seed + b * seed_stride``
    bit for bit (default stride: one frame of samples, W*H*spp).  The backward
    is ONE launch of the views' material adjoint, the gradient summed over the
    views, returned as float32 for the inputs that require it.  Bounded
    estimator only (max_bounces 0..62).  `adjoint_seed` as in ``render``."""
    return _materials("render_views", scene, views, kd, ks, ke, width, height, spp, max_bounces, seed, seed_stride,
                      adjoint_seed)


def render_views_batch(scene: Scene, views, kd, ks, ke, width: int, height: int, spp: int, max_bounces=4,
                       seed: int = 0, seed_stride=None, adjoint_seed=None) -> torch.Tensor:
    """``render_views`` for S material sets over one geometry: kd, ks, ke are
    (S, nT, 3) CUDA tensors (any may be None = the scene's own values in every
    set, or not require grad; at least one is given and all share S) -> HDR
    images (S, V, H, W, 3).  ONE forward launch (ipt_render_views_batch_dev):
    image (s, b) is view b of ``render_views`` with set s's rows at ``seed +
    (s * V + b) * seed_stride`` bit for bit (default stride: one frame of
    samples).  The backward is ONE launch of the material adjoint over the
    S * V pairs, each set's gradient summed over its views, returned as
    float32 for the inputs that require it.  Bounded estimator only
    (max_bounces 0..62).  `adjoint_seed` as in ``render_views``."""
    return _materials("render_views_batch", scene, views, kd, ks, ke, width, height, spp, max_bounces, seed,
                      seed_stride, adjoint_seed)


def render_views_batch_unbounded(scene: Scene, views, kd, ks, ke, width: int, height: int, spp: int, seed: int = 0,
                                 seed_stride=None, adjoint_seed=None) -> torch.Tensor:
    """``render_views_batch`` for the reference's own estimator (no bounce cap,
    paths end by Russian roulette or a miss): kd, ks, ke (S, nT, 3) CUDA
    tensors as there -> HDR images (S, V, H, W, 3).  ONE forward launch
    (ipt_render_views_batch_unbounded_dev) and ONE backward launch of the
    unbounded material adjoint over the S * V pairs
    (ipt_adjoint_views_batch_unbounded_dev), float32 gradients
    for the inputs that require them, None for the others.  Seeds, masks and
    `adjoint_seed` as in ``render_views_batch``."""
    return _materials("render_views_batch_unbounded", scene, views, kd, ks, ke, width, height, spp, None, seed,
                      seed_stride, adjoint_seed)
