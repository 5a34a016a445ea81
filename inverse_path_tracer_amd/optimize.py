"""Material recovery by gradient descent (BASELINE.json configs[4], "C5").

The reference recovers per-triangle albedo by regressing a GCN on transport
graphs (ipt.py:86-140).  With the adjoint integrator the same unknowns are
optimised directly: per scene, Kd (nT, 3) starts at a constant and Adam
minimises the L2 distance between the rendered HDR image and a target render
(the reference's imgs/*.png are not shipped; targets are forward renders at
the ground-truth Kd with many more samples).

* Scene batches: scenes/0..99.txt share their geometry and differ only in the
  cube's Kd (ipt_cuda.py:115-134 writes them that way), so the scenes of a rank
  form ONE batch over one loaded geometry: each step is one batched forward
  launch and one batched adjoint launch (torch_ops.render_batch) for all of
  them, instead of two launches and an autograd graph per scene.  Scenes whose
  geometry differs fall back to per-scene renders.
* Unbiased gradients: the adjoint of step t traces an independent sample
  stream (``adjoint_seed``), so the residual I - T of the forward is not
  correlated with the derivative (same-stream replay biases Adam towards
  darker albedo by O(1/spp)).
* Scene-parallel: rank r owns a contiguous block of the scenes
  (``shard_scenes``); per-scene parameters need no collective.  Every sample
  stream is keyed on the GLOBAL scene index and the global scene count (the
  target render of scene i, the forward / adjoint frames of step t), so a
  split over ranks traces exactly the samples of the one-rank run: images
  bitwise, gradients to fp64 summation order (tests/test_gpu_multirank.py).  ``tie_shared=k`` additionally treats the first k triangles
  (18 = the Cornell box, identical in every scene) as ONE parameter set shared
  by all scenes -- their gradient is summed across scenes and ranks with a
  single RCCL all-reduce per step.

* Specular and emission: ``MaterialOptimizer(learn=("ks", "ke"))`` (any subset
  of kd, ks, ke) optimises those blocks through the batched material adjoint
  (torch_ops.render_materials_batch): still one forward and one
  adjoint launch per batch and step, over scenes that share geometry, emitter
  list, lobe flags and exponents and differ only in the values of Kd, Ks, Ke.
  The default, ``learn=("kd",)``, is the Kd-only path above, unchanged.
* Views: ``build_tasks(views=cams)`` / ``MaterialOptimizer(views=cams)`` with
  cams (V, 4, 4) observe every scene through V caller-supplied cameras
  (DESIGN.md §20): targets are (V, H, W, 3), a step is still one forward and
  one adjoint launch per batch (torch_ops.render_views_batch, S sets x V
  views), for every ``learn``.  Without ``views`` nothing changes.
* No bounce cap: with ``max_bounces=None`` (or negative; the reference's own
  estimator) the two materials paths above render targets and steps through
  torch_ops.render_views_batch_unbounded -- without ``views``
  through one view of the scene's own camera, at the ``views=None`` seeds.
  The Kd-only path takes ``max_bounces=None`` as it always did.

    python -m inverse_path_tracer_amd.optimize --scenes assets/scenes --n 13 --steps 200
"""
from __future__ import annotations

import argparse
import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import torch_ops
from .distributed import allreduce_, world
from .scene import Scene, Views

# ipt_scene_export_triangles columns holding the diffuse Kd (everything else
# is geometry / other material fields that must agree for a batch)
_KD_COLS = slice(25, 28)
# ... and Kd, Ks, Ke together (28:31 Ks, 31:34 Ke): the values a material batch may differ in
_MAT_COLS = slice(25, 34)
_BLOCKS = ("kd", "ks", "ke")


@dataclass
class SceneTask:
    path: str
    scene: Scene                  # geometry handle (shared by the tasks of one batch)
    truth: torch.Tensor           # ground-truth Kd (nT, 3)
    target: torch.Tensor          # target HDR image (H, W, 3)
    kd: torch.Tensor              # parameters (nT, 3)
    history: List[float] = field(default_factory=list)
    index: int = 0                # global scene index (keys the task's sample streams)
    # specular and emitted colour (nT, 3) and their ground truths: only for MaterialOptimizer(learn=...)
    # with "ks" / "ke"; None = the geometry handle's own values
    ks: Optional[torch.Tensor] = None
    ke: Optional[torch.Tensor] = None
    truth_ks: Optional[torch.Tensor] = None
    truth_ke: Optional[torch.Tensor] = None
    views: Optional[Views] = None  # build_tasks(views=...): the cameras over `scene`; target is then (V, H, W, 3)


def _scene_files(root: str, n: int) -> List[str]:
    return [os.path.join(root, "%d.txt" % i) for i in range(n)]


def shard_scenes(n: int, world: int, rank: int):
    """Contiguous block [begin, end) of the n scenes owned by `rank` (balanced:
    sizes differ by at most one).  Contiguous, so a rank's scenes of one
    geometry are ONE batch whose sample streams continue the global ones."""
    base, rem = divmod(n, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


def _runs(idx: List[int], tasks: List[SceneTask], limit: int):
    """Split task positions into runs of consecutive global indices (<= limit each)."""
    runs, cur = [], []
    for i in idx:
        if cur and (tasks[i].index != tasks[cur[-1]].index + 1 or len(cur) >= limit):
            runs.append(cur)
            cur = []
        cur.append(i)
    if cur:
        runs.append(cur)
    return runs


def _geometry_key(sc: Scene, materials: bool = False) -> bytes:
    """What the scenes of one batch must share.  Kd-only batches: everything
    but Kd.  Material batches: everything but the VALUES of Kd, Ks, Ke -- the
    emitter list (column 56), the exponent (34) and the lobe flags are
    structure, fixed when the geometry handle is loaded."""
    t = sc.triangles()
    cols = _MAT_COLS if materials else _KD_COLS
    parts = [t[:, :cols.start], t[:, cols.stop:]]
    if materials:
        parts.append(sc.lobe_mask[:, None].astype(np.float32))
    return np.concatenate(parts, axis=1).tobytes()


def _unbounded(max_bounces) -> bool:
    """The reference's own estimator: no bounce cap (None or negative)."""
    return max_bounces is None or max_bounces < 0


def _view_cams(views) -> np.ndarray:
    cams = np.ascontiguousarray(np.asarray(views, np.float32))
    if cams.ndim != 3 or cams.shape[0] < 1 or cams.shape[1:] != (4, 4):
        raise ValueError("views must be (V, 4, 4) camera matrices, got %s" % (cams.shape,))
    return cams


def _route(learn, cams, max_bounces):
    """(render, own_view): how targets and steps are rendered, for build_tasks
    and MaterialOptimizer alike.  render(scene, views, kd, ks, ke, W, H, spp,
    seed=, seed_stride=[, adjoint_seed=]) -> (S, [V,] H, W, 3) is one batched
    torch_ops op; own_view: the caller passes a Views of the scene's own
    camera as the single view (V = 1), and render drops the view axis.
      1. learn ("kd",), no views, any max_bounces: render_batch;
      2. no bounce cap: render_views_batch_unbounded, through
         the own camera without views;
      3. views: render_views_batch;  4. otherwise: render_materials_batch."""
    mb = max_bounces
    if learn == ("kd",) and cams is None:
        return lambda sc, vh, kd, ks, ke, *frame, **seeds: torch_ops.render_batch(sc, kd, *frame, mb, **seeds), False
    if _unbounded(mb):
        own_view = cams is None

        def render(sc, vh, *args, **seeds):
            img = torch_ops.render_views_batch_unbounded(sc, vh, *args, **seeds)
            return img[:, 0] if own_view else img
        return render, own_view
    if cams is not None:
        return lambda sc, vh, *args, **seeds: torch_ops.render_views_batch(sc, vh, *args, mb, **seeds), False
    return lambda sc, vh, *args, **seeds: torch_ops.render_materials_batch(sc, *args, mb, **seeds), False


def _target_seed(seed, index, V, frame):
    """Scene `index` view b is target frame index * V + b of the stream at seed + 10^9 (V = 1 without views)."""
    return seed + 10**9 + index * V * frame


def _step_seeds(seed, step, T, n_before, V, frame, decorrelate):
    """(seed, adjoint_seed) of a batch whose first scene is n_before: step t of T scenes takes the frames
    [2 t T V, 2 (t + 1) T V), the T V forward frames first (V = 1 without views)."""
    base = seed + (2 * step * T + n_before) * V * frame
    return base, (base + T * V * frame) if decorrelate else None


def build_tasks(files: List[str], width: int, height: int, target_spp: int, max_bounces: int, init: float,
                device: torch.device, seed: int = 7, target_chunk: int = 16, first_index: int = 0,
                learn: Sequence[str] = ("kd",), init_ks: float = 0.5, init_ke: float = 5.0,
                views=None) -> List[SceneTask]:
    """Load the scenes (one device geometry per distinct geometry), render the
    targets in batches of `target_chunk`, and create the parameters.  files[i]
    is global scene first_index + i: its target render traces the samples of
    seed + 10^9 + (first_index + i) * W*H*target_spp, whichever rank loads it.

    learn with "ks" / "ke" (MaterialOptimizer's): scenes that differ only in
    the values of Kd, Ks, Ke share one geometry handle; the tasks carry ks, ke
    and their truths, the learned blocks start at init / init_ks / init_ke on
    the rows they act on (lobe rows, emitter rows) and the others at the truth;
    the targets are rendered with the true values of all three.

    views, (V, 4, 4) camera matrices: one Views handle per geometry handle
    (the tasks' ``views``), targets (V, H, W, 3) rendered with the truth through
    torch_ops.render_views_batch -- scene i view b traces seed + 10^9 +
    (i * V + b) * W*H*target_spp."""
    cams = None if views is None else _view_cams(views)
    if set(learn) - set(_BLOCKS) or not tuple(learn):
        raise ValueError("learn must name some of %s, got %r" % (_BLOCKS, tuple(learn)))
    learn = tuple(b for b in _BLOCKS if b in tuple(learn))
    mats = learn != ("kd",)
    groups = {}  # geometry key -> device Scene
    handles = {}  # ... -> its Views (views given)
    tasks = []
    for k, f in enumerate(files):
        host = Scene.from_file(f, device=False)
        key = _geometry_key(host, mats)
        if key not in groups:
            groups[key] = Scene.from_file(f)
            if cams is not None:
                handles[key] = groups[key].views(cams)
        truth = torch.tensor(host.materials, device=device)
        kd0 = torch.full_like(truth, init) if "kd" in learn else truth.clone()
        task = SceneTask(f, groups[key], truth, None, kd0.requires_grad_("kd" in learn), index=first_index + k,
                         views=handles.get(key))
        if mats:
            _, ks, ke, _ = host.material_params()
            lobe = torch.tensor(host.lobe_mask, device=device)[:, None].float().expand(-1, 3)
            emit = torch.tensor(host.emitter_mask, device=device)[:, None].float().expand(-1, 3)
            task.truth_ks, task.truth_ke = torch.tensor(ks, device=device), torch.tensor(ke, device=device)
            task.ks = (lobe * init_ks).requires_grad_(True) if "ks" in learn else task.truth_ks.clone()
            task.ke = (emit * init_ke).requires_grad_(True) if "ke" in learn else task.truth_ke.clone()
        host.close()
        tasks.append(task)
    frame = width * height * target_spp
    render, own_view = _route(learn, cams, max_bounces)
    with torch.no_grad():
        for sc in groups.values():
            mine = [i for i, t in enumerate(tasks) if t.scene is sc]
            own = sc.views(sc.camera()) if own_view else None
            for idx in _runs(mine, tasks, target_chunk):
                vh = own if own_view else tasks[idx[0]].views
                kd, ks, ke = (torch.stack([getattr(tasks[i], b) for i in idx]) if mats or b == "truth" else None
                              for b in ("truth", "truth_ks", "truth_ke"))
                img = render(sc, vh, kd, ks, ke, width, height, target_spp, seed_stride=frame,
                             seed=_target_seed(seed, tasks[idx[0]].index, 1 if vh is None else len(vh), frame))
                for j, i in enumerate(idx):
                    tasks[i].target = img[j].clone()
            if own is not None:
                own.close()
    return tasks


class MaterialOptimizer:
    """Persistent Adam state over every task's kd (nT, 3).  Each group of
    tasks sharing a geometry is one batch: a (S, nT, 3) parameter whose rows
    the tasks' kd become views of, rendered by one batched forward and one
    batched adjoint launch per step.  tie_shared = number of leading
    triangles whose Kd is shared by all scenes (18 = the Cornell box), or
    None.  Losses reach the tasks' histories with one device->host copy every
    `flush_every` steps (on every rank) and at the end of each run().

    Sample streams: step t of the whole job (n_total scenes over all ranks,
    default max(task index) + 1) traces frames [2 t n_total, 2 (t + 1) n_total) of the
    sample-index space, scene i's forward in frame 2 t n_total + i and its
    adjoint n_total frames later -- so each rank of a scene-parallel split
    traces exactly the one-rank run's samples for its scenes.  A batch is
    one geometry's tasks with consecutive global indices (seed_stride = one
    frame between its sets).

    learn: the blocks to optimise, a subset of ("kd", "ks", "ke"); the default
    ("kd",) is the Kd-only optimiser above.  With "ks" and/or "ke" a batch
    holds one (S, nT, 3) leaf per learned block (the tasks' kd / ks / ke become
    views of their rows; the other blocks stay at the tasks' values, None = the
    geometry handle's own) and renders through
    torch_ops.render_materials_batch: one batched forward and one batched
    material-adjoint launch per step, on the same sample streams.  Rows the
    blocks do not act on are masked (scene.lobe_mask for Ks, scene.emitter_mask
    for Ke: structure is frozen at load); Kd and Ks are clamped to [0, 1], Ke to
    [0, inf).  `lr` may then be a dict per block, e.g. {"ks": 0.02, "ke":
    0.2} (emission lives on another scale).  tie_shared is a Kd-only feature.

    views, (V, 4, 4) camera matrices (the tasks come from
    ``build_tasks(views=...)``: targets (V, H, W, 3)): every batch renders
    through torch_ops.render_views_batch, for every `learn`, ("kd",) included
    -- one forward and one adjoint launch over the batch's S x V (scene, view)
    pairs; a scene's loss is the mean over (V, H, W, 3).  Step t of the job
    then takes frames [2 t T V, 2 (t + 1) T V) with T = n_total: scene i view
    b's forward is frame 2 t T V + i V + b, its adjoint T V frames later, so a
    rank of a scene-parallel split still traces the one-rank run's samples.
    tie_shared together with views raises ValueError."""

    def __init__(self, tasks: List[SceneTask], width: int, height: int, spp: int, max_bounces: int,
                 lr: Union[float, Dict[str, float]] = 1e-2, tie_shared: Optional[int] = None, seed: int = 0,
                 flush_every: int = 16, decorrelate: bool = True, n_total: Optional[int] = None,
                 learn: Sequence[str] = ("kd",), views=None):
        self.tasks, self.W, self.H, self.spp, self.mb = tasks, width, height, spp, max_bounces
        self.cams = None if views is None else _view_cams(views)
        if self.cams is not None and tie_shared:
            raise ValueError("MaterialOptimizer: tie_shared is not supported together with views")
        if not tuple(learn) or set(learn) - set(_BLOCKS):
            raise ValueError("learn must name some of %s, got %r" % (_BLOCKS, tuple(learn)))
        self.learn = tuple(b for b in _BLOCKS if b in tuple(learn))
        self.tie, self.seed, self.flush_every, self.decorrelate = tie_shared, seed, flush_every, decorrelate
        # the job's scene count: the caller's, else max(index) + 1 (a rank
        # given only the tasks of global scenes b .. b+k-1 must pass the job's n)
        idx = [t.index for t in tasks]
        if len(set(idx)) != len(idx):
            raise ValueError("MaterialOptimizer: task indices must be unique (build_tasks(first_index=...))")
        self.n_total = (max(idx) + 1 if idx else 0) if n_total is None else int(n_total)
        if idx and max(idx) >= self.n_total:
            raise ValueError("MaterialOptimizer: task index %d >= n_total %d" % (max(idx), self.n_total))
        self.frame = width * height * spp
        self.batches = []  # (scene, tasks)
        for t in tasks:
            b = self.batches[-1] if self.batches else None
            if b is not None and b[0] is t.scene and t.index == b[1][-1].index + 1:
                b[1].append(t)
            else:
                self.batches.append((t.scene, [t]))
        self.leaves, self.targets, self.offsets = [], [], []
        self.shared = None
        self.step_count = 0
        self.pending = []  # (tasks, per-scene loss tensor) in step order
        self.view_handles = []  # per batch (views given)
        if self.cams is not None:
            made = {}  # geometry handle -> Views: the tasks' own when they hold these cameras
            for sc, ts in self.batches:
                if id(sc) not in made:
                    own = ts[0].views
                    reuse = own is not None and np.array_equal(own.cams, self.cams)
                    made[id(sc)] = own if reuse else sc.views(self.cams)
                self.view_handles.append(made[id(sc)])
                want = (len(self.cams), height, width, 3)
                for t in ts:
                    if tuple(t.target.shape) != want:
                        raise ValueError("MaterialOptimizer: views need targets of shape %s (build_tasks(views=...)), "
                                         "got %s" % (want, tuple(t.target.shape)))
        # no bounce cap on the materials path: every batch renders through
        # torch_ops.render_views_batch_unbounded; without views the scene's own
        # camera is the one view (V = 1: the frames are the views=None ones)
        self.render, own_view = _route(self.learn, self.cams, max_bounces)
        if own_view:
            made = {}
            for sc, ts in self.batches:
                if id(sc) not in made:
                    made[id(sc)] = sc.views(sc.camera())
                self.view_handles.append(made[id(sc)])
        if self.learn != ("kd",) or self.cams is not None:
            self._init_materials(lr, tie_shared)
            return
        if isinstance(lr, dict):
            lr = lr["kd"]
        for sc, ts in self.batches:
            leaf = torch.stack([t.kd.detach() for t in ts]).clone().requires_grad_(True)
            tgt = torch.stack([t.target for t in ts])
            for j, t in enumerate(ts):
                t.kd, t.target = leaf[j], tgt[j]
            self.offsets.append(ts[0].index)  # global index of the batch's first scene
            self.leaves.append(leaf)
            self.targets.append(tgt)
        if tie_shared:
            self.shared = tasks[0].kd.detach()[:tie_shared].clone().requires_grad_(True) if tasks else \
                torch.full((tie_shared, 3), 0.5, device="cuda", requires_grad=True)
        self.params = self.leaves + ([self.shared] if self.shared is not None else [])
        self.opt = torch.optim.Adam(self.params, lr=lr)

    def _init_materials(self, lr, tie_shared):
        """learn with "ks" / "ke": per batch, one leaf per learned block and the fixed (S, nT, 3) values (or
        None) of the others; self.leaves[i] is the dict block -> leaf of batch i."""
        if tie_shared:
            raise ValueError("MaterialOptimizer: tie_shared is supported for learn=('kd',) only")
        self.fixed, self.masks = [], []
        for sc, ts in self.batches:
            leaf, fixed = {}, {}
            for b in _BLOCKS:
                vals = [getattr(t, b) for t in ts]
                if b in self.learn:
                    if any(v is None for v in vals):
                        raise ValueError("MaterialOptimizer: learn has %r but a task carries no %s "
                                         "(build_tasks(learn=...))" % (b, b))
                    leaf[b] = torch.stack([v.detach() for v in vals]).clone().requires_grad_(True)
                    for j, t in enumerate(ts):
                        setattr(t, b, leaf[b][j])
                else:
                    fixed[b] = None if any(v is None for v in vals) else torch.stack([v.detach() for v in vals])
            tgt = torch.stack([t.target for t in ts])
            for j, t in enumerate(ts):
                t.target = tgt[j]
            dev = tgt.device
            self.masks.append({"ks": torch.tensor(sc.lobe_mask, device=dev)[None, :, None].float(),
                               "ke": torch.tensor(sc.emitter_mask, device=dev)[None, :, None].float()})
            self.offsets.append(ts[0].index)
            self.leaves.append(leaf)
            self.fixed.append(fixed)
            self.targets.append(tgt)
        rate = lr if isinstance(lr, dict) else {b: lr for b in self.learn}
        groups = [{"params": [leaf[b] for leaf in self.leaves], "lr": rate[b]} for b in self.learn]
        self.params = [q for g in groups for q in g["params"]]
        self.opt = torch.optim.Adam([g for g in groups if g["params"]] or [{"params": []}])

    def _forward_backward(self, k, kd, ks, ke):
        """Batch k's forward on the frames of this step, the loss per scene (the mean over its [V,] H, W, 3)
        and its backward on the step's adjoint frames: each scene's loss only reaches its own parameters."""
        sc, ts = self.batches[k]
        vh = self.view_handles[k] if self.view_handles else None
        # step t uses 2 T V frames of the sample-index space: the T V forward frames, then the T V adjoint frames
        seed, adjoint_seed = _step_seeds(self.seed, self.step_count, self.n_total, self.offsets[k],
                                         1 if vh is None else len(vh), self.frame, self.decorrelate)
        img = self.render(sc, vh, kd, ks, ke, self.W, self.H, self.spp, seed=seed, seed_stride=self.frame,
                          adjoint_seed=adjoint_seed)
        per_scene = ((img - self.targets[k]) ** 2).mean(dim=tuple(range(1, img.dim())))
        per_scene.sum().backward()
        self.pending.append((ts, per_scene.detach()))

    def _end_step(self):
        self.step_count += 1
        if self.flush_every and self.step_count % self.flush_every == 0:
            _flush_losses(self.pending)

    def _step_materials(self):
        self.opt.zero_grad(set_to_none=False)
        for k, (leaf, fixed, mask) in enumerate(zip(self.leaves, self.fixed, self.masks)):
            v = {b: leaf[b] if b in leaf else fixed[b] for b in _BLOCKS}
            for b in ("ks", "ke"):  # frozen rows: no value, no gradient
                if b in leaf:
                    v[b] = leaf[b] * mask[b]
            self._forward_backward(k, v["kd"], v["ks"], v["ke"])
        self.opt.step()
        with torch.no_grad():
            for leaf in self.leaves:
                for b, q in leaf.items():
                    q.clamp_(0.0, None if b == "ke" else 1.0)  # emission has no upper bound
        self._end_step()

    def step(self):
        """One Adam step over every scene (no host synchronisation)."""
        if self.learn != ("kd",) or self.cams is not None:
            return self._step_materials()
        self.opt.zero_grad(set_to_none=False)
        for k, ((_, ts), leaf) in enumerate(zip(self.batches, self.leaves)):
            kd = leaf
            if self.shared is not None:
                kd = torch.cat([self.shared.unsqueeze(0).expand(len(ts), -1, -1), leaf[:, self.tie:]], dim=1)
            self._forward_backward(k, kd, None, None)
        if self.shared is not None:
            if self.shared.grad is None:
                self.shared.grad = torch.zeros_like(self.shared)
            allreduce_(self.shared.grad)  # the only exchange: one nT_shared*3 all-reduce
        self.opt.step()
        with torch.no_grad():
            for p in self.params:
                p.clamp_(0.0, 1.0)
        self._end_step()

    def run(self, steps: int, log_every: int = 0):
        _, R = world()
        for i in range(steps):
            self.step()
            if log_every and i % log_every == 0:
                _flush_losses(self.pending)
                if R == 0:
                    print("step %d loss %.6g" % (self.step_count - 1, sum(t.history[-1] for t in self.tasks) /
                                                 max(1, len(self.tasks))), flush=True)
        _flush_losses(self.pending)
        return self


def optimize(tasks: List[SceneTask], width: int, height: int, spp: int, max_bounces: int, steps: int,
             lr: float = 1e-2, tie_shared: Optional[int] = None, seed: int = 0, log_every: int = 0,
             flush_every: int = 16, decorrelate: bool = True, n_total: Optional[int] = None):
    """`steps` Adam steps of a fresh MaterialOptimizer; returns the shared
    (tied) parameter or None."""
    m = MaterialOptimizer(tasks, width, height, spp, max_bounces, lr, tie_shared, seed, flush_every, decorrelate,
                          n_total)
    m.run(steps, log_every)
    return m.shared


def gauss_newton_materials(scene: Scene, target_hdr, groups, width: int, height: int, spp: int, max_bounces: int,
                           seed: int, steps: int, damping: float = 0.0, tangent_seed: Optional[int] = None):
    """Gauss-Newton on a few tied material parameters, with the Jacobian from
    the tangent launch.

    `groups` is a list of (block, rows), block in ("kd", "ks", "ke"): the rows
    of a group share ONE value per channel (started from the scene's value in
    the group's first row), K = len(groups) <= 16.  A step is one
    ipt_render_mat_dev launch and one ipt_tangent_mat_dev launch with one
    indicator tangent per group; then per channel c, with A the K x pixels
    matrix of the tangents' channel c and r = target - I, delta solves
    (A A^T + damping I) delta = A r (least squares when singular), and is added
    to the groups' rows.  The scene's own values are not changed.

    `tangent_seed` None differentiates the forward's own paths (the exact
    Jacobian of the returned image).  When the target is a noisy render on an
    independent sample stream, DESIGN.md §5.4 applies: with the forward's own
    samples E[(I - T) dI] = (E[I] - T) E[dI] + Cov(I, dI), and the covariance
    term biases the right side A r (towards darker albedo; at the truth it
    measured 7x the remaining noise at 4 spp).  Give `tangent_seed` an
    independent stream to remove it -- one whose seeds differ from the
    forward's in the LOW 32 bits, e.g. seed + W*H*spp: curand_init hashes a
    seed's halves separately, and seeds equal modulo 2^32 stay correlated (a
    bias of 14% of the same-stream one).  With a target rendered at the truth on the SAME seed
    the residual is exactly 0 there and the forward's own paths are right.

    Returns the groups' values after each step, (steps, K, 3) float64."""
    K = len(groups)
    if not 1 <= K <= 16:
        raise ValueError("gauss_newton_materials takes 1..16 groups, got %d" % K)
    names = ("kd", "ks", "ke")
    host = scene.material_params()[:3]
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in host]
    tang = [None, None, None]
    idx, val = [], np.zeros((K, 3), np.float64)
    for k, (block, rows) in enumerate(groups):
        if block not in names:
            raise ValueError("group block must be one of %s, got %r" % (names, block))
        b = names.index(block)
        r = torch.as_tensor(np.asarray(list(rows), np.int64), device="cuda")
        if r.numel() == 0 or int(r.min()) < 0 or int(r.max()) >= scene.nT:
            raise ValueError("group %d: rows must be in 0..%d" % (k, scene.nT - 1))
        if tang[b] is None:
            tang[b] = torch.zeros((K, scene.nT, 3), device="cuda", dtype=torch.float32)
        tang[b][k, r] = 1.0
        idx.append((b, r))
        val[k] = host[b][int(r[0])]
    target = torch.as_tensor(np.asarray(target_hdr, np.float32) if not torch.is_tensor(target_hdr) else target_hdr,
                             device="cuda").reshape(height, width, 3).double()
    history = np.zeros((steps, K, 3), np.float64)
    for s in range(steps):
        for k, (b, r) in enumerate(idx):
            dev[b][r] = torch.as_tensor(val[k], dtype=torch.float32, device="cuda")
        with torch.no_grad():
            img = torch_ops.render_materials(scene, dev[0], dev[1], dev[2], width, height, spp, max_bounces, seed)
        tan = torch_ops.tangent_materials(scene, dev[0], dev[1], dev[2], tang[0], tang[1], tang[2], width, height, spp,
                                          max_bounces, seed if tangent_seed is None else int(tangent_seed))
        res = (target - img.double()).reshape(-1, 3)
        A = tan.reshape(K, -1, 3)
        for c in range(3):
            Ac = A[:, :, c]
            n = (Ac @ Ac.T).cpu().numpy() + damping * np.eye(K)
            rhs = (Ac @ res[:, c]).cpu().numpy()
            val[:, c] += np.linalg.lstsq(n, rhs, rcond=None)[0]
        history[s] = val
    return history


def _flush_losses(pending):
    """Move the pending per-scene losses to the tasks' histories (one copy)."""
    if pending:
        vals = torch.cat([l for _, l in pending]).float().cpu().tolist()
        k = 0
        for ts, _ in pending:
            for t in ts:
                t.history.append(vals[k])
                k += 1
        pending.clear()


def observable_mask(tasks: List[SceneTask], width: int, height: int, spp: int, max_bounces: int, seed: int = 5,
                    frac: float = 0.25, first: int = 18):
    """Per task, the triangles >= `first` whose Kd the image constrains: |dL/dKd|
    at the start above `frac` of the largest (the cube's back and bottom faces
    never reach the camera and cannot be recovered)."""
    masks = []
    for t in tasks:
        kd = t.kd.detach().clone().requires_grad_(True)
        img = torch_ops.render(t.scene, kd, width, height, spp, max_bounces, seed=seed)
        ((img - t.target) ** 2).mean().backward()
        g = kd.grad.abs().sum(1)[first:]
        masks.append(g > frac * float(g.max()))
    return masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=os.path.join(os.path.dirname(os.path.dirname(__file__)), "assets", "scenes"))
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--target-spp", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--tie", action="store_true")
    args = ap.parse_args()
    import torch.distributed as dist

    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if ws > 1:
        dist.init_process_group("nccl", device_id=dev)
    b, e = shard_scenes(args.n, ws, rank)
    files = _scene_files(args.scenes, args.n)[b:e]
    t0 = time.time()
    tasks = build_tasks(files, args.width, args.height, args.target_spp, args.bounces, 0.5, dev, first_index=b)
    torch.cuda.synchronize()
    t1 = time.time()
    m = MaterialOptimizer(tasks, args.width, args.height, args.spp, args.bounces, args.lr,
                          tie_shared=18 if args.tie else None, n_total=args.n)
    m.run(args.steps, log_every=10)
    torch.cuda.synchronize()
    t2 = time.time()
    err = [float((t.kd.detach() - t.truth).abs()[18:].mean()) for t in tasks]
    if rank == 0:
        print("scenes/rank %d  targets %.2fs  optimise %.2fs  mean |Kd - truth| (cube) %.4f" % (
            len(tasks), t1 - t0, t2 - t1, sum(err) / max(1, len(err))))
    if ws > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
