"""The unbounded material adjoint over material sets x views, and MaterialOptimizer at
no bounce cap (run with -m gpu).

ipt_render_views_batch_unbounded_dev / ipt_adjoint_views_batch_unbounded_dev trace S material sets through V
cameras with the reference's own estimator (max_bounces = -1): launch set i = s * V + b is material set s seen
through view b at seed + i * seed_stride.  References:
  * through the scene's own camera (V = 1) the CPU oracle's material adjoint, every entry of Kd, Ks and Ke at
    rtol 1e-9 / atol 1e-12, and ipt_adjoint_mat_unbounded_dev at 1e-10 (the same floats in another fp64 order);
  * for other cameras -- the oracle has none -- the same launch under rings forced tiny (a replay restarts the
    path through its view's camera), the sum of V = 1 launches, and the bounded views adjoint at a cap no path
    comes near;
  * the decomposition: grad[s] is the S = 1 launch of set s at seed + s * V * stride, S != V in every mixed case.
Frames are the small ones of tests/test_gpu_views.py and tests/test_oracle_materials.py: 30x24x8 (W = 30 takes
the camera's dividing path), 32x32x8, a (3, 21, 2) row band, 19x13x7 at seed 2^33 + 11 (spp no power of two, a
64-bit seed, a partial last grab per set).  Material sets are per-triangle distinct; one lobe row carries Ks = 0
and one emitter row Ke = 0 in every set.
"""
import ctypes as C

import numpy as np
import pytest

import test_oracle_materials as OM
from conftest import product_scene
from test_gpu_materials import scene_b
from test_gpu_materials_unbounded import RINGS, ring, sphere_records
from test_gpu_views import RECORDS, bits, cameras
from test_gpu_views_batch import adj_sv, draw_sets, recovery_cameras, rotated_truth_files, row, same_sums

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TINY = [r for r in RINGS if r]
FULL = (0, None, 1)
BAND = (3, 21, 2)
F30, F32, F19 = (30, 24, 8, 2024), (32, 32, 8, 11), (19, 13, 7, 2 ** 33 + 11)  # W, H, spp, seed


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


class World:
    """This file's own scenes (their values are set and restored here) and oracles, built on first use."""

    def __init__(self, oracle, tmp):
        self.oracle = oracle
        self.records = dict(RECORDS)
        self.records["B"] = scene_b(tmp)
        self.records["sphere"] = sphere_records(tmp)
        self.P, self.Q = {}, {}

    def scene(self, name):
        if name not in self.P:
            self.P[name] = product_scene(self.records[name])
        return self.P[name]

    def oracle_scene(self, name):
        if name not in self.Q:
            self.Q[name] = self.oracle.OracleScene(self.records[name])
        return self.Q[name]

    def close(self):
        for p in self.P.values():
            p.close()


@pytest.fixture(scope="module")
def world(oracle, tmp_path_factory):
    w = World(oracle, tmp_path_factory.mktemp("vbu"))
    yield w
    w.close()


def band_kw(band):
    return dict(row_begin=band[0], row_end=band[1], row_step=band[2])


def stack(g):
    """(S, 3, nT, 3) from the three (S, nT, 3) blocks."""
    return np.stack(g, axis=1)


def launch(P, v, adj, mats, frame, stride=None, band=FULL):
    W, H, spp, seed = frame
    kd, ks, ke = mats
    return stack(P.adjoint_views_batch_unbounded(v, adj, kd, ks, ke, W, H, spp, seed, stride, **band_kw(band)))


def images(P, v, mats, frame, S, stride=None, band=FULL):
    W, H, spp, seed = frame
    kd, ks, ke = mats
    return P.render_views_batch_unbounded(v, kd, ks, ke, W, H, spp, seed, stride, n_sets=S, **band_kw(band))


def render_mat_unbounded_dev(P, mats, frame, band=FULL):
    """ipt_render_mat_dev at max_bounces = -1 with device overrides."""
    from inverse_path_tracer_amd import _native as N

    W, H, spp, seed = frame
    p = N.make_params(W, H, spp, None, seed, *band)
    t = [None if m is None else torch.tensor(np.ascontiguousarray(m, np.float32), device="cuda") for m in mats]
    hdr = torch.empty((p.rows, W, 3), device="cuda", dtype=torch.float32)
    N.check(N.lib().ipt_render_mat_dev(P.handle, C.byref(p), *[None if x is None else x.data_ptr() for x in t],
                                       hdr.data_ptr(), None, torch.cuda.current_stream().cuda_stream), "render_mat")
    return hdr.cpu().numpy()


class own_values:
    """The scene's own materials replaced for the block, restored afterwards."""

    def __init__(self, P, kd, ks, ke):
        self.P, self.new = P, (kd, ks, ke)

    def __enter__(self):
        self.old = self.P.material_params()[:3]
        self.P.set_material_params(*self.new)

    def __exit__(self, *exc):
        self.P.set_material_params(*self.old)
        return False


def oracle_blocks(Q, mats, frame, adj, band=FULL, stats=False):
    """The oracle's unbounded material adjoint under the set's values (its own restored)."""
    W, H, spp, seed = frame
    old = Q.material_params()
    Q.set_material_params(*mats)
    try:
        out = Q.adjoint_materials(W, H, spp, None, seed, adj, band[0], H if band[1] is None else band[1], band[2],
                                  stats=stats)
        img = Q.render(W, H, spp, None, seed)[0][band[0]:band[1]:band[2]]
    finally:
        Q.set_material_params(*old)
    return (np.stack(out[:3]), img) + ((out[3],) if stats else ())


def meets_oracle(got, want, P, tag):
    diffs = [OM.rel_diff(g, w) for g, w in zip(got, want)]
    print("GPU/oracle %s: Kd %.2e Ks %.2e Ke %.2e" % (tag, diffs[0], diffs[1], diffs[2]))
    for blk, g, w in zip(("Kd", "Ks", "Ke"), got, want):
        np.testing.assert_allclose(g, w, rtol=OM.RTOL, atol=OM.ATOL, err_msg="%s %s" % (tag, blk))
        assert np.array_equal(g == 0, w == 0), (tag, blk)
    assert not got[1][~P.lobe_mask].any() and not got[2][~P.emitter_mask].any()  # rows frozen at load
    assert want[0].any() and want[2].any() and (want[1].any() or not P.lobe_mask.any())


def one_set(P, seed=5):
    kd, ks, ke = draw_sets(P, 1, seed)
    return kd[0], ks[0], ke[0]


# ------------------------------------------------------------------ 1. own camera, S = 1, V = 1
OWN = [("A", F30, FULL), ("A", F32, FULL), ("A", F30, BAND), ("A", F19, FULL), ("B", F32, FULL), ("B", F19, FULL),
       ("cornell", F30, FULL), ("northstar", (32, 24, 4, 2024), FULL), ("sphere", (32, 24, 8, 12), FULL)]


@pytest.mark.parametrize("name,frame,band", OWN,
                         ids=["%s-%dx%dx%d%s" % (n, f[0], f[1], f[2], "-band" if b != FULL else "") for n, f, b in OWN])
def test_own_camera_is_the_oracle_and_the_single_set_launch(world, name, frame, band):
    P, Q = world.scene(name), world.oracle_scene(name)
    W, H, spp, seed = frame
    mats = one_set(P)
    sets = tuple(m[None] for m in mats)
    adj = np.random.RandomState(3).uniform(-1, 1, (1, 1, H, W, 3)).astype(np.float32)
    want, img_q, stats = oracle_blocks(Q, mats, frame, adj[0, 0], band, stats=True)
    # the tiny rings (17 slots at most) are meant to replay: a path of at least 17 vertices exists
    assert stats["longest"] >= OM.LONG and stats["escaped"] > 0, stats
    v = P.views(P.camera())
    img = images(P, v, sets, frame, 1, band=band)
    assert img.shape[:2] == (1, 1)
    assert np.array_equal(bits(img[0, 0]), bits(render_mat_unbounded_dev(P, mats, frame, band)))
    assert np.array_equal(bits(img[0, 0]), bits(img_q))
    with own_values(P, *mats):
        single = np.stack(P.adjoint_materials_unbounded(adj[0, 0], W, H, spp, seed, *band))
    for size in RINGS:
        with ring(size):
            got = launch(P, v, adj, sets, frame, band=band)[0]
        meets_oracle(got, want, P, "%s ring %s (longest path %d)" % (name, size, stats["longest"]))
        same_sums(got, single)
    v.close()


# ------------------------------------------------------------------ 2. own camera, S = 3, V = 1
@pytest.mark.parametrize("name,frame", [("A", F30), ("B", F19)], ids=["A", "B"])
def test_three_sets_through_the_own_camera(world, name, frame):
    P, Q = world.scene(name), world.oracle_scene(name)
    W, H, spp, seed = frame
    S, stride = 3, W * H * spp
    sets = draw_sets(P, S)
    adj = adj_sv(S, 1, W, H, seed=3)
    v = P.views(P.camera())
    g = launch(P, v, adj, sets, frame)
    img = images(P, v, sets, frame, S)
    for s in range(S):
        mats = tuple(m[s] for m in sets)
        fs = (W, H, spp, seed + s * stride)
        want, img_q = oracle_blocks(Q, mats, fs, adj[s, 0])
        meets_oracle(g[s], want, P, "%s set %d" % (name, s))
        assert np.array_equal(bits(img[s, 0]), bits(img_q)), s
        with own_values(P, *mats):
            same_sums(g[s], np.stack(P.adjoint_materials_unbounded(adj[s, 0], W, H, spp, fs[3])))
    assert not np.array_equal(img[0], img[1])
    v.close()


# ------------------------------------------------------------------ 3. other cameras
VIEW_FRAMES = {"A": F30, "sphere": (32, 24, 8, 12), "northstar": (32, 24, 4, 2024)}


@pytest.mark.parametrize("name", ["A", "sphere", "northstar"])
def test_three_views_replay_through_their_own_cameras(world, name):
    """A replay through the scene's camera instead of the view's changes every record of the path, hence the
    gradient: the default ring (long paths replay seldom or never) against rings under which every path longer
    than 1, 2, 17 or 4 vertices replays."""
    P = world.scene(name)
    W, H, spp, seed = frame = VIEW_FRAMES[name]
    st = W * H * spp
    cams = cameras(P)
    mats = tuple(m[None] for m in one_set(P))
    adj = adj_sv(1, 3, W, H)
    v = P.views(cams)
    g = launch(P, v, adj, mats, frame)[0]
    assert g[0].any() and g[2].any()
    for size in TINY:
        with ring(size):
            same_sums(launch(P, v, adj, mats, frame)[0], g)
    img = images(P, v, mats, frame, 1)
    kw = dict(kd=mats[0][0], ks=mats[1][0], ke=mats[2][0])
    assert np.array_equal(bits(img[0]), bits(P.render_views(v, W, H, spp, None, seed, **kw)))
    assert not np.array_equal(img[0, 0], img[0, 1]) and not np.array_equal(img[0, 0], img[0, 2])
    total, parts = 0, []
    for b in range(3):
        one = P.views(cams[b:b + 1])
        fb = (W, H, spp, seed + b * st)
        parts.append(launch(P, one, adj[:, b:b + 1], mats, fb)[0])
        for size in ((1, 1), (1, 4)):
            with ring(size):
                same_sums(launch(P, one, adj[:, b:b + 1], mats, fb)[0], parts[-1])
        total = total + parts[-1]
        one.close()
    same_sums(g, total)
    assert not np.allclose(parts[0], parts[1], rtol=1e-3) and not np.allclose(parts[0], parts[2], rtol=1e-3)
    v.close()


# ------------------------------------------------------------------ 4. against the bounded views adjoint
# The bounded adjoint keeps max_bounces + 1 records per lane in LDS: about 29 bounces on scene A (5-word records),
# more on Cornell (3 words).  Frames and seeds were chosen so that the precondition below holds for all three
# cameras.
CAPPED = [("A", (30, 24, 8, 77), 28), ("A", (32, 32, 8, 3), 28), ("cornell", (30, 24, 8, 5), 40)]


@pytest.mark.parametrize("name,frame,cap", CAPPED, ids=["A-30x24x8", "A-32x32x8", "cornell"])
def test_equals_the_bounded_views_adjoint_at_a_cap_no_path_reaches(world, name, frame, cap):
    P = world.scene(name)
    W, H, spp, seed = frame
    st = W * H * spp
    cams = cameras(P)
    mats = tuple(m[None] for m in one_set(P))
    kw = dict(kd=mats[0][0], ks=mats[1][0], ke=mats[2][0])
    adj = adj_sv(1, 3, W, H)
    v = P.views(cams)
    # the precondition, for every camera: the frame at the cap and four bounces below it is the frame at -1
    free = P.render_views(v, W, H, spp, None, seed, **kw)
    for mb in (cap, cap - 4):
        capped = P.render_views(v, W, H, spp, mb, seed, **kw)
        for b in range(3):
            assert np.array_equal(bits(capped[b]), bits(free[b])), "camera %d: a path comes near %d bounces" % (b, mb)
    got = launch(P, v, adj, mats, frame)[0]
    want = P.adjoint_views(v, adj[0], W, H, spp, cap, seed, **kw)
    print("%s V = 3 against the cap of %d: %.2e" % (name, cap, OM.rel_diff(got, want)))
    same_sums(got, want)
    for b in range(3):  # no camera is left out
        one = P.views(cams[b:b + 1])
        fb = (W, H, spp, seed + b * st)
        got = launch(P, one, adj[:, b:b + 1], mats, fb)[0]
        want = P.adjoint_views(one, adj[0, b:b + 1], W, H, spp, cap, fb[3], **kw)
        print("%s camera %d against the cap of %d: %.2e" % (name, b, cap, OM.rel_diff(got, want)))
        same_sums(got, want)
        assert want[0].any() and want[2].any()
        one.close()
    v.close()


# ------------------------------------------------------------------ 5. S x V
def check_pairs(P, cams, S, frame, stride, mats, band=FULL):
    """The S x V launch against S launches of one set: images bitwise, gradients to summation order."""
    W, H, spp, seed = frame
    V = cams.shape[0]
    v = P.views(cams)
    img = images(P, v, mats, frame, S, stride, band)
    rows = len(range(band[0], H if band[1] is None else band[1], band[2]))
    assert img.shape == (S, V, rows, W, 3) and img.dtype == np.float32
    adj = adj_sv(S, V, W, H)
    g = launch(P, v, adj, mats, frame, stride, band)
    assert g.shape == (S, 3, P.nT, 3) and g.dtype == np.float64
    st = W * H * spp if stride is None else stride
    worst = 0.0
    for s in range(S):
        m1 = tuple(None if m is None else m[s:s + 1] for m in mats)
        fs = (W, H, spp, seed + s * V * st)
        want = launch(P, v, adj[s:s + 1], m1, fs, stride, band)[0]
        worst = max(worst, OM.rel_diff(g[s], want))
        same_sums(g[s], want)
        assert want[0].any() and want[2].any()
        assert not g[s][1][~P.lobe_mask].any() and not g[s][2][~P.emitter_mask].any()
        one = P.render_views(v, W, H, spp, None, fs[3], seed_stride=stride, kd=row(mats[0], s), ks=row(mats[1], s),
                             ke=row(mats[2], s), **band_kw(band))
        assert np.array_equal(bits(img[s]), bits(one)), s
    print("S %d V %d: largest relative difference to the one-set launches %.2e" % (S, V, worst))
    if S > 1 and any(m is not None for m in mats):
        assert not np.array_equal(img[0], img[1]) and not np.allclose(g[0], g[1], rtol=1e-3)
    return v, img, adj, g


@pytest.mark.parametrize("which,band", [("all", FULL), ("null", FULL), ("all", BAND)],
                         ids=["overrides", "null", "band"])
def test_two_sets_by_three_views(world, which, band):
    P = world.scene("A")
    mats = draw_sets(P, 2) if which == "all" else (None, None, None)
    check_pairs(P, cameras(P), 2, (30, 24, 8, 77), None, mats, band)[0].close()


def test_two_sets_by_three_views_partial_grabs_and_bvh(world):
    """19x13x7: 1729 samples per pair, every pair's last grab partial; the north star: BVH, kd / pi from scratch."""
    P = world.scene("A")
    check_pairs(P, cameras(P), 2, F19, None, draw_sets(P, 2))[0].close()
    P = world.scene("northstar")
    kd, _, ke = draw_sets(P, 2)
    check_pairs(P, cameras(P), 2, (32, 24, 4, 2024), None, (kd, None, ke))[0].close()


def test_five_sets_by_three_views_do_not_divide_the_grid(world):
    P = world.scene("cornell")
    kd, _, ke = draw_sets(P, 5)
    check_pairs(P, cameras(P), 5, (30, 24, 8, 5), 1000, (kd, None, ke))[0].close()  # a stride of 1000 samples


# ------------------------------------------------------------------ 6. isolation
def test_sets_and_views_are_isolated(world):
    P = world.scene("A")
    W, H, spp, seed = frame = (30, 24, 8, 77)
    st = W * H * spp
    cams = cameras(P)
    mats = draw_sets(P, 2)
    v, _, adj, g = check_pairs(P, cams, 2, frame, None, mats)
    a = adj.copy()
    a[1] = 0  # zero in all views of set 1: grad[1] exactly zero, grad[0] unchanged
    h = launch(P, v, a, mats, frame)
    assert not h[1].any()
    same_sums(h[0], g[0])
    a = adj.copy()
    a[0, 1] = 0  # zero in view 1 of set 0: the sum of that set's two other single-view gradients
    h = launch(P, v, a, mats, frame)
    m0 = tuple(m[:1] for m in mats)
    want = 0
    for b in (0, 2):
        one = P.views(cams[b:b + 1])
        want = want + launch(P, one, adj[:1, b:b + 1], m0, (W, H, spp, seed + b * st))[0]
        one.close()
    same_sums(h[0], want)
    same_sums(h[1], g[1])
    v.close()


# ------------------------------------------------------------------ 7. the torch op
def test_torch_op_is_one_forward_and_one_backward_launch(world, monkeypatch):
    from inverse_path_tracer_amd import _native as N
    from inverse_path_tracer_amd import torch_ops

    P = world.scene("A")
    W, H, spp, _ = F30
    S, V = 2, 3
    v = P.views(cameras(P))
    kd0, ks0, ke0 = draw_sets(P, S)
    kd = torch.tensor(kd0, device="cuda", requires_grad=True)
    ks = torch.tensor(ks0, device="cuda", requires_grad=True)
    ke = torch.tensor(ke0, device="cuda")  # given, no gradient wanted
    calls = {}
    for name in [n for n in N.SIGNATURES if n.startswith(("ipt_render", "ipt_adjoint"))]:
        def wrap(*a, _f=getattr(N.lib(), name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        monkeypatch.setattr(N.lib(), name, wrap)
    img = torch_ops.render_views_batch_unbounded(P, v, kd, ks, ke, W, H, spp, seed=9)
    adj = adj_sv(S, V, W, H, seed=4)
    (img * torch.from_numpy(adj).cuda()).sum().backward()
    monkeypatch.undo()
    assert calls == {"ipt_render_views_batch_unbounded_dev": 1, "ipt_adjoint_views_batch_unbounded_dev": 1}, calls
    assert tuple(img.shape) == (S, V, H, W, 3) and img.dtype == torch.float32
    f9 = (W, H, spp, 9)
    assert np.array_equal(bits(img.detach().cpu().numpy()), bits(images(P, v, (kd0, ks0, ke0), f9, S)))
    g = launch(P, v, adj, (kd0, ks0, ke0), f9)
    assert kd.grad.dtype == torch.float32 and ks.grad.dtype == torch.float32 and ke.grad is None
    assert tuple(kd.grad.shape) == (S, P.nT, 3)
    assert np.allclose(kd.grad.cpu().numpy(), g[:, 0].astype(np.float32), rtol=1e-6, atol=0)
    assert np.allclose(ks.grad.cpu().numpy(), g[:, 1].astype(np.float32), rtol=1e-6, atol=0)
    # adjoint_seed replays the other stream: another estimate of the same gradient
    kd2 = torch.tensor(kd0, device="cuda", requires_grad=True)
    img2 = torch_ops.render_views_batch_unbounded(P, v, kd2, None, None, W, H, spp, seed=9, adjoint_seed=12345)
    assert np.array_equal(bits(img2.detach().cpu().numpy()), bits(images(P, v, (kd0, None, None), f9, S)))
    (img2 * torch.from_numpy(adj).cuda()).sum().backward()
    g2 = launch(P, v, adj, (kd0, None, None), (W, H, spp, 12345))
    assert np.allclose(kd2.grad.cpu().numpy(), g2[:, 0].astype(np.float32), rtol=1e-6, atol=0)
    assert not np.allclose(kd2.grad.cpu().numpy(), g[:, 0].astype(np.float32), rtol=1e-6, atol=0)
    img3 = torch_ops.render_views_batch_unbounded(P, v, kd2.detach(), None, None, W, H, spp, seed=9, seed_stride=1000)
    assert np.array_equal(bits(img3.cpu().numpy()), bits(images(P, v, (kd0, None, None), f9, S, 1000)))
    t = [torch.tensor(x, device="cuda") for x in (kd0, ks0, ke0)]
    with pytest.raises(ValueError, match="same number of sets"):
        torch_ops.render_views_batch_unbounded(P, v, t[0], t[1][:1], t[2], W, H, spp)
    with pytest.raises(ValueError, match="nT"):
        torch_ops.render_views_batch_unbounded(P, v, t[0][0], None, None, W, H, spp)
    with pytest.raises(ValueError, match="at least one"):
        torch_ops.render_views_batch_unbounded(P, v, None, None, None, W, H, spp)
    v.close()


# ------------------------------------------------------------------ 8. the optimizer at no bounce cap
def test_optimizer_one_step_at_the_documented_seeds(world, tmp_path):
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    W = H = 64
    spp, tspp, V, T, seed, tseed = 16, 32, 3, 2, 40, 7
    dev = torch.device("cuda")
    cams = recovery_cameras(world.scene("A"))
    learn = ("kd", "ks", "ke")
    tasks = build_tasks(rotated_truth_files(tmp_path), W, H, tspp, None, 0.5, dev, seed=tseed, learn=learn, views=cams)
    sc, vh = tasks[0].scene, tasks[0].views
    assert tasks[1].scene is sc and tasks[1].views is vh and len(vh) == V
    lobe = torch.tensor(sc.lobe_mask, device=dev)[:, None].float()
    emit = torch.tensor(sc.emitter_mask, device=dev)[:, None].float()
    frame = W * H * spp
    for i, t in enumerate(tasks):  # scene i view b: seed + 10^9 + (i V + b) W H target_spp, no bounce cap
        assert tuple(t.target.shape) == (V, H, W, 3)
        want = sc.render_views(vh, W, H, tspp, None, tseed + 10**9 + i * V * W * H * tspp, kd=t.truth.cpu().numpy(),
                               ks=t.truth_ks.cpu().numpy(), ke=t.truth_ke.cpu().numpy())
        assert np.array_equal(bits(t.target.cpu().numpy()), bits(want)), i
    assert not torch.equal(tasks[0].target, tasks[1].target)
    start = [[getattr(t, b).detach().clone() for b in learn] for t in tasks]
    opt = MaterialOptimizer(tasks, W, H, spp, None, lr=0.02, seed=seed, learn=learn, views=cams)
    opt.step()
    assert len(opt.leaves) == 1
    for i, t in enumerate(tasks):  # forward frames 2tTV + iV + b (t = 0), the adjoint T V frames later
        kd, ks, ke = (x.clone().requires_grad_(True) for x in start[i])
        base = seed + i * V * frame
        img = torch_ops.render_views_batch_unbounded(sc, vh, kd[None], (ks * lobe)[None], (ke * emit)[None], W, H, spp,
                                                     seed=base, seed_stride=frame, adjoint_seed=base + T * V * frame)
        loss = ((img[0] - t.target) ** 2).mean()
        loss.backward()
        for b, leaf in zip(learn, (kd, ks, ke)):
            got, want = opt.leaves[0][b].grad[i].cpu().numpy(), leaf.grad.cpu().numpy()
            print("scene %d %s: max |grad| %.3e, max |difference| %.3e" % (i, b, np.abs(want).max(),
                                                                           np.abs(got - want).max()))
            assert np.any(want != 0)
            assert np.allclose(got, want, rtol=1e-6, atol=0), (i, b)
        assert abs(float(opt.pending[0][1][i]) - float(loss.detach())) <= 1e-5 * float(loss.detach())


def test_optimizer_recovers_two_cubes_through_three_views_where_one_cannot(world, tmp_path):
    """tests/test_gpu_views_batch.py's recovery run at no bounce cap: the mean |Kd - truth| over the ten cube
    triangles that do not face the floor ends below half its start with three views, for both sets, and not with
    the default view alone at the same samples per step.  Measured: DESIGN.md §21.3."""
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    P = world.scene("A")
    W = H = 64
    cube = list(range(P.nT - 12, P.nT))
    tri = P.triangles()
    floor = [t for t in cube if tri[t, 19] < -0.99]
    assert len(floor) == 2
    seen = torch.tensor([t for t in cube if t not in floor], device="cuda")
    cams = recovery_cameras(P)
    files = rotated_truth_files(tmp_path)
    dev = torch.device("cuda")

    def run(views, spp):
        tasks = build_tasks(files, W, H, 4 * spp, None, 0.5, dev, views=views)
        for t in tasks:
            with torch.no_grad():
                t.kd[:cube[0]] = t.truth[:cube[0]]
        err = lambda: [float((t.kd.detach() - t.truth)[seen].abs().mean()) for t in tasks]  # noqa: E731
        e0 = err()
        MaterialOptimizer(tasks, W, H, spp, None, lr=0.02, learn=("kd",), views=views).run(200)
        assert all(len(t.history) == 200 for t in tasks)
        return e0, err()

    s3, e3 = run(cams, 16)
    s1, e1 = run(cams[:1], 48)
    for i in range(2):
        print("recovery set %d: start %.4f  three views %.4f  default view alone %.4f" % (i, s3[i], e3[i], e1[i]))
    for i in range(2):
        assert s1[i] == s3[i]
        assert e3[i] < 0.5 * s3[i], i
        assert not e1[i] < 0.5 * s1[i], i


def test_optimizer_without_views_learns_ks_and_ke_at_no_bounce_cap(world, tmp_path):
    """views=None, learn=("ks", "ke"), max_bounces=None: a NativeError at the first step before; now one launch per
    step through a one-view handle of the scene's own camera, at the views=None frames."""
    from inverse_path_tracer_amd import torch_ops
    from inverse_path_tracer_amd.optimize import MaterialOptimizer, build_tasks

    W = H = 32
    spp, tspp, T, seed, tseed = 8, 16, 2, 40, 7
    dev = torch.device("cuda")
    learn = ("ks", "ke")
    tasks = build_tasks(rotated_truth_files(tmp_path), W, H, tspp, None, 0.5, dev, seed=tseed, learn=learn)
    sc = tasks[0].scene
    assert tasks[1].scene is sc and tasks[0].views is None
    lobe = torch.tensor(sc.lobe_mask, device=dev)[:, None].float()
    emit = torch.tensor(sc.emitter_mask, device=dev)[:, None].float()
    for i, t in enumerate(tasks):  # targets keep their (H, W, 3) shape and the views=None seeds
        assert tuple(t.target.shape) == (H, W, 3)
        want = torch_ops.render_materials_unbounded(sc, t.truth, t.truth_ks, t.truth_ke, W, H, tspp,
                                                    seed=tseed + 10**9 + i * W * H * tspp)
        assert torch.equal(t.target, want), i
    start = [[getattr(t, b).detach().clone() for b in ("kd", "ks", "ke")] for t in tasks]
    opt = MaterialOptimizer(tasks, W, H, spp, None, lr=0.02, seed=seed, learn=learn)
    opt.step()
    assert len(opt.leaves) == 1 and set(opt.leaves[0]) == set(learn)
    frame = W * H * spp
    for i, t in enumerate(tasks):
        kd = start[i][0]
        ks, ke = (x.clone().requires_grad_(True) for x in start[i][1:])
        base = seed + i * frame
        img = torch_ops.render_materials_unbounded(sc, kd, ks * lobe, ke * emit, W, H, spp, seed=base,
                                                   adjoint_seed=base + T * frame)
        loss = ((img - t.target) ** 2).mean()
        loss.backward()
        for b, leaf in zip(learn, (ks, ke)):
            got, want = opt.leaves[0][b].grad[i].cpu().numpy(), leaf.grad.cpu().numpy()
            print("scene %d %s: max |grad| %.3e, max |difference| %.3e" % (i, b, np.abs(want).max(),
                                                                           np.abs(got - want).max()))
            assert np.any(want != 0)
            assert np.allclose(got, want, rtol=1e-6, atol=0), (i, b)
        assert abs(float(opt.pending[0][1][i]) - float(loss.detach())) <= 1e-5 * float(loss.detach())
    opt.run(2)
    assert all(len(t.history) == 3 for t in tasks)


# ------------------------------------------------------------------ 9. refusals on a device scene
def test_refusals_leave_the_stream_and_the_buffers_intact(world):
    from inverse_path_tracer_amd import _native as N

    P = world.scene("A")
    W, H, spp, seed = frame = (30, 24, 8, 21)
    S, V = 2, 3
    v = P.views(cameras(P))
    mats = draw_sets(P, S)
    adj = adj_sv(S, V, W, H)
    ref_img = images(P, v, mats, frame, S)
    ref_g = launch(P, v, adj, mats, frame)

    def intact():
        assert np.array_equal(bits(images(P, v, mats, frame, S)), bits(ref_img))
        same_sums(launch(P, v, adj, mats, frame), ref_g)

    dead = P.views(P.camera())
    dead.close()
    other_scene = world.scene("cornell")
    other = other_scene.views(other_scene.camera())
    for call in (lambda: images(P, dead, mats, frame, S), lambda: launch(P, dead, adj[:, :1], mats, frame)):
        with pytest.raises(N.NativeError, match="null views handle"):
            call()
        intact()
    with pytest.raises(N.NativeError, match="invalid render parameters"):
        images(P, v, mats, (W, H, 0, seed), S)
    intact()
    # through the C ABI: nothing is written into the refused call's buffers
    out = torch.zeros((S, V, H, W, 3), device="cuda")
    a = torch.tensor(adj, device="cuda")
    g = torch.zeros((S, 3, P.nT, 3), device="cuda", dtype=torch.float64)
    st = torch.cuda.current_stream().cuda_stream
    free = N.make_params(W, H, spp, None, seed)
    raw = C.c_void_p(dead.handle.value or 1)
    cases = [(other.handle, S, free, "another scene"), (raw, S, free, "not live"), (v.handle, 0, free, "n_sets"),
             (v.handle, 21846, free, "65535"),
             (v.handle, S, N.make_params(W, H, spp, 0, seed), "max_bounces must be -1"),
             (v.handle, S, N.make_params(W, H, spp, 4, seed), "ipt_adjoint_views_batch_dev"),
             (v.handle, S, N.make_params(W, H, spp, None, seed, 5, 3), "invalid render parameters"),
             (v.handle, S, N.make_params(0, H, spp, None, seed), "invalid render parameters")]
    for handle, n_sets, p, text in cases:
        N.lib().ipt_clear_error()
        assert N.lib().ipt_render_views_batch_unbounded_dev(P.handle, handle, C.byref(p), n_sets, 1, None, None, None,
                                                            out.data_ptr(), st) == -1
        assert text in N.last_error(), N.last_error()
        N.lib().ipt_clear_error()
        assert N.lib().ipt_adjoint_views_batch_unbounded_dev(P.handle, handle, C.byref(p), n_sets, 1, None, None, None,
                                                             a.data_ptr(), g.data_ptr(), st) == -1
        assert text in N.last_error(), N.last_error()
        assert float(out.abs().sum()) == 0 and float(g.abs().sum()) == 0
        intact()
    # a launch that fails after its counters and scratch are taken
    for call in (lambda: images(P, v, mats, frame, S), lambda: launch(P, v, adj, mats, frame)):
        N.lib().ipt_debug_fail_launches(1)
        try:
            with pytest.raises(N.NativeError, match="on request"):
                call()
        finally:
            N.lib().ipt_debug_fail_launches(0)
        intact()
    other.close()
    v.close()


def test_ring_slot_caches_of_the_two_unbounded_material_adjoints_are_their_own(world):
    """Alternating the new adjoint with ipt_adjoint_mat_unbounded_dev: each gives its lone-launch result."""
    P = world.scene("A")
    W, H, spp, seed = frame = F30
    v = P.views(cameras(P))
    adj = adj_sv(2, 3, W, H)
    mats = draw_sets(P, 2)
    adj1 = adj[0, 0]
    # each launch alone, on a scene that never ran the other kernel
    fresh = product_scene(RECORDS["A"])
    fv = fresh.views(cameras(fresh))
    lone_new = launch(fresh, fv, adj, mats, frame)
    fv.close()
    fresh.close()
    fresh = product_scene(RECORDS["A"])
    lone_old = np.stack(fresh.adjoint_materials_unbounded(adj1, W, H, spp, seed))
    fresh.close()
    for _ in range(3):
        same_sums(np.stack(P.adjoint_materials_unbounded(adj1, W, H, spp, seed)), lone_old)
        same_sums(launch(P, v, adj, mats, frame), lone_new)
    v.close()
