"""The fused forward's in-phase refill: in the brute-force
instances of the fused render a lane whose path has just ended takes its next
sample inside the shading phase, and a group's pixel index math is done once
per group.  Only WHICH lane runs a sample changes, and when: every sample
keeps its seed, its draws and its arithmetic, so the fused frame must equal
the unfused two-kernel render of the same rows (ipt_render_samples_sm_dev +
ipt_pixel_mean_sm_dev, which this change does not touch) bit for bit, and for
two of the cases the oracle's render_samples + pixel_mean.

The shapes are the smallest at which the new code can go wrong: every lane
refilling in phase every iteration (0 bounces), groups that end mid-wave with
non-power-of-two W and spp, the headline's group shape with a one-pixel last
chunk, one pixel per group, unbounded paths that hold their slots, the Phong
(SPEC) instance, an interleaved share of rows, a scene that most camera rays
miss, and the material batch's fused forward."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, CORNELL_MTL, CORNELL_OBJ, SCENE0, product_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PHONG = CORNELL + [((0, -1.5, 4), (0, 0.3, 0), (1, 1, 1), os.path.join(ASSETS, "phong", "cube_phong.obj"),
                    os.path.join(ASSETS, "phong", "cube_phong.mtl"))]
# the camera sits at the origin looking down +z: with the box moved aside most
# camera rays pass it (a few meet the outside of its right wall)
ASIDE = [((3.6, 0, 4), (0, 0, 0), (2, 2, 2), CORNELL_OBJ, CORNELL_MTL)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes():
    return {n: product_scene(r) for n, r in (("cornell", CORNELL), ("scene0", SCENE0), ("phong", PHONG),
                                             ("aside", ASIDE))}


def two_kernel(P, W, H, spp, mb, seed, row_begin=0, row_end=None, row_step=1):
    """The unfused render of the same rows, (rows, W, 3)."""
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    p = N.make_params(W, H, spp, mb, seed, row_begin, row_end, row_step)
    rows = len(range(row_begin, H if row_end is None else row_end, row_step))
    samples = torch.empty((spp * rows * W, 3), device="cuda")
    hdr = torch.empty((rows * W, 3), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    N.check(L.ipt_render_samples_sm_dev(P.handle, C.byref(p), None, samples.data_ptr(), st))
    N.check(L.ipt_pixel_mean_sm_dev(samples.data_ptr(), rows * W, spp, hdr.data_ptr(), None, st))
    return hdr.cpu().numpy().reshape(rows, W, 3)


CASES = [
    ("cornell", 16, 8, 8, 0, 5, True),       # 0 bounces: every vertex ends its path, every lane refills in phase
    ("scene0", 13, 7, 5, 1, 9, True),        # W and spp no powers of two; groups end mid-wave
    ("cornell", 33, 17, 64, 4, 3, False),    # the headline's group shape (4 pixels); last chunk of 1 pixel
    ("cornell", 9, 5, 256, 4, 1, False),     # one pixel per group
    ("scene0", 16, 8, 8, None, 4, False),    # unbounded: long paths hold their slots
    ("phong", 16, 8, 16, 4, 6, False),       # the SPEC instance
    ("aside", 16, 8, 32, 4, 2, False),       # most camera rays miss: missed lanes refill in phase again and again
]


@pytest.mark.parametrize("name,W,H,spp,mb,seed,with_oracle", CASES)
def test_fused_equals_two_kernel(scenes, oracle, name, W, H, spp, mb, seed, with_oracle):
    P = scenes[name]
    hdr = P.render(W, H, spp, mb, seed)
    assert np.array_equal(bits(hdr), bits(two_kernel(P, W, H, spp, mb, seed)))
    if with_oracle:
        Q = oracle.OracleScene(CORNELL if name == "cornell" else SCENE0)
        s, _ = Q.render_samples(W, H, spp, mb, seed)
        hq, _ = oracle.pixel_mean(s, W * H, spp)
        assert np.array_equal(bits(hdr.reshape(-1, 3)), bits(hq))


def test_rays_that_miss_give_black_pixels(scenes):
    """The box moved aside: a camera ray that misses adds nothing, so the
    pixels that look past the box (the unfused render's exact zeros, at least
    the half of the frame on the far side) are exactly 0, and the box is
    still seen somewhere."""
    P = scenes["aside"]
    hdr = P.render(16, 8, 32, 4, 2)
    black = np.all(bits(two_kernel(P, 16, 8, 32, 4, 2)) == 0, axis=-1)
    assert black.mean() >= 0.5 and not black.all()
    assert np.all(bits(hdr)[black] == 0)
    assert np.any(hdr[~black] != 0)


def test_interleaved_share(scenes):
    """Rows 1, 4, 7, ... of 24 (row0 / row_step through the per-group pixel
    entries) == the two-kernel render of those rows == the full frame's rows."""
    P = scenes["scene0"]
    W, H, spp, mb, seed = 20, 24, 16, 4, 8
    share = P.render(W, H, spp, mb, seed, 1, H, row_step=3)
    assert np.array_equal(bits(share), bits(two_kernel(P, W, H, spp, mb, seed, 1, H, 3)))
    assert np.array_equal(bits(share), bits(P.render(W, H, spp, mb, seed)[1::3]))


def test_material_batch_forward_equals_single(scenes):
    """ipt_render_mat_batch_dev (the fused forward with one material table
    per set) for S = 2 sets == the same sets rendered one by one."""
    from inverse_path_tracer_amd import torch_ops

    P = scenes["phong"]
    W, H, spp, mb, seed, stride = 24, 12, 32, 4, 21, 1 << 20
    kd0 = torch.tensor(P.materials, device="cuda:0")
    kd = torch.stack([kd0 * (0.5 + 0.25 * b) for b in range(2)])
    ks = torch.stack([torch.full_like(kd0, 0.2 + 0.3 * b) for b in range(2)])
    with torch.no_grad():
        img = torch_ops.render_materials_batch(P, kd, ks, None, W, H, spp, mb, seed=seed, seed_stride=stride)
        for b in range(2):
            one = torch_ops.render_materials(P, kd[b].clone(), ks[b].clone(), None, W, H, spp, mb,
                                             seed=seed + b * stride)
            assert torch.equal(img[b], one)
