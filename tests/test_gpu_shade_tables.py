"""Small-scene shading tables (scene_layout.h TriShade / EmitShade, DESIGN.md
§23): with nT <= 32 and nE <= 16 the brute-force instances read normals,
sampling frames, Ke, the emitters' vertices, CDF and pmf from packed LDS
records instead of TriGeom / TriMat / the emitter arrays in global memory,
and walk the emitter CDF wave-uniformly.  Only where operands come from
changes, so every case must equal the CPU oracle: per-sample radiance bit for
bit, the fused frame bit for bit (and equal to the two-kernel render of the
same rows), gradients at rtol 1e-9 (only the order of the fp64 atomics differs;
entries no path reaches are exactly 0 on both sides).

The shapes are the smallest that reach each path: more than one workgroup's
worth of samples, odd sizes with partial groups, a 14-emitter scene whose CDF
walk takes several steps with different emitters inside a wave, an 18-emitter
scene that must fall back to the old reads, faces that are not axis-flat (the
blended normal at the vertex and in the emitter term), the Phong (SPEC)
instance, both bounded adjoint instances, and an interleaved share of rows.
One case counts the launches that ran a trace_shade_kernel instance
(ipt_debug_shade_launches), so that the tables are known to be taken where
they fit and left out where they do not."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ASSETS, CORNELL, CORNELL_MTL, CORNELL_OBJ, CUBE_KD, CUBE_OBJ, SCENE0, product_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CUBE_AT = ((0, -1.5, 4), (0, 0, 0), (1, 1, 1))
TURNED = ((0, -1.5, 4), (0.3, 0.5, 0.2), (1, 1, 1))
PHONG = CORNELL + [(CUBE_AT[0], (0, 0.3, 0), CUBE_AT[2], os.path.join(ASSETS, "phong", "cube_phong.obj"),
                    os.path.join(ASSETS, "phong", "cube_phong.mtl"))]


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def glow_cube(tmp):
    """(obj, mtl) under tmp: shapes/cube.obj under one emissive material."""
    mtl = os.path.join(str(tmp), "glowcube.mtl")
    with open(mtl, "w") as f:
        f.write("newmtl glow\nKd 0.4 0.5 0.6\nKe 3 2 1\n")
    body = open(CUBE_OBJ).read()
    i = body.index("\nf ") + 1
    obj = os.path.join(str(tmp), "glowcube.obj")
    with open(obj, "w") as f:
        f.write(body[:i] + "mtllib glowcube.mtl\nusemtl glow\n" + body[i:])
    return obj, mtl


def all_ke_mtl(tmp):
    """The Cornell box's MTL with a different nonzero Ke on every material."""
    out, n = [], 0
    for line in open(CORNELL_MTL):
        if line.split()[:1] == ["Ke"]:
            n += 1
            line = "Ke %g %g %g\n" % (0.5 * n, 0.25 * n + 1, 3.0 / n)
        out.append(line)
    assert n == 6
    mtl = os.path.join(str(tmp), "all_ke.mtl")
    with open(mtl, "w") as f:
        f.writelines(out)
    return mtl


@pytest.fixture(scope="module")
def recs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shade_tables")
    gobj, gmtl = glow_cube(tmp)
    return {
        "cornell": CORNELL,
        "scene0": SCENE0,
        "glow": CORNELL + [CUBE_AT + (gobj, gmtl)],
        "all_ke": [CORNELL[0][:3] + (CORNELL_OBJ, all_ke_mtl(tmp))],
        "turned": CORNELL + [TURNED + (CUBE_OBJ, CUBE_KD)],
        "turned_glow": CORNELL + [TURNED + (gobj, gmtl)],
        "phong": PHONG,
    }


@pytest.fixture(scope="module")
def pairs(recs, oracle):
    """name -> (product scene, oracle scene), loaded once."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (product_scene(recs[name]), oracle.OracleScene(recs[name]))
        return made[name]

    yield get
    for P, _ in made.values():
        P.close()


def two_kernel(P, W, H, spp, mb, seed):
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    p = N.make_params(W, H, spp, mb, seed, 0, None, 1)
    samples = torch.empty((spp * H * W, 3), device="cuda")
    hdr = torch.empty((H * W, 3), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    N.check(L.ipt_render_samples_sm_dev(P.handle, C.byref(p), None, samples.data_ptr(), st))
    N.check(L.ipt_pixel_mean_sm_dev(samples.data_ptr(), H * W, spp, hdr.data_ptr(), None, st))
    return hdr.cpu().numpy().reshape(H, W, 3)


def check_forward(oracle, P, Q, W, H, spp, mb, seed):
    want, _ = Q.render_samples(W, H, spp, mb, seed)
    got = P.render_samples(W, H, spp, mb, seed)
    assert np.array_equal(bits(got), bits(want))
    assert np.any(want != 0)
    hdr = P.render(W, H, spp, mb, seed)
    hq, _ = oracle.pixel_mean(want, W * H, spp)
    assert np.array_equal(bits(hdr.reshape(-1, 3)), bits(hq))
    assert np.array_equal(bits(hdr), bits(two_kernel(P, W, H, spp, mb, seed)))
    return hdr


def check_adjoint(P, Q, W, H, spp, mb, seed):
    adj = np.random.RandomState(seed).uniform(-1, 1, (H, W, 3)).astype(np.float32)
    want = Q.adjoint(W, H, spp, mb, seed, adj)
    assert np.any(want != 0)
    np.testing.assert_allclose(P.adjoint(adj, W, H, spp, mb, seed), want, rtol=1e-9, atol=0)


# name, nT, nE, W, H, spp, max_bounces, seed
FORWARD = [
    ("cornell", 18, 2, 32, 32, 8, 4, 11),        # tables on; several workgroups' worth of samples
    ("cornell", 18, 2, 33, 17, 5, None, 12),     # odd sizes, partial groups, unbounded paths
    ("scene0", 30, 2, 24, 24, 4, 4, 13),
    ("glow", 30, 14, 24, 24, 4, 4, 14),          # 14 emitters: a multi-step walk, mixed emitters inside a wave
    ("all_ke", 18, 18, 24, 24, 4, 4, 15),        # nE > 16: the old reads must run and match
    ("turned", 30, 2, 24, 24, 4, 4, 16),         # faces that are not axis-flat: the blended normal at the vertex
    ("turned_glow", 30, 14, 24, 24, 4, 4, 17),   # ... and in the emitter term
    ("phong", 30, 2, 24, 24, 4, 4, 18),          # the SPEC instance
]


@pytest.mark.parametrize("name,nT,nE,W,H,spp,mb,seed", FORWARD)
def test_forward_and_fused_equal_oracle(pairs, oracle, name, nT, nE, W, H, spp, mb, seed):
    P, Q = pairs(name)
    assert (P.nT, P.nE) == (nT, nE)
    if name.startswith("turned"):  # some triangle's vertex normal is off the axes
        vn = P.triangles()[18:, 9:12]
        assert np.any((np.abs(vn) > 1e-3).sum(1) > 1)
    check_forward(oracle, P, Q, W, H, spp, mb, seed)


@pytest.mark.parametrize("name", ["scene0", "cornell"])
@pytest.mark.parametrize("six_wave", [False, True])
def test_bounded_adjoint_both_instances(pairs, monkeypatch, name, six_wave):
    """Through trace_kernel<1> and, forced, the six-wave trace_kernel<5>.  (The
    six-wave launch of scenes/0 keeps its sixth workgroup per CU by leaving the
    tables out; the Cornell box's holds both.)"""
    if six_wave:
        monkeypatch.setenv("IPT_ADJW", "1")
    P, Q = pairs(name)
    check_adjoint(P, Q, 24, 24, 4, 4, 13)


@pytest.mark.parametrize("name,mb", [("glow", 4), ("glow", None), ("all_ke", 4), ("turned_glow", 4), ("phong", 4)])
def test_adjoint_equals_oracle(pairs, name, mb):
    P, Q = pairs(name)
    check_adjoint(P, Q, 24, 24, 4, mb, 21)


def test_interleaved_share(pairs):
    """Rows 1, 4, ... < 32 of the first case == the same rows of the full frame."""
    P, _ = pairs("cornell")
    W, H, spp, mb, seed = 32, 32, 8, 4, 11
    share = P.render(W, H, spp, mb, seed, 1, 32, row_step=3)
    assert np.array_equal(bits(share), bits(P.render(W, H, spp, mb, seed)[1:32:3]))


def test_tables_are_taken_where_they_fit_and_only_there(pairs, monkeypatch):
    """Launches that ran a trace_shade_kernel instance, counted by the library:
    the Cornell box's forwards, fused render and both bounded adjoints take the
    tables; the six-wave adjoint of scenes/0 (no sixth workgroup per CU with
    them), the 18-emitter scene and the unbounded adjoint do not."""
    from inverse_path_tracer_amd import _native as N

    L = N.lib()
    W, H, spp, mb, seed = 24, 24, 8, 4, 3
    adj = np.ones((H, W, 3), np.float32)

    def taken(call):
        before = L.ipt_debug_shade_launches()
        call()
        return L.ipt_debug_shade_launches() - before

    C0, S0, K18 = pairs("cornell")[0], pairs("scene0")[0], pairs("all_ke")[0]
    assert taken(lambda: C0.render_samples(W, H, spp, mb, seed)) > 0
    assert taken(lambda: C0.render(W, H, spp, mb, seed)) > 0
    assert taken(lambda: S0.render(W, H, spp, mb, seed)) > 0
    assert taken(lambda: pairs("phong")[0].render(W, H, spp, mb, seed)) > 0
    assert taken(lambda: K18.render(W, H, spp, mb, seed)) == 0
    assert taken(lambda: K18.adjoint(adj, W, H, spp, mb, seed)) == 0
    assert taken(lambda: C0.adjoint(adj, W, H, spp, None, seed)) == 0  # the unbounded adjoint keeps the old reads
    monkeypatch.setenv("IPT_ADJW", "0")  # trace_shade_kernel<1>
    assert taken(lambda: C0.adjoint(adj, W, H, spp, mb, seed)) > 0
    assert taken(lambda: S0.adjoint(adj, W, H, spp, mb, seed)) > 0
    monkeypatch.setenv("IPT_ADJW", "1")  # the six-wave instance
    assert taken(lambda: C0.adjoint(adj, W, H, spp, mb, seed)) > 0
    assert taken(lambda: S0.adjoint(adj, W, H, spp, mb, seed)) == 0


def test_longest_bounded_adjoint_still_launches(pairs):
    """The Cornell box's bounded adjoint holds 52 vertex records per lane in
    160 KiB of LDS (max_bounces = 51) without the tables and 51 with them: the
    launch leaves the tables out, it is not refused, and it matches the oracle."""
    from inverse_path_tracer_amd import _native as N

    P, Q = pairs("cornell")
    before = N.lib().ipt_debug_shade_launches()
    check_adjoint(P, Q, 8, 8, 2, 51, 5)
    assert N.lib().ipt_debug_shade_launches() == before
