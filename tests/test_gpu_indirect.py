"""One-bounce indirect light on the GPU (rr_indirect_at_device, rr_render_indirect, rr_render_indirect_device; DESIGN.md
§3.23).  The definition is a composition of public entries: a point's value is indirect_resolve of what
rr_color_at_device writes for its K indirect_rays, and a frame's points are over_point / normalv of rr_hit_at_device
over rr_camera_rays_device.  On scenes whose materials share one shininess the comparison is np.array_equal; the stock
mixed-shininess scenes get the bound rray.h's caveat allows, and the oracle the project's gate.  Device buffers are
torch tensors with a sentinel behind every output, as in tests/test_gpu_rays.py, whose helpers these tests use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import test_gpu_rays as Q  # noqa: E402  its helpers: same, sync, to_dev, camera_rays_dev, hit_dev, color_dev, SENT, TOL
import test_gpu_views_aov as V  # noqa: E402  its scenes, cameras, oracle records and environment switch

pytestmark = pytest.mark.gpu
SENT = Q.SENT
same = Q.same
SH = 50.0  # the one shininess of the scenes built here
COUNTERS = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "nan_rays")


@pytest.fixture(scope="module")
def R():
    import rray_amd

    if rray_amd.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")
    return rray_amd


@pytest.fixture(scope="module")
def renderer(R):
    r = R.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- scenes whose materials all share one shininess (rray.h: every value is then the composition's bit for bit) ----
def _floor_and_balls(b, reflective=0.0):
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.2, SH, reflective, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0.3, 0.3, 0.3))))
    for x, z, s, col in ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9))):
        b.sphere(transform=V.scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, SH, reflective, 0.0, 1.0),
                 pattern=b.pattern("solid", color=col))


def flat_scene(R):
    """a checker floor and three coloured spheres, two point lights"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (0.7, 0.7, 0.7))
    b.point_light((4, 5, 1), (0.3, 0.3, 0.4))
    _floor_and_balls(b)
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.5, 0))


def chain_scene(R):
    """the same with a reflective floor and spheres (the in-wave reflection chains)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    _floor_and_balls(b, reflective=0.3)
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.5, 0))


def group_scene(R):
    """the spheres and two cubes inside nested groups over the floor (G = 1)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, SH, 0.0, 0.0, 1.0),
            pattern=b.pattern("solid", color=(0.9, 0.9, 0.8)))
    g = b.group(transform=V.translate(0, 0, -4.5))
    h = b.group(transform=V.translate(-1.4, 0, 0), parent=g)
    b.sphere(transform=V.scale_at(0.8, 0, -0.2, 0), material=(0.1, 0.8, 0.3, SH, 0.0, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.9, 0.2, 0.2)), parent=h)
    b.cube(transform=V.scale_at(0.5, 1.2, -0.5, 0.3), material=(0.1, 0.8, 0.3, SH, 0.0, 0.0, 1.0),
           pattern=b.pattern("solid", color=(0.2, 0.3, 0.9)), parent=h)
    b.cube(transform=V.scale_at(0.6, 1.5, -0.4, 0), material=(0.1, 0.8, 0.3, SH, 0.0, 0.0, 1.0),
           pattern=b.pattern("solid", color=(0.2, 0.9, 0.3)), parent=g)
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.3, 0))


def csg_scene(R):
    """a lens and a cube minus a sphere over a floor: the general kernels (G = 2)"""
    b = R.SceneBuilder()
    b.point_light((-6, 8, 4), (1, 1, 1))
    m = (0.1, 0.8, 0.3, SH, 0.0, 0.0, 1.0)
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, SH, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(0.9, 0.9, 0.9)), b=b.pattern("solid", color=(0.1, 0.1, 0.1))))
    c = b.csg("intersection", transform=V.translate(-1.2, 0, -5))
    b.sphere(transform=V.translate(-0.4, 0, 0), material=m, pattern=b.pattern("solid", color=(0.9, 0.2, 0.2)), parent=c)
    b.sphere(transform=V.translate(0.4, 0, 0), material=m, pattern=b.pattern("solid", color=(0.2, 0.9, 0.2)), parent=c)
    d = b.csg("difference", transform=V.translate(1.3, 0, -5))
    b.cube(transform=V.scale_at(0.8, 0, 0, 0), material=m, pattern=b.pattern("solid", color=(0.2, 0.3, 0.9)), parent=d)
    b.sphere(material=m, pattern=b.pattern("solid", color=(0.9, 0.8, 0.1)), parent=d)
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.3, 0))


def glass_scene(R):
    """a glass sphere and a coloured one over the floor: reflection and refraction (the in-wave trees)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, SH, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0.8, 0.2, 0.2))))
    b.sphere(transform=V.scale_at(1.0, -0.6, 0.0, -4), material=(0.05, 0.1, 0.9, SH, 0.9, 0.9, 1.5),
             pattern=b.pattern("solid", color=(0.1, 0.1, 0.1)))
    b.sphere(transform=V.scale_at(0.6, 1.2, -0.4, -3.5), material=(0.1, 0.7, 0.3, SH, 0.0, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.2, 0.4, 0.9)))
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.4, 0))


def area_scene(R):
    """flat_scene's objects under an area light of 2 x 2 cells: the jittered shadow samples"""
    b = R.SceneBuilder()
    b.area_light((-3, 5, 1), (2, 0, 0), (0, 0, 2), (1, 1, 1), 2)
    _floor_and_balls(b)
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.5, 0))


SCENES = {"flat": flat_scene, "group": group_scene, "csg": csg_scene, "glass": glass_scene, "chain": chain_scene}


def mesh_scene(R):
    """the teapot over its floor: groups and triangles, mixed shininess"""
    s = V.yaml_scene(R, "c4_teapot.yaml", 16, 16)
    return s, s.camera


def lds_scene(R):
    """a fuzz scene small enough for culls staged in LDS (tests/test_gpu_views_aov.py VARIANTS)"""
    P, spec, _, _ = V.F.build(0)
    return P.b, V.F.cameras(P, spec, 16, 16)[0]


# ---- the entries through tensors with sentinels, and the composition of the public entries ----
def points_dev(r, P, N, ind, dev, stream=None, **kw):
    """rr_indirect_at_device over host arrays: (n, 3) f64"""
    n = len(P)
    p, nn = Q.to_dev(P, dev), Q.to_dev(N, dev)
    out = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
    Q.sync()
    r.indirect_at_device(n, p.data_ptr(), nn.data_ptr(), ind, out.data_ptr(), stream=stream, **kw)
    Q.sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "indirect_at_device wrote past its points"
    return a[:n]


def composed(R, r, P, N, ind, dev, first=0, **kw):
    """the definition through the public entries: indirect_rays in numpy, one color_at_device over the n * K rays,
    indirect_resolve"""
    rays = R.indirect_rays(P, N, ind, first)
    L = Q.color_dev(r, Q.to_dev(rays, dev), len(rays), dev, remaining=ind.remaining, **kw)
    return R.indirect_resolve(L, ind.samples)


def first_hits(R, r, cam, dev):
    """hit_at_device over camera_rays_device(cam): the records of the frame's samples"""
    n = cam.hsize * cam.vsize
    return Q.hit_dev(R, r, Q.camera_rays_dev(r, cam, dev), n, dev)


def composed_frame(R, r, cam, ind, dev, **kw):
    """A frame by the public entries over a full batch: a miss gets a placeholder ray whose result is dropped, so ray
    identities are i * K + k.  -> (plane (vsize, hsize, 3), hit mask (n,), the sum of the stats the frame must report:
    hit_at_device's over the camera's rays + color_at_device's over the rays of the samples that hit, only those)"""
    rec = first_hits(R, r, cam, dev)
    stats = {k: r.last_stats()[k] for k in COUNTERS}
    hit = rec["object"] >= 0
    P = np.ascontiguousarray(np.where(hit[:, None], rec["over_point"], [0.0, 1e6, 0.0]))
    N = np.ascontiguousarray(np.where(hit[:, None], rec["normalv"], [0.0, 1.0, 0.0]))
    K, n = ind.samples, len(rec)
    rays = R.indirect_rays(P, N, ind)
    L = Q.color_dev(r, Q.to_dev(rays, dev), n * K, dev, remaining=ind.remaining, **kw)
    G = R.indirect_resolve(L, K)
    G[~hit] = 0.0
    live = np.ascontiguousarray(rays.reshape(n, K, 6)[hit].reshape(-1, 6))
    if len(live):
        Q.color_dev(r, Q.to_dev(live, dev), len(live), dev, remaining=ind.remaining, **kw)
        st = r.last_stats()
        for k in COUNTERS:
            stats[k] += st[k]
    return G.reshape(cam.vsize, cam.hsize, 3), hit, stats


def frame_dev(R, r, cam, ind, dev, stream=None, aa=1, seed=0, jitter_mode=0):
    """rr_render_indirect_device into a tensor with a sentinel: (vsize, hsize, 3)"""
    n = cam.hsize * cam.vsize
    out = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
    o = R._lib.RenderOpts(aa, 0, seed, jitter_mode, 0, 1, 8, 0, 0, 0)
    Q.sync()
    r.render_indirect_device(cam, o, ind, out.data_ptr(), stream)
    Q.sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "render_indirect_device wrote past its plane"
    return a[:n].reshape(cam.vsize, cam.hsize, 3)


# ---- 1. points against the public entries ----
@pytest.mark.parametrize("name", list(SCENES))
def test_points_equal_the_composition_of_the_public_entries(R, renderer, dev, name):
    scene, cam_like = SCENES[name](R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 20, 13, 2)[1]
    rec = first_hits(R, renderer, cam, dev)
    rec = rec[rec["object"] >= 0]
    assert len(rec) >= 100, name
    rec = np.resize(rec, 257)  # the hits, repeated: a repeated point has another hash index and other rays
    coloured = False
    for n in (1, 63, 65, 257):
        P, N = np.ascontiguousarray(rec["over_point"][:n]), np.ascontiguousarray(rec["normalv"][:n])
        for K in (1, 3, 16, 65):  # 64 % 3 and 64 % 65 != 0: a point's rays straddle waves
            for remaining in (0, 2):
                ind = R.Indirect(K, remaining, seed=n * 1000 + K)
                want = composed(R, renderer, P, N, ind, dev)
                traced = renderer.last_stats()  # color_at_device's over the n * K rays
                got = points_dev(renderer, P, N, ind, dev)
                assert same(got, want), (name, n, K, remaining)
                st = renderer.last_stats()
                assert st["samples"] == n and traced["samples"] == n * K and st["rays"] >= n * K, (name, st)
                assert {k: st[k] for k in COUNTERS} == {k: traced[k] for k in COUNTERS}, (name, n, K, remaining)
                coloured = coloured or bool((got.max(axis=1) - got.min(axis=1)).max() > 0.01)
    assert coloured, name  # coloured surroundings send coloured light


# ---- 2. frames against the public entries ----
@pytest.mark.parametrize("W,H", [(7, 5), (13, 5), (16, 4), (65, 1)], ids=["7x5", "13x5", "16x4", "65x1"])
def test_frames_equal_the_composition_of_the_public_entries(R, renderer, dev, W, H):
    cases = [(name, fn, {}) for name, fn in SCENES.items()] + [("area", area_scene, dict(seed=9, jitter_mode=0)),  # 0: the hashed jitter is on
                                                                  ("area_centres", area_scene, dict(seed=9, jitter_mode=1))]
    for name, fn, kw in cases:
        scene, cam_like = fn(R)
        renderer.upload(scene)
        cam = V.ring(R, cam_like, W, H, 2)[1]
        for K in (3, 16):  # 64 % 3 != 0: a point's rays straddle waves
            ind = R.Indirect(K, 1 if name != "glass" else 2, seed=5 + K)
            want, hit, stats = composed_frame(R, renderer, cam, ind, dev, **kw)
            got = renderer.render_indirect(cam, ind, **kw)
            assert same(got["indirect"], want), (name, W, H, K)
            st = got["stats"]
            assert st["samples"] == W * H and st["kernel_ms"] > 0, (name, st)
            assert {k: st[k] for k in COUNTERS} == stats, (name, W, H, K)
            assert same(frame_dev(R, renderer, cam, ind, dev, **kw), want), (name, W, H, K)
    # never averaged: with aa = 2 the camera is the supersampled one and the plane has its size
    scene, cam_like = flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 2 * W, 2 * H, 1)[0]
    ind = R.Indirect(4, 1, seed=2)
    got = renderer.render_indirect(cam, ind, aa=2)["indirect"]
    assert got.shape == (2 * H, 2 * W, 3) and same(got, renderer.render_indirect(cam, ind)["indirect"])


def test_the_area_lights_keep_the_calls_seed(R, renderer, dev):
    scene, cam_like = area_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 13, 5, 1)[0]
    ind = R.Indirect(3, 1, seed=4)
    a = renderer.render_indirect(cam, ind, seed=9, jitter_mode=0)["indirect"]  # 0: the hashed jitter
    assert not same(a, renderer.render_indirect(cam, ind, seed=10, jitter_mode=0)["indirect"])
    assert not same(a, renderer.render_indirect(cam, ind, seed=9, jitter_mode=1)["indirect"])  # 1: cell centres
    assert not same(a, renderer.render_indirect(cam, R.Indirect(3, 1, seed=5), seed=9, jitter_mode=0)["indirect"])
    assert same(a, renderer.render_indirect(cam, ind, seed=9, jitter_mode=0)["indirect"])  # repeatable
    # with cell centres the call's seed plays no part, the directions' seed still does
    c = renderer.render_indirect(cam, ind, seed=9, jitter_mode=1)["indirect"]
    assert same(c, renderer.render_indirect(cam, ind, seed=10, jitter_mode=1)["indirect"])
    assert not same(c, renderer.render_indirect(cam, R.Indirect(3, 1, seed=5), seed=9, jitter_mode=1)["indirect"])


# ---- 3. misses cost nothing ----
def test_a_frame_in_which_half_the_samples_miss(R, renderer, dev):
    scene, _ = flat_scene(R)
    renderer.upload(scene)
    cam = R.camera(24, 16, math.pi / 3, V.translate(0, -0.5, 0))  # level with the horizon: sky above it
    ind = R.Indirect(16, 1, seed=3)
    got = renderer.render_indirect(cam, ind)
    obj = renderer.render_aov(cam, planes=("object",))["object"]
    miss = obj < 0
    assert 0.3 < miss.mean() < 0.7
    assert (got["indirect"][miss] == 0.0).all() and (got["indirect"][~miss] > 0.0).any()
    want, hit, stats = composed_frame(R, renderer, cam, ind, dev)
    assert same(hit.reshape(16, 24), ~miss) and same(got["indirect"], want)
    # the rays of a color_at_device over the hits' rays only, on top of the camera's
    rec = first_hits(R, renderer, cam, dev)
    rays = R.indirect_rays(rec["over_point"][hit], rec["normalv"][hit], ind)  # any identities: the count is what matters
    Q.color_dev(renderer, Q.to_dev(rays, dev), len(rays), dev, remaining=1)
    assert got["stats"]["rays"] == 24 * 16 + renderer.last_stats()["rays"]
    assert {k: got["stats"][k] for k in COUNTERS} == stats
    assert got["stats"]["rays"] < 24 * 16 + 24 * 16 * 16  # fewer than a full batch would take (remaining 1, nothing reflects)


def test_a_frame_of_sky_traces_nothing(R, renderer, dev):
    scene, _ = flat_scene(R)
    renderer.upload(scene)
    up = R.camera(9, 7, math.pi / 4, [1, 0, 0, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, 0, 0, 1])  # looking along +y or -y
    got = renderer.render_indirect(up, R.Indirect(16, 2, seed=1))
    obj = renderer.render_aov(up, planes=("object",))["object"]
    if (obj >= 0).any():  # the other way round
        up = R.camera(9, 7, math.pi / 4, [1, 0, 0, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1])
        got = renderer.render_indirect(up, R.Indirect(16, 2, seed=1))
        obj = renderer.render_aov(up, planes=("object",))["object"]
    assert (obj < 0).all()
    assert (got["indirect"] == 0.0).all() and got["stats"]["rays"] == 63 and got["stats"]["shade_events"] == 0
    assert (frame_dev(R, renderer, up, R.Indirect(16, 2, seed=1), dev) == 0.0).all()


# ---- 4. passes ----
@pytest.mark.parametrize("env", [dict(RRAY_INDIRECT_PASS="64"), dict(RRAY_INDIRECT_PASS="1"), dict(RRAY_BATCH="1024")],
                         ids=["pass64", "pass1_rounds_up", "batch1024"])
def test_passes_equal_the_default_contexts_frame(R, renderer, dev, env):
    """41 x 30 = 1230 samples: under RRAY_INDIRECT_PASS=64 twenty passes, the last of 14 points; under RRAY_BATCH=1024
    two passes of 1024 and 206 points whose rays (K = 16: 16 384) are traced in chunks of 1024 list slots."""
    with V.environment(**env):  # read when a context is created
        r = R.Renderer(0)
    try:
        for name in ("flat", "group", "glass"):
            scene, cam_like = SCENES[name](R)
            cam = V.ring(R, cam_like, 41, 30, 1)[0]
            renderer.upload(scene)
            r.upload(scene)
            for ind in (R.Indirect(3, 1, seed=8), R.Indirect(16, 2, seed=1)):
                want = renderer.render_indirect(cam, ind)
                got = r.render_indirect(cam, ind)
                assert same(got["indirect"], want["indirect"]), (env, name, ind)
                for k in COUNTERS + ("samples",):
                    assert got["stats"][k] == want["stats"][k], (env, name, k)
                assert same(frame_dev(R, r, cam, ind, dev), want["indirect"])  # the sentinel behind the last pass
        # and the point query in passes: 257 points
        rec = first_hits(R, renderer, cam, dev)
        rec = np.resize(rec[rec["object"] >= 0], 257)
        P, N = np.ascontiguousarray(rec["over_point"]), np.ascontiguousarray(rec["normalv"])
        ind = R.Indirect(5, 2, seed=3)
        assert same(points_dev(r, P, N, ind, dev), points_dev(renderer, P, N, ind, dev))
    finally:
        r.close()


# ---- 5. the stock scenes, whose materials mix shininess values ----
@pytest.mark.parametrize("name", ["flat", "mesh", "lds"])
def test_mixed_shininess_scenes_within_the_pow_bound(R, renderer, dev, name):
    """rray.h's caveat: in a wave that mixes shininess values a specular term may move by an ulp of pow with the wave's
    composition, and the frame's waves hold only the hits' rays.  OpenCL bounds pow by 16 ulp, 3.6e-15 per specular
    term; a margin of a few hundred for lights x levels gives 1e-12 * max(1, |value|) per channel."""
    scene, cam_like = {"flat": V.flat_scene, "mesh": mesh_scene, "lds": lds_scene}[name](R)
    renderer.upload(scene)
    worst, exact, count = 0.0, 0, 0
    for W, H in ((13, 5), (16, 12)):
        cam = V.ring(R, cam_like, W, H, 2)[1]
        for K in (3, 16):
            ind = R.Indirect(K, 2, seed=K)
            want, hit, stats = composed_frame(R, renderer, cam, ind, dev)
            got = renderer.render_indirect(cam, ind)
            d = np.abs(got["indirect"] - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(d.max()))
            exact += int((got["indirect"] == want).sum())
            count += want.size
            assert np.isfinite(got["indirect"]).all()
            assert {k: got["stats"][k] for k in COUNTERS} == stats, (name, W, H, K)
    print(f"{name}: frame against composition: largest |d| / max(1, |value|) = {worst:.3g}, bit-exact share {exact / count:.6f}")
    assert worst <= 1e-12, (name, worst)


# ---- 6. the oracle itself ----
def oracle_scene(R, oracle):
    """a white floor, a red cube and a white sphere resting on it, one shininess, a black sky; on both sides"""
    floor = (0.1, 0.9, 0.0, SH, 0.0, 0.0, 1.0)
    body = (0.1, 0.9, 0.3, SH, 0.0, 0.0, 1.0)
    cub, sph = V.scale_at(0.8, -1.5, 0.8, 0.0), V.scale_at(0.8, 1.5, 0.8, 0.0)
    b, o = R.SceneBuilder(), oracle.Oracle()
    for s in (b, o):
        s.point_light((-2.0, 6.0, -5.0), (1, 1, 1))
    b.plane(material=floor, pattern=b.pattern("solid", color=(1, 1, 1)))
    b.cube(transform=cub, material=body, pattern=b.pattern("solid", color=(1, 0, 0)))
    b.sphere(transform=sph, material=body, pattern=b.pattern("solid", color=(1, 1, 1)))
    o.add("plane", material=floor, pattern=o.pattern("solid", color=(1, 1, 1)))
    o.add("cube", transform=cub, material=body, pattern=o.pattern("solid", color=(1, 0, 0)))
    o.add("sphere", transform=sph, material=body, pattern=o.pattern("solid", color=(1, 1, 1)))
    view = oracle.Oracle.mat.view_transform((0.0, 2.0, -5.0), (0.0, 0.8, 0.0), (0.0, 1.0, 0.0))
    return b, o, view


def oracle_frame(R, oracle, o, cam, ind):
    """the definition on the oracle: P and N from prepare_computations, every L from color_at over indirect_rays"""
    ocam = oracle.Oracle.camera(cam.hsize, cam.vsize, cam.field_of_view, list(cam.transform))
    rec = V.oracle_hits(R, o, V.camera_rays(oracle, ocam))
    hit = rec["object"] >= 0
    N = np.where(hit[:, None], rec["normalv"], [0.0, 1.0, 0.0])
    rays = R.indirect_rays(rec["over_point"], N, ind).reshape(len(rec), ind.samples, 6)
    L = np.zeros((len(rec), ind.samples, 3))
    for i in np.flatnonzero(hit):
        for k in range(ind.samples):
            L[i, k] = o.color_at(rays[i, k, :3].tolist(), rays[i, k, 3:].tolist(), ind.remaining)[:3]
    G = R.indirect_resolve(L.reshape(-1, 3), ind.samples)
    G[~hit] = 0.0
    return G.reshape(cam.vsize, cam.hsize, 3), rec


def test_a_frame_against_the_oracle(R, renderer):
    """12 x 8, K = 4, remaining 1.  Every sample within the project's gate TOL = 1e-5; no sample is set aside.  The
    picture follows from the scene: the floor beside the red cube's lit faces receives red light; the floor beside the
    white sphere receives more light than the open floor far from both, whose gathered rays mostly leave for the black
    sky; a miss is black."""
    import oracle

    b, o, view = oracle_scene(R, oracle)
    renderer.upload(b)
    W, H = 12, 8
    cam = R.camera(W, H, math.pi / 3, view)
    ind = R.Indirect(4, 1, seed=2026)
    got = renderer.render_indirect(cam, ind)["indirect"]
    want, rec = oracle_frame(R, oracle, o, cam, ind)
    hit = (rec["object"] >= 0).reshape(H, W)
    err = float(np.abs(got - want).max())
    print(f"indirect frame against the oracle: {int(hit.sum())} hits of {W * H}, max|d|={err:.3g}, "
          f"bit-exact share {float(np.mean(got == want)):.6f}")
    assert 40 < hit.sum() < W * H  # some sky
    assert np.isfinite(got).all() and err <= Q.TOL
    assert (got[~hit] == 0.0).all()
    _picture(rec, got.reshape(-1, 3))


def _picture(rec, G):
    """the assertions about the image, on (n, 3) values of the records' samples"""
    P = rec["over_point"]
    floor = rec["object"] == 0
    # the cube spans x in [-2.3, -0.7], z in [-0.8, 0.8]; the sphere is centred at (1.5, 0.8, 0) with radius 0.8
    d_cube = np.maximum(np.maximum(np.abs(P[:, 0] + 1.5) - 0.8, np.abs(P[:, 2]) - 0.8), 0.0)
    d_sph = np.hypot(P[:, 0] - 1.5, P[:, 2])
    near_cube = floor & (d_cube > 0.0) & (d_cube < 0.8) & (P[:, 2] < 0.8)  # in front of it or beside it, not behind
    near_sph = floor & (d_sph < 1.6) & (P[:, 2] < 0.8)
    far = floor & (d_cube > 2.5) & (d_sph > 3.3)
    assert near_cube.sum() >= 3 and near_sph.sum() >= 3 and far.sum() >= 3, (near_cube.sum(), near_sph.sum(), far.sum())
    assert G[near_cube, 0].mean() > G[near_cube, 2].mean() + 0.01  # red bleeds onto the white floor
    assert G[far].mean() < G[near_sph].mean()
    assert G[far].mean() < G[near_cube, 0].mean()


def test_filtering_lowers_the_error_of_a_sparse_gather(R, renderer):
    """Usefulness: at 48 x 32 on the oracle scene, the squared error of a K = 4 plane against a K = 1024 plane over the
    hits, before and after rr_denoise with 3 levels guided by the first-hit planes."""
    import oracle

    b, _, view = oracle_scene(R, oracle)
    renderer.upload(b)
    cam = R.camera(48, 32, math.pi / 3, view)
    ref = renderer.render_indirect(cam, R.Indirect(1024, 1, seed=7))["indirect"]
    noisy = renderer.render_indirect(cam, R.Indirect(4, 1, seed=8))["indirect"]
    aov = renderer.render_aov(cam)
    clean = renderer.denoise(noisy, R.Denoise(3), depth=aov["depth"], normal=aov["normal"], object=aov["object"],
                             albedo=aov["albedo"])
    hit = aov["object"] >= 0
    before = float(((noisy - ref)[hit] ** 2).sum())
    after = float(((clean - ref)[hit] ** 2).sum())
    print(f"K = 4 against K = 1024 over {int(hit.sum())} hits: squared error {before:.4g} before, {after:.4g} after "
          f"denoise (3 levels): ratio {before / after:.3g}")
    assert same(clean[~hit], noisy[~hit]) and (noisy[~hit] == 0.0).all()
    assert after < before


# ---- 7. the entries ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_device_entries_on_a_torch_stream(R, renderer, dev):
    scene, cam_like = csg_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 16, 12, 1)[0]
    ind = R.Indirect(5, 1, seed=4)
    n = 192
    want, hit, stats = composed_frame(R, renderer, cam, ind, dev)
    rec = first_hits(R, renderer, cam, dev)
    o = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        P = torch.from_numpy(np.ascontiguousarray(rec["over_point"])).to(dev)
        N = torch.from_numpy(np.ascontiguousarray(rec["normalv"])).to(dev)
        pts = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        renderer.indirect_at_device(n, P.data_ptr(), N.data_ptr(), ind, pts.data_ptr(), stream=s.cuda_stream)
        img = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        renderer.render_indirect_device(cam, o, ind, img.data_ptr(), s.cuda_stream)
        brightest = img[:n].max()  # a consumer on the same stream
    s.synchronize()
    a = img.cpu().numpy()
    assert same(a[:n].reshape(12, 16, 3), want) and (a[n] == SENT).all()
    assert float(brightest) == float(want.max())
    p = pts.cpu().numpy()
    assert same(p[:n][hit], want.reshape(-1, 3)[hit]) and (p[n] == SENT).all()  # the same identities: i is the sample
    st = renderer.last_stats()  # the frame's, pending until asked for
    assert st["samples"] == n and {k: st[k] for k in COUNTERS} == stats and st["kernel_ms"] > 0


def test_indirect_leaves_frames_and_stats_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = V.yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = V.ring(R, scene.camera, 16, 16, 3)
            rec = first_hits(R, r, cams[0], dev)

            def work():
                r.render_indirect(cams[1], R.Indirect(3, 1, seed=1))
                frame_dev(R, r, cams[2], R.Indirect(16, 2), dev)
                points_dev(r, np.ascontiguousarray(rec["over_point"]), np.ascontiguousarray(rec["normalv"]), R.Indirect(5), dev)

            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            work()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            # a frame's stats are its own: rr_last_stats after the indirect frame is not the render's
            got = r.render_indirect(cams[1], R.Indirect(3, 1, seed=1))
            assert _without_time(r.last_stats()) == _without_time(got["stats"]) and got["stats"]["samples"] == 256
    finally:
        r.close()


@pytest.mark.parametrize("switch", ["RRAY_NO_TREE", "RRAY_UNFUSED", "RRAY_NO_CHAIN"])
def test_the_per_level_paths_refuse_frames_and_serve_points(R, renderer, dev, switch):
    scene, cam_like = {"RRAY_NO_TREE": glass_scene, "RRAY_UNFUSED": flat_scene, "RRAY_NO_CHAIN": chain_scene}[switch](R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 13, 5, 1)[0]
    ind = R.Indirect(3, 2, seed=1)
    rec = first_hits(R, renderer, cam, dev)
    rec = rec[rec["object"] >= 0]
    P, N = np.ascontiguousarray(rec["over_point"]), np.ascontiguousarray(rec["normalv"])
    want_frame = renderer.render_indirect(cam, ind)["indirect"]
    want = points_dev(renderer, P, N, ind, dev)
    with V.environment(**{switch: "1"}):
        with pytest.raises(R.RRError) as e:
            renderer.render_indirect(cam, ind)
        assert e.value.code == R._lib.RR_E_ARG and switch in str(e.value)
        img = torch.full((66, 3), SENT, dtype=torch.float64, device=dev)
        o = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
        with pytest.raises(R.RRError):
            renderer.render_indirect_device(cam, o, ind, img.data_ptr())
        Q.sync()
        assert (img.cpu().numpy() == SENT).all()  # refused before anything was enqueued
        got = points_dev(renderer, P, N, ind, dev)  # the point query has no list: the per-level kernels serve it
        assert np.abs(got - want).max() <= Q.TOL
    assert same(renderer.render_indirect(cam, ind)["indirect"], want_frame)


def test_refusals_and_the_empty_batch(R, renderer, dev):
    L, E = R.lib(), R._lib
    scene, cam_like = flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 8, 8, 1)[0]
    pts = torch.full((65, 3), 0.25, dtype=torch.float64, device=dev)
    nrm = torch.tensor([[0.0, 1.0, 0.0]] * 65, dtype=torch.float64, device=dev)
    img = torch.full((65, 3), SENT, dtype=torch.float64, device=dev)
    host = np.full((8, 8, 3), SENT)
    Q.sync()
    pp, pn, pi, ph = C.c_void_p(pts.data_ptr()), C.c_void_p(nrm.data_ptr()), C.c_void_p(img.data_ptr()), host.ctypes.data_as(E._D)
    h, pc = renderer.h, C.byref(cam)

    def err():
        return L.rr_last_error().decode()

    def opts(**kw):
        f = dict(aa=1, max_depth=0, seed=0, jitter_mode=0, part=0, nparts=1, block_rows=8, flags=0, row_begin=0, row_end=0)
        f.update(kw)
        return C.byref(E.RenderOpts(*f.values()))

    def ind(**kw):
        f = dict(samples=4, remaining=1, seed=0)
        f.update(kw)
        return C.byref(E.IndirectDesc(*f.values()))

    def frame(o=None, a=None, cam_=pc, ctx=h):
        """(device entry, host entry) return codes"""
        o, a = o or opts(), a or ind()
        return (L.rr_render_indirect_device(ctx, cam_, o, a, pi, None), L.rr_render_indirect(ctx, cam_, o, a, ph, None))

    def points(n=64, a=None, ctx=h, p=pp, nn=pn, out=pi):
        return L.rr_indirect_at_device(ctx, n, p, nn, a or ind(), 0, 0, out, None)

    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    # null pointers
    assert frame(ctx=None) == (ARG, ARG) and frame(cam_=None) == (ARG, ARG)
    assert L.rr_render_indirect_device(h, pc, None, ind(), pi, None) == ARG and L.rr_render_indirect(h, pc, None, ind(), ph, None) == ARG
    assert L.rr_render_indirect_device(h, pc, opts(), None, pi, None) == ARG and L.rr_render_indirect(h, pc, opts(), None, ph, None) == ARG
    assert L.rr_render_indirect_device(h, pc, opts(), ind(), None, None) == ARG and L.rr_render_indirect(h, pc, opts(), ind(), None, None) == ARG
    assert points(ctx=None) == ARG and points(p=None) == ARG and points(nn=None) == ARG and points(out=None) == ARG
    assert L.rr_indirect_at_device(h, 64, pp, pn, None, 0, 0, pi, None) == ARG
    assert points(n=-1) == ARG
    # the parameters
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=E.RR_MAX_INDIRECT_SAMPLES + 1)):
        assert frame(a=ind(**kw)) == (ARG, ARG), kw
        assert points(a=ind(**kw)) == ARG, kw
    for kw in (dict(remaining=-1), dict(remaining=Q.E_MAX_DEPTH + 1)):
        assert frame(a=ind(**kw)) == (LIM, LIM) and "remaining" in err(), kw
        assert points(a=ind(**kw)) == LIM, kw
    # the options: rr_render_ao's rules
    for kw in (dict(aa=0), dict(aa=3), dict(part=1, nparts=2), dict(nparts=2), dict(row_begin=0, row_end=4),
               dict(row_begin=2, row_end=4)):
        assert frame(o=opts(**kw)) == (ARG, ARG), kw
    big = E.Camera.from_buffer_copy(cam)
    for hs, vs in ((0, 8), (8, 0), (-1, 8)):
        big.hsize, big.vsize = hs, vs
        assert frame(cam_=C.byref(big)) == (ARG, ARG)
    # hsize * vsize * K >= 2^32, n * K >= 2^32
    big.hsize, big.vsize = 2**16, 2**14
    assert frame(cam_=C.byref(big), a=ind(samples=4)) == (LIM, LIM) and "2^32" in err()
    big.hsize, big.vsize = 2**16, 2**16
    assert frame(cam_=C.byref(big), a=ind(samples=1)) == (LIM, LIM)
    assert points(n=2**22, a=ind(samples=1024)) == LIM and "2^32" in err()
    assert points(n=2**32, a=ind(samples=1)) == LIM
    # the empty batch: RR_OK, nothing enqueued, null buffers allowed
    assert points(n=0) == 0 and L.rr_indirect_at_device(h, 0, None, None, ind(), 0, 0, None, None) == 0
    # no scene uploaded
    fresh = R.Renderer(0)
    try:
        assert frame(ctx=fresh.h) == (ARG, ARG) and "no scene" in err()
        assert points(ctx=fresh.h) == ARG and "no scene" in err()
    finally:
        fresh.close()
    # a virtual (multi-device) context
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert frame(ctx=v.h) == (ARG, ARG) and "single-device" in err()
        assert points(ctx=v.h) == ARG and "single-device" in err()
    finally:
        v.close()
    Q.sync()
    assert (img.cpu().numpy() == SENT).all() and (host == SENT).all()
    # and the calls still serve afterwards
    assert frame() == (0, 0)
    Q.sync()
    assert same(img[:64].cpu().numpy().reshape(8, 8, 3), host) and (img[64].cpu().numpy() == SENT).all()
    assert same(host, renderer.render_indirect(cam, R.Indirect(4, 1))["indirect"])
    # max_depth and flags are ignored
    keep = host.copy()
    assert frame(o=opts(max_depth=99, flags=E.RR_OUT_AVG)) == (0, 0) and same(host, keep)
    assert points() == 0
    Q.sync()
    a = img[:64].cpu().numpy()
    assert np.isfinite(a).all() and (a >= 0.0).all() and (img[64].cpu().numpy() == SENT).all()
