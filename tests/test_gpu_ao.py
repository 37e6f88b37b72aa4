"""Ambient occlusion on the GPU (rr_ao_at_device, rr_render_ao, rr_render_ao_device).  The definition
is exact: a point's value is ao_resolve of what rr_is_shadowed_device answers for its K (point, ao_targets) pairs, and a
frame's points are over_point / normalv of rr_hit_at_device over rr_camera_rays_device — so every comparison is
np.array_equal with no tolerance, and the counts against the oracle itself are equal integers.  Device buffers are torch
tensors with a sentinel behind every output, as in tests/test_gpu_rays.py, whose helpers these tests use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import test_gpu_lens as LN  # noqa: E402  its glass scene
import test_gpu_rays as Q  # noqa: E402  its helpers: same, sync, to_dev, camera_rays_dev, hit_dev, shadow_dev, SENT
import test_gpu_views_aov as V  # noqa: E402  its scenes, cameras, oracle records and environment switch

pytestmark = pytest.mark.gpu
SENT = Q.SENT
same = Q.same


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


def mesh_scene(R):
    """the teapot over its floor: groups and triangles (G = 1)"""
    s = V.yaml_scene(R, "c4_teapot.yaml", 16, 16)
    return s, s.camera


def lds_scene(R):
    """a fuzz scene small enough for culls staged in LDS (tests/test_gpu_views_aov.py VARIANTS)"""
    P, spec, _, _ = V.F.build(0)
    return P.b, V.F.cameras(P, spec, 16, 16)[0]


SCENES = {"flat": V.flat_scene, "chain": V.chain_scene, "csg": V.csg_scene, "glass": LN.glass_scene, "mesh": mesh_scene,
          "lds": lds_scene}


def ao_dev(r, P, N, ao, dev, stream=None):
    """rr_ao_at_device over host arrays, through tensors with sentinels: (n,) f64"""
    n = len(P)
    p, nn = Q.to_dev(P, dev), Q.to_dev(N, dev)
    out = torch.full((n + 1,), SENT, dtype=torch.float64, device=dev)
    Q.sync()
    r.ao_at_device(n, p.data_ptr(), nn.data_ptr(), ao, out.data_ptr(), stream)
    Q.sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "ao_at_device wrote past its points"
    return a[:n]


def composed(R, r, P, N, ao, dev, first=0):
    """the definition through the public entries: ao_targets in numpy, one is_shadowed_device over the n * K pairs,
    ao_resolve"""
    K, n = ao.samples, len(P)
    t = R.ao_targets(P, N, ao, first).reshape(n * K, 3)
    occ = Q.shadow_dev(r, Q.to_dev(np.repeat(P, K, axis=0), dev), Q.to_dev(t, dev), n * K, dev)
    return R.ao_resolve(occ, K)


def first_hits(R, r, cam, dev):
    """hit_at_device over camera_rays_device(cam): the records of the frame's samples"""
    n = cam.hsize * cam.vsize
    return Q.hit_dev(R, r, Q.camera_rays_dev(r, cam, dev), n, dev)


def composed_frame(R, r, cam, ao, dev):
    """a frame by the public entries: the composition at over_point / normalv of every sample that hit, 1.0 elsewhere;
    -> (plane (vsize, hsize), hits)"""
    rec = first_hits(R, r, cam, dev)
    miss = rec["object"] < 0
    P = np.where(miss[:, None], [0.0, 1e6, 0.0], rec["over_point"])  # a miss takes part in no walk: any free segment
    N = np.where(miss[:, None], [0.0, 1.0, 0.0], rec["normalv"])
    v = composed(R, r, np.ascontiguousarray(P), np.ascontiguousarray(N), ao, dev)
    v[miss] = 1.0
    return v.reshape(cam.vsize, cam.hsize), int((~miss).sum())


def frame_dev(R, r, cam, ao, dev, stream=None, aa=1):
    """rr_render_ao_device into a tensor with a sentinel: (vsize, hsize)"""
    n = cam.hsize * cam.vsize
    out = torch.full((n + 1,), SENT, dtype=torch.float64, device=dev)
    o = R._lib.RenderOpts(aa, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    Q.sync()
    r.render_ao_device(cam, o, ao, out.data_ptr(), stream)
    Q.sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "render_ao_device wrote past its plane"
    return a[:n].reshape(cam.vsize, cam.hsize)


# ---- 1. points against the public entries ----
@pytest.mark.parametrize("name", list(SCENES))
def test_points_equal_the_composition_of_the_public_entries(R, renderer, dev, name):
    scene, cam_like = SCENES[name](R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 20, 13, 2)[1]
    rec = first_hits(R, renderer, cam, dev)  # 260 records, misses (zeros) among them: every point is evaluated
    assert (rec["object"] >= 0).sum() >= 30, name
    for n in (1, 63, 65, 257):
        # from the frame's middle on, where most samples hit
        at = 0 if n == 257 else 130
        P, N = np.ascontiguousarray(rec["over_point"][at:at + n]), np.ascontiguousarray(rec["normalv"][at:at + n])
        for K in (1, 3, 16, 65):  # 64 % 3 and 64 % 65 != 0: a point's pairs straddle waves and count by atomics
            ao = R.Ao(K, 0.8, seed=n * 1000 + K)
            want = composed(R, renderer, P, N, ao, dev)
            got = ao_dev(renderer, P, N, ao, dev)
            assert same(got, want), (name, n, K)
            assert ((got >= 0.0) & (got <= 1.0)).all()
    if name not in ("flat", "chain", "csg", "glass"):
        return
    # objects resting on a floor: something is occluded (the creases) and something is open
    ao = R.Ao(16, 0.8, seed=1)
    hit = rec["object"] >= 0
    v = ao_dev(renderer, np.ascontiguousarray(rec["over_point"][hit]), np.ascontiguousarray(rec["normalv"][hit]), ao, dev)
    assert v.min() < 1.0 and v.max() == 1.0, name


# ---- 2. frames against the public entries ----
@pytest.mark.parametrize("W,H", [(7, 5), (13, 5), (16, 4), (65, 1)], ids=["7x5", "13x5", "16x4", "65x1"])
def test_frames_equal_the_composition_of_the_public_entries(R, renderer, dev, W, H):
    for name in ("flat", "csg", "mesh", "glass", "chain", "lds"):
        scene, cam_like = SCENES[name](R)
        renderer.upload(scene)
        cam = V.ring(R, cam_like, W, H, 2)[1]
        for K in (3, 16):
            ao = R.Ao(K, 0.7, seed=5 + K)
            want, hits = composed_frame(R, renderer, cam, ao, dev)
            got = renderer.render_ao(cam, ao)
            assert same(got["ao"], want), (name, W, H, K)
            st = got["stats"]
            assert st["samples"] == st["rays"] == W * H and st["shadow_rays"] == K * hits, (name, st)
            assert st["shade_events"] == 0 and st["nan_rays"] == 0 and st["kernel_ms"] > 0, (name, st)
            assert same(frame_dev(R, renderer, cam, ao, dev), want), (name, W, H, K)
    # never averaged: with aa = 2 the camera is the supersampled one and the plane has its size
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 2 * W, 2 * H, 1)[0]
    ao = R.Ao(4, 0.7, seed=2)
    got = renderer.render_ao(cam, ao, aa=2)["ao"]
    assert got.shape == (2 * H, 2 * W) and same(got, renderer.render_ao(cam, ao)["ao"])


# ---- 3. passes ----
@pytest.mark.parametrize("env", [dict(RRAY_AO_PASS="64"), dict(RRAY_AO_PASS="1"), dict(RRAY_BATCH="1024"),
                                 dict(RRAY_AO_PASS="4096", RRAY_BATCH="1024")],
                         ids=["pass64", "pass1_rounds_up", "batch1024", "pass4096_batch1024"])
def test_passes_equal_the_default_contexts_frame(R, renderer, dev, env):
    """41 x 30 = 1230 samples: under RRAY_AO_PASS=64 twenty passes, the last of 14 points; under RRAY_BATCH=1024 two
    passes of 1024 and 206 (the batch caps the pass, whatever RRAY_AO_PASS asks)."""
    with V.environment(**env):  # read when a context is created
        r = R.Renderer(0)
    try:
        for name in ("flat", "mesh", "csg"):
            scene, cam_like = SCENES[name](R)
            cam = V.ring(R, cam_like, 41, 30, 1)[0]
            renderer.upload(scene)
            r.upload(scene)
            for ao in (R.Ao(3, 0.7, seed=8), R.Ao(16, 0.7, seed=1)):
                want = renderer.render_ao(cam, ao)
                got = r.render_ao(cam, ao)
                assert same(got["ao"], want["ao"]), (env, name, ao)
                for k in ("rays", "shadow_rays", "shade_events", "samples", "nan_rays"):
                    assert got["stats"][k] == want["stats"][k], (env, name, k)
                assert same(frame_dev(R, r, cam, ao, dev), want["ao"])  # the sentinel behind the last pass
    finally:
        r.close()


def test_a_frame_in_which_half_the_samples_miss(R, renderer, dev):
    scene, _ = V.flat_scene(R)
    renderer.upload(scene)
    cam = R.camera(24, 16, math.pi / 3, V.translate(0, -0.5, 0))  # level with the horizon: sky above it
    ao = R.Ao(16, 0.7, seed=3)
    got = renderer.render_ao(cam, ao)
    obj = renderer.render_aov(cam, planes=("object",))["object"]
    miss = obj < 0
    assert 0.3 < miss.mean() < 0.7
    assert (got["ao"][miss] == 1.0).all() and got["ao"][~miss].min() < 1.0
    assert got["stats"]["shadow_rays"] == 16 * int((~miss).sum()) and got["stats"]["rays"] == 24 * 16
    want, hits = composed_frame(R, renderer, cam, ao, dev)
    assert hits == int((~miss).sum()) and same(got["ao"], want)


# ---- 4. the oracle itself ----
def ground_scene(R, oracle):
    """a floor, a sphere and a cube resting on it, on both sides"""
    mat = (0.1, 0.9, 0.0, 200.0, 0.0, 0.0, 1.0)
    sph, cub = V.scale_at(1.0, -1.2, 1.0, 0.0), V.scale_at(0.7, 1.3, 0.7, 0.4)
    b = R.SceneBuilder()
    b.point_light((-5, 6, -4), (1, 1, 1))
    b.plane(material=mat)
    b.sphere(transform=sph, material=mat)
    b.cube(transform=cub, material=mat)
    o = oracle.Oracle()
    o.point_light((-5, 6, -4), (1, 1, 1))
    o.add("plane", material=mat)
    o.add("sphere", transform=sph, material=mat)
    o.add("cube", transform=cub, material=mat)
    view = oracle.Oracle.mat.view_transform((0.3, 2.5, -6.0), (0.0, 0.7, 0.0), (0.0, 1.0, 0.0))
    return b, o, view


def test_a_frame_against_the_oracle_pair_by_pair(R, renderer):
    """24 x 16, K = 16, radius 1: P and N from the oracle's prepare_computations, every pair from the oracle's
    is_shadowed.  The counts must be equal.  A pair may be set aside only if the oracle's own intersection list for its
    segment has a t within 1e-9 * distance of 0 or of distance; none is (asserted)."""
    import oracle

    b, o, view = ground_scene(R, oracle)
    renderer.upload(b)
    W, H, K = 24, 16, 16
    cam = R.camera(W, H, math.pi / 3, view)
    ao = R.Ao(K, 1.0, seed=2026)
    got = renderer.render_ao(cam, ao)
    ocam = oracle.Oracle.camera(W, H, cam.field_of_view, list(cam.transform))
    rec = V.oracle_hits(R, o, V.camera_rays(oracle, ocam))
    hit = rec["object"] >= 0
    assert 200 < hit.sum() < W * H  # some sky
    T = R.ao_targets(rec["over_point"], np.where(hit[:, None], rec["normalv"], [0.0, 1.0, 0.0]), ao)
    want = np.zeros(W * H, np.int64)
    set_aside, nearest = 0, math.inf
    for i in np.flatnonzero(hit):
        p = rec["over_point"][i]
        for k in range(K):
            t = T[i, k]
            want[i] += int(o.is_shadowed(p.tolist() + [1.0], t.tolist() + [1.0]))
            v = t - p
            dist = math.sqrt(float(v @ v))
            for x in o.intersect(p.tolist() + [1.0], (v / dist).tolist() + [0.0], cap=64):
                edge = min(abs(x[0]), abs(x[0] - dist)) / dist
                nearest = min(nearest, edge)
                set_aside += edge <= 1e-9
    counts = np.rint((1.0 - got["ao"].reshape(-1)) * K).astype(np.int64)
    assert same((K - counts).astype(np.float64) / float(K), got["ao"].reshape(-1))  # the values are (K - c) / K exactly
    exact = float(np.mean(counts == want))
    print(f"AO frame against the oracle: {int(hit.sum())} hits, {int(hit.sum()) * K} pairs, {int(want.sum())} occluded, "
          f"set aside {set_aside}, nearest intersection to a segment's end {nearest:.3g} (relative), bit-exact share {exact:.6f}")
    assert set_aside == 0
    assert np.array_equal(counts, want)
    assert got["stats"]["shadow_rays"] == K * int(hit.sum())
    # the picture: the sky is open, the creases under the sphere and along the cube darken the floor
    plane = got["ao"]
    assert (plane[~hit.reshape(H, W)] == 1.0).all() and plane.min() <= 0.5 and np.median(plane) >= 0.75


# ---- 5. further cases ----
def test_a_lone_sphere_is_open_everywhere(R, renderer):
    b = R.SceneBuilder()
    b.point_light((-5, 6, -4), (1, 1, 1))
    b.sphere(transform=V.scale_at(1.5, 0, 0, 0))
    renderer.upload(b)
    got = renderer.render_ao(R.camera(20, 15, math.pi / 3, V.translate(0, 0, -5)), R.Ao(64, 3.0, seed=1))
    assert got["stats"]["shadow_rays"] > 64 * 40 and (got["ao"] == 1.0).all()


def test_a_short_radius_on_the_open_plane_is_open(R, renderer, dev):
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 20, 15, 1)[0]
    obj = renderer.render_aov(cam, planes=("object",))["object"]
    floor = obj == np.bincount(obj[obj >= 0]).argmax()  # the object most samples hit
    assert floor.sum() > 50
    short = renderer.render_ao(cam, R.Ao(16, 1e-3, seed=4))["ao"]
    # 1e-3 is a hundred times over_point's offset and far less than any gap between the floor's samples and a sphere
    assert (short[floor] == 1.0).all()
    assert renderer.render_ao(cam, R.Ao(16, 2.0, seed=4))["ao"][floor].min() < 1.0  # a long one reaches the spheres


def test_a_point_inside_a_closed_cube_is_closed(R, renderer, dev):
    b = R.SceneBuilder()
    b.point_light((-5, 6, -4), (1, 1, 1))
    b.cube(transform=V.translate(3, 0, 0))
    renderer.upload(b)
    rng = np.random.default_rng(3)
    P = np.array([3.0, 0.0, 0.0]) + rng.uniform(-0.9, 0.9, size=(65, 3))
    N = rng.normal(size=(65, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    assert (ao_dev(renderer, P, N, R.Ao(16, 4.0, seed=6), dev) == 0.0).all()  # 4 > the cube's diagonal
    assert (ao_dev(renderer, P, N, R.Ao(16, 0.05, seed=6), dev) == 1.0).all()  # and a segment that stays inside is free
    out = P + np.array([10.0, 0.0, 0.0])
    assert (ao_dev(renderer, out, np.tile([1.0, 0.0, 0.0], (65, 1)), R.Ao(16, 4.0, seed=6), dev) == 1.0).all()


# ---- 6. the entries ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_device_entries_on_a_torch_stream(R, renderer, dev):
    scene, cam_like = V.csg_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 16, 12, 1)[0]
    ao = R.Ao(5, 0.7, seed=4)
    n = 192
    want, hits = composed_frame(R, renderer, cam, ao, dev)
    rec = first_hits(R, renderer, cam, dev)
    o = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        img = torch.full((n + 1,), SENT, dtype=torch.float64, device=dev)
        renderer.render_ao_device(cam, o, ao, img.data_ptr(), s.cuda_stream)
        darkest = img[:n].min()
        # the same values from the points of the same stream's records
        P = torch.from_numpy(np.ascontiguousarray(rec["over_point"])).to(dev)
        N = torch.from_numpy(np.ascontiguousarray(rec["normalv"])).to(dev)
        pts = torch.full((n + 1,), SENT, dtype=torch.float64, device=dev)
        renderer.ao_at_device(n, P.data_ptr(), N.data_ptr(), ao, pts.data_ptr(), s.cuda_stream)
    s.synchronize()
    a = img.cpu().numpy()
    assert same(a[:n].reshape(12, 16), want) and a[n] == SENT
    assert float(darkest) == float(want.min())
    b = pts.cpu().numpy()
    hit = rec["object"] >= 0
    assert same(b[:n][hit], want.reshape(-1)[hit]) and b[n] == SENT
    # the frame's stats are pending until asked for; the point query left them alone
    st = renderer.last_stats()
    assert st["samples"] == st["rays"] == n and st["shadow_rays"] == 5 * hits and st["shade_events"] == 0
    assert st["kernel_ms"] > 0


def test_ao_leaves_frames_and_stats_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = V.yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = V.ring(R, scene.camera, 16, 16, 3)
            rec = first_hits(R, r, cams[0], dev)

            def ao_work():
                r.render_ao(cams[1], R.Ao(3, 0.5, seed=1))
                frame_dev(R, r, cams[2], R.Ao(16, 0.5), dev)
                ao_dev(r, np.ascontiguousarray(rec["over_point"]), np.ascontiguousarray(rec["normalv"]), R.Ao(5, 0.5), dev)

            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            ao_work()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            # the point query leaves the last stats as they are
            st = r.last_stats()
            ao_dev(r, np.ascontiguousarray(rec["over_point"]), np.ascontiguousarray(rec["normalv"]), R.Ao(5, 0.5), dev)
            assert r.last_stats() == st, src
    finally:
        r.close()


def test_refusals_and_the_empty_batch(R, renderer, dev):
    L, E = R.lib(), R._lib
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 8, 8, 1)[0]
    pts = torch.full((65, 3), 0.25, dtype=torch.float64, device=dev)
    img = torch.full((65,), SENT, dtype=torch.float64, device=dev)
    host = np.full((8, 8), SENT)
    Q.sync()
    pp, pi, ph = C.c_void_p(pts.data_ptr()), C.c_void_p(img.data_ptr()), host.ctypes.data_as(E._D)
    h, pc = renderer.h, C.byref(cam)

    def err():
        return L.rr_last_error().decode()

    def opts(**kw):
        f = dict(aa=1, max_depth=0, seed=0, jitter_mode=0, part=0, nparts=1, block_rows=8, flags=0, row_begin=0, row_end=0)
        f.update(kw)
        return C.byref(E.RenderOpts(*f.values()))

    def ao(**kw):
        f = dict(samples=4, reserved=0, radius=1.0, seed=0)
        f.update(kw)
        return C.byref(E.AoDesc(*f.values()))

    def frame(o=None, a=None, cam_=pc, ctx=h):
        """(device entry, host entry) return codes"""
        o, a = o or opts(), a or ao()
        return (L.rr_render_ao_device(ctx, cam_, o, a, pi, None), L.rr_render_ao(ctx, cam_, o, a, ph, None))

    def points(n=64, a=None, ctx=h, p=pp, nn=pp, out=pi):
        return L.rr_ao_at_device(ctx, n, p, nn, a or ao(), out, None)

    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    # null pointers
    assert frame(ctx=None) == (ARG, ARG) and frame(cam_=None) == (ARG, ARG)
    assert L.rr_render_ao_device(h, pc, None, ao(), pi, None) == ARG and L.rr_render_ao(h, pc, None, ao(), ph, None) == ARG
    assert L.rr_render_ao_device(h, pc, opts(), None, pi, None) == ARG and L.rr_render_ao(h, pc, opts(), None, ph, None) == ARG
    assert L.rr_render_ao_device(h, pc, opts(), ao(), None, None) == ARG and L.rr_render_ao(h, pc, opts(), ao(), None, None) == ARG
    assert points(ctx=None) == ARG and points(p=None) == ARG and points(nn=None) == ARG and points(out=None) == ARG
    assert L.rr_ao_at_device(h, 64, pp, pp, None, pi, None) == ARG
    assert points(n=-1) == ARG
    # the parameters
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=E.RR_MAX_AO_SAMPLES + 1), dict(reserved=1),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=math.nan), dict(radius=math.inf)):
        assert frame(a=ao(**kw)) == (ARG, ARG), kw
        assert points(a=ao(**kw)) == ARG, kw
    # the options: rr_render_aov's rules
    for kw in (dict(aa=0), dict(aa=3), dict(part=1, nparts=2), dict(nparts=2), dict(row_begin=0, row_end=4),
               dict(row_begin=2, row_end=4)):
        assert frame(o=opts(**kw)) == (ARG, ARG), kw
    big = E.Camera.from_buffer_copy(cam)
    for hs, vs in ((0, 8), (8, 0), (-1, 8)):
        big.hsize, big.vsize = hs, vs
        assert frame(cam_=C.byref(big)) == (ARG, ARG)
    big.hsize, big.vsize = 2**16, 2**15
    assert L.rr_render_ao_device(h, C.byref(big), opts(), ao(), pi, None) == LIM and "2^31" in err()
    # n * K >= 2^32
    assert points(n=2**22, a=ao(samples=1024)) == LIM and "2^32" in err()
    assert points(n=2**32, a=ao(samples=1)) == LIM
    # the empty batch: RR_OK, nothing enqueued, null buffers allowed
    assert points(n=0) == 0 and L.rr_ao_at_device(h, 0, None, None, ao(), None, None) == 0
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
    assert same(img[:64].cpu().numpy().reshape(8, 8), host) and img[64].item() == SENT
    assert same(host, renderer.render_ao(cam, R.Ao(4, 1.0))["ao"])
    # max_depth, seed, jitter_mode and flags are ignored, as by rr_render_aov
    keep = host.copy()
    assert frame(o=opts(max_depth=99, seed=5, jitter_mode=1, flags=E.RR_OUT_AVG)) == (0, 0) and same(host, keep)
    assert points() == 0
    Q.sync()
    assert ((img[:64].cpu().numpy() >= 0.0) & (img[:64].cpu().numpy() <= 1.0)).all() and img[64].item() == SENT
