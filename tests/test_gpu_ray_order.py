"""Ordered ray batches on the GPU (rr_ray_order_device, rr_color_at_device_ordered, rr_hit_at_device_ordered;
DESIGN.md §3.19).  The definitions are exact: the order is argsort(rray_amd.ray_order_keys(rays), kind="stable"), and an
ordered query writes what the plain device entry writes for the same batch, bit for bit, whatever permutation it walks
— so every comparison is np.array_equal (NaN equal to NaN) with no tolerance.  Every output is allocated one row longer
than needed and prefilled with a sentinel, and the tail must come back untouched (tests/test_gpu_rays.py's helpers)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import scene_fuzz as F  # noqa: E402
import test_gpu_rays as G  # noqa: E402  its helpers and FAMILIES
import test_gpu_views_aov as V  # noqa: E402  its scenes and cameras

pytestmark = pytest.mark.gpu
SENT = G.SENT
COUNTS = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples", "nan_rays")
same, sync, records_equal = G.same, G.sync, G.records_equal


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


def perm_tensor(perm, dev):
    """a host permutation as a device tensor (uint32 bits in int32) with one sentinel entry behind it"""
    a = np.concatenate([np.asarray(perm, np.uint32), np.array([0xFFFFFFF9], np.uint32)])
    return torch.from_numpy(a.view(np.int32).copy()).to(dev)


def order_dev(r, rays, n, dev, stream=None):
    out = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    sync()
    r.ray_order_device(n, rays.data_ptr(), out.data_ptr(), stream)
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == -7).all(), "ray_order_device wrote past its entries"
    return a[:n].view(np.uint32)


def color_ord(r, rays, n, dev, perm=None, **kw):
    out = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
    p = None if perm is None else perm_tensor(perm, dev)
    sync()
    r.color_at_device_ordered(n, rays.data_ptr(), out.data_ptr(), None if p is None else p.data_ptr(), **kw)
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "color_at_device_ordered wrote past its rays"
    return a[:n]


def hit_ord(R, r, rays, n, dev, perm=None):
    out = torch.full((n + 1, 192), 0xA5, dtype=torch.uint8, device=dev)
    p = None if perm is None else perm_tensor(perm, dev)
    sync()
    r.hit_at_device_ordered(n, rays.data_ptr(), out.data_ptr(), None if p is None else p.data_ptr())
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == 0xA5).all(), "hit_at_device_ordered wrote past its records"
    return np.ascontiguousarray(a[:n]).reshape(-1).view(R._lib.hit_dtype())


def want_order(R, rays_host):
    return np.argsort(R.ray_order_keys(rays_host), kind="stable").astype(np.uint32)


def check_order(R, r, host, dev, what):
    n = len(host)
    got = order_dev(r, G.to_dev(host, dev), n, dev)
    want = want_order(R, host)
    if not same(got, want):
        bad = np.flatnonzero(got != want)
        print(f"{what}: {len(bad)} of {n} entries differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}")
    assert same(got, want), what
    return got


# ---- 1. the order itself (no scene uploaded) ----
@pytest.fixture(scope="module")
def cam_rays(R, dev):
    """the rays of a 20 x 15 and of a 150 x 140 camera, on the host"""
    r = R.Renderer(0)
    try:
        _, cam_like = V.chain_scene(R)
        small = G.camera_rays_dev(r, V.ring(R, cam_like, 20, 15, 1)[0], dev)[:300].cpu().numpy()
        large = G.camera_rays_dev(r, V.ring(R, cam_like, 150, 140, 1)[0], dev)[:21000].cpu().numpy()
    finally:
        r.close()
    return small, large


@pytest.fixture(scope="module")
def bare(R):
    r = R.Renderer(0)  # no scene: the order needs none
    yield r
    r.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_the_order_of_camera_prefixes(R, bare, dev, cam_rays, n):
    check_order(R, bare, cam_rays[0][:n], dev, f"n {n}")


def test_the_order_over_many_blocks_and_twice(R, bare, dev, cam_rays):
    large = cam_rays[1]
    first = check_order(R, bare, large, dev, "150 x 140")
    assert same(check_order(R, bare, large, dev, "150 x 140 again"), first)  # two calls, one answer
    # the batch twice: every key occurs at i and at 21000 + i, in different blocks; stable means i comes first
    twice = check_order(R, bare, np.concatenate([large, large]), dev, "twice")
    pos = np.empty(42000, np.int64)
    pos[twice] = np.arange(42000)
    assert (pos[:21000] < pos[21000:]).all()


def test_the_order_of_random_rays_in_every_digit(R, bare, dev):
    n = 2**20 + 17
    rng = np.random.default_rng(20261021)
    host = np.concatenate([rng.uniform(-50.0, 50.0, (n, 3)), rng.normal(size=(n, 3))], axis=1)
    keys = R.ray_order_keys(host)
    for shift in (0, 8, 16, 24):  # every digit of every pass is in use
        assert len(np.unique((keys >> np.uint32(shift)) & np.uint32(255))) == 256, shift
    check_order(R, bare, host, dev, "random")


def test_the_order_with_invalid_rays(R, bare, dev, cam_rays):
    host = cam_rays[0].copy()
    host[::7, 4] = np.nan
    host[3::11, 1] = np.inf
    host[5::13, 0] = -np.inf
    host[2::17, 3:] = 0.0  # no direction
    host[9::19, 3:] = -0.0
    keys = R.ray_order_keys(host)
    n_bad = int((keys == 0xFFFFFFFF).sum())
    assert 80 < n_bad < 200
    got = check_order(R, bare, host, dev, "mixed")
    assert sorted(got[300 - n_bad:]) == sorted(np.flatnonzero(keys == 0xFFFFFFFF))  # they sort to the end
    host[:] = np.nan
    assert same(check_order(R, bare, host, dev, "all invalid"), np.arange(300, dtype=np.uint32))
    host[:] = 0.0
    assert same(check_order(R, bare, host[:65], dev, "all zero"), np.arange(65, dtype=np.uint32))


# ---- 2. any permutation gives the plain answer ----
@pytest.fixture(scope="module")
def chain300(R, dev):
    """chain_scene and the 300 rays of a 20 x 15 camera with the plain device entries' answers (computed once)"""
    r = R.Renderer(0)
    try:
        scene, cam_like = V.chain_scene(R)
        r.upload(scene)
        rays = G.camera_rays_dev(r, V.ring(R, cam_like, 20, 15, 1)[0], dev)
        ref = {"scene": scene, "rays": rays}
        for n in (1, 63, 64, 65, 257, 300):
            ref[n] = (G.color_dev(r, rays, n, dev), G.hit_dev(R, r, rays, n, dev))
    finally:
        r.close()
    assert (ref[300][1]["object"] >= 0).any() and (ref[300][1]["object"] < 0).any()
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300])
def test_any_permutation_gives_the_plain_answer(R, renderer, dev, chain300, n):
    renderer.upload(chain300["scene"])
    rays = chain300["rays"]
    want_c, want_h = chain300[n]
    own = order_dev(renderer, rays, n, dev)
    assert sorted(own) == list(range(n))
    perms = {"identity": np.arange(n), "reverse": np.arange(n)[::-1], "random": np.random.default_rng(5).permutation(n),
             "own": own, "none": None}
    for name, p in perms.items():
        assert same(color_ord(renderer, rays, n, dev, p), want_c), (n, name)
        records_equal(R, hit_ord(R, renderer, rays, n, dev, p), want_h, f"n {n} {name}")


# ---- 3. every kernel family ----
@pytest.mark.parametrize("name,src", G.FAMILIES, ids=[v[0] for v in G.FAMILIES])
def test_every_kernel_family(R, renderer, dev, name, src):
    """The 143 rays of a camera, shuffled in HBM: the ordered queries equal the plain ones on the shuffled buffer, and,
    un-shuffled, the canvas of render(cam).  The area-light row proves that the jitter identity of a ray is its own
    index in the batch (sample perm[t]), not the slot that works on it."""
    kw = {}
    if src is None:
        scene, cam_like = V.csg_scene(R)
    elif src == "chain":
        scene, cam_like = V.chain_scene(R)
    elif isinstance(src, tuple):
        P, spec, _, _ = F.build(src[1])
        scene, cam_like = P.b, F.cameras(P, spec, 16, 16)[0]
    else:
        scene = V.yaml_scene(R, src, 16, 16, 1, G.GOLDEN if src == "perturbed_pattern.yaml" else G.SCENES)
        cam_like = scene.camera
    if name == "c5_area_light":
        kw = {"seed": 12345, "jitter_mode": 0}
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 13, 11, 2)[1]
    n = 143
    straight = G.camera_rays_dev(renderer, cam, dev)[:n].cpu().numpy()
    shuffle = np.random.default_rng(143).permutation(n)
    rays = G.to_dev(straight[shuffle], dev)
    got_c, got_h = color_ord(renderer, rays, n, dev, **kw), hit_ord(R, renderer, rays, n, dev)
    assert same(got_c, G.color_dev(renderer, rays, n, dev, **kw)), name
    records_equal(R, got_h, G.hit_dev(R, renderer, rays, n, dev), name)
    # un-shuffled: ray shuffle[j] of the camera sits at j.  Its jitter identity there is sample j, so the frame's canvas
    # is matched by the batch in camera order, walked in the library's order
    rays = G.to_dev(straight, dev)
    frame = renderer.render(cam, canvas=True, **kw)["canvas"].reshape(n, 3)
    got = color_ord(renderer, rays, n, dev, **kw)
    print(f"{name}: ordered colours differing from the canvas {int((got != frame).any(axis=1).sum())} of {n}")
    assert same(got, frame), name
    if name != "c5_area_light":  # without jitter a ray's colour does not depend on its place in the batch
        assert same(got_c, frame[shuffle]), name


# ---- 4. passes ----
def test_passes_under_a_small_batch(R, renderer, dev):
    scene, cam_like = V.chain_scene(R)
    cam = V.ring(R, cam_like, 50, 50, 1)[0]
    n = 2500
    renderer.upload(scene)
    straight = G.camera_rays_dev(renderer, cam, dev)[:n].cpu().numpy()
    rays = G.to_dev(straight[np.random.default_rng(2500).permutation(n)], dev)
    want_c, want_h = color_ord(renderer, rays, n, dev), hit_ord(R, renderer, rays, n, dev)
    records_equal(R, want_h, G.hit_dev(R, renderer, rays, n, dev), "default context")
    # the colours are held to the default context's ordered ones, not to the plain entry's: of these 2500 shuffled rays
    # one (row 235) differs from the plain call by 2 ulps in one channel, and the plain entry gives that ray this other
    # value too when it runs alone or in camera order: pow_shininess takes the library pow for lanes whose shininess
    # is not their wave's first lane's, so a specular term depends on the wave's composition
    diff = int((want_c != G.color_dev(renderer, rays, n, dev)).any(axis=1).sum())
    print(f"ordered colours differing from the plain entry's on the shuffled buffer: {diff} of {n}")
    with V.environment(RRAY_BATCH="1024"):  # read when a context is created: three passes (1024, 1024, 452)
        r = R.Renderer(0)
    try:
        r.upload(scene)
        assert same(color_ord(r, rays, n, dev), want_c)
        records_equal(R, hit_ord(R, r, rays, n, dev), want_h, "batch 1024")
        assert r.last_stats()["samples"] == n
        rev = np.arange(n)[::-1]
        records_equal(R, hit_ord(R, r, rays, n, dev, rev), want_h, "batch 1024, reversed")
    finally:
        r.close()


# ---- 5. coherence, by counter ----
def test_the_order_lowers_the_wave_visits(R, dev):
    r = R.Renderer(0)
    try:
        scene = V.yaml_scene(R, "c2_s1024.yaml", 64, 64)
        r.upload(scene)
        n = 4096
        straight = G.camera_rays_dev(r, scene.camera, dev)[:n].cpu().numpy()
        rays = G.to_dev(straight[np.random.default_rng(4096).permutation(n)], dev)
        for what, plain, ordered in (("hit", lambda: G.hit_dev(R, r, rays, n, dev), lambda: hit_ord(R, r, rays, n, dev)),
                                     ("colour", lambda: G.color_dev(r, rays, n, dev, remaining=5),
                                      lambda: color_ord(r, rays, n, dev, remaining=5))):
            a = plain()
            sp = r.last_stats()
            b = ordered()
            so = r.last_stats()
            if what == "colour":
                assert same(a, b)
            else:
                records_equal(R, b, a, what)
            print(f"{what}: wave_visits[0] plain {sp['wave_visits'][0]} ordered {so['wave_visits'][0]} "
                  f"ratio {sp['wave_visits'][0] / max(1, so['wave_visits'][0]):.2f}; prim_tests plain {sp['prim_tests']} "
                  f"ordered {so['prim_tests']}")
            assert so["wave_visits"][0] < sp["wave_visits"][0], what
            for k in COUNTS:
                assert so[k] == sp[k], (what, k)
    finally:
        r.close()


# ---- 6. a torch stream, no synchronisation before the end ----
def test_ordered_queries_on_a_torch_stream(R, renderer, dev):
    scene, cam_like = V.chain_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 16, 16, 1)[0]
    n = 256
    sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        rays = torch.full((n + 1, 6), SENT, dtype=torch.float64, device=dev)
        perm = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
        rgb = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        rgb2 = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        hits = torch.full((n + 1, 192), 0xA5, dtype=torch.uint8, device=dev)
        renderer.camera_rays_device(cam, rays.data_ptr(), s.cuda_stream)
        rays[:n] = rays[:n].flip(0)  # on the stream, between the calls
        rays[:n, :3] += torch.tensor([0.25, 0.125, -0.5], dtype=torch.float64, device=dev)
        renderer.ray_order_device(n, rays.data_ptr(), perm.data_ptr(), s.cuda_stream)
        first = perm[:n].clone()
        renderer.color_at_device_ordered(n, rays.data_ptr(), rgb.data_ptr(), perm.data_ptr(), stream=s.cuda_stream)
        brightest = rgb[:n].max()
        renderer.hit_at_device_ordered(n, rays.data_ptr(), hits.data_ptr(), stream=s.cuda_stream)  # the library's order
        n_hits = (hits.view(torch.int32)[:n, 0] >= 0).sum()
        renderer.color_at_device_ordered(n, rays.data_ptr(), rgb2.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    host = rays[:n].cpu().numpy()
    assert same(first.cpu().numpy().view(np.uint32), want_order(R, host)) and int(perm[n]) == -7
    o, d = np.ascontiguousarray(host[:, :3]), np.ascontiguousarray(host[:, 3:])
    want_c, want_h = renderer.color_at(o, d), renderer.hit_at(o, d)
    assert same(rgb[:n].cpu().numpy(), want_c) and (rgb[n:].cpu().numpy() == SENT).all()
    assert same(rgb2[:n].cpu().numpy(), want_c) and (rgb2[n:].cpu().numpy() == SENT).all()
    a = hits.cpu().numpy()
    assert (a[n:] == 0xA5).all()
    records_equal(R, np.ascontiguousarray(a[:n]).reshape(-1).view(R._lib.hit_dtype()), want_h, "stream")
    assert float(brightest) == float(want_c.max())
    assert int(n_hits) == int((want_h["object"] >= 0).sum()) > 0


# ---- 7. isolation ----
def test_ordered_queries_leave_frames_and_batches_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = V.yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = V.ring(R, scene.camera, 16, 16, 3)

            def queries():
                rays = G.camera_rays_dev(r, cams[1], dev)
                p = order_dev(r, rays, 256, dev)
                color_ord(r, rays, 256, dev, p)
                hit_ord(R, r, rays, 256, dev)

            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            queries()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert G._without_time(before["stats"]) == G._without_time(after["stats"]), src
            before = r.render_views(cams, max_depth=5)
            queries()
            after = r.render_views(cams, max_depth=5)
            assert same(before["avg"], after["avg"]), src
            assert G._without_time(before["stats"]) == G._without_time(after["stats"]), src
    finally:
        r.close()


# ---- 8. stats, NaN rays, refusals, n == 0 ----
def test_stats_after_the_ordered_queries(R, renderer, dev, chain300):
    renderer.upload(chain300["scene"])
    n, rays = 300, chain300["rays"]
    want = chain300[300][1]
    G.hit_dev(R, renderer, rays, n, dev)
    plain = renderer.last_stats()
    hit_ord(R, renderer, rays, n, dev)
    scratch = perm_tensor(np.zeros(n), dev)
    renderer.ray_order_device(n, rays.data_ptr(), scratch.data_ptr())  # leaves the stats alone
    sync()
    st = renderer.last_stats()
    assert st["rays"] == st["samples"] == n and st["n1n2_scans"] == int((want["object"] >= 0).sum()) > 0
    assert st["shadow_rays"] == st["shade_events"] == 0 and st["nan_rays"] == 0 and st["kernel_ms"] > 0
    for k in COUNTS:
        assert st[k] == plain[k], k
    G.color_dev(renderer, rays, n, dev)
    plain = renderer.last_stats()
    color_ord(renderer, rays, n, dev)
    st = renderer.last_stats()
    assert st["samples"] == n and st["kernel_ms"] > 0
    for k in COUNTS:
        assert st[k] == plain[k], k


def test_nan_rays_are_counted_and_the_ordered_entries_return_ok(R, renderer, dev):
    """the NaN scene of tests/test_gpu_rays.py: every ray of a NaN camera meets two NaN entries"""
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    b.plane()
    b.plane(transform=(1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 1))
    renderer.upload(b)
    sound = R.camera(8, 8, 1.0, V.translate(0, -0.5, 0))
    nan_cam = R.camera(8, 8, 1.0, tuple([math.nan] * 12 + [0.0, 0.0, 0.0, 1.0]))
    rays = torch.cat([G.camera_rays_dev(renderer, nan_cam, dev)[:64], G.camera_rays_dev(renderer, sound, dev)])
    n = 128
    want_h = G.hit_dev(R, renderer, rays, n, dev)
    nan_h = renderer.last_stats()["nan_rays"]
    want_c = G.color_dev(renderer, rays, n, dev)
    nan_c = renderer.last_stats()["nan_rays"]
    assert nan_h == 64 and nan_c >= 64
    own = order_dev(renderer, rays, n, dev)
    assert sorted(own[64:]) == list(range(64))  # the NaN rays sort to the end
    records_equal(R, hit_ord(R, renderer, rays, n, dev), want_h, "nan rays")  # RR_OK (the mirror raises otherwise)
    assert renderer.last_stats()["nan_rays"] == nan_h
    assert same(color_ord(renderer, rays, n, dev), want_c)
    assert renderer.last_stats()["nan_rays"] == nan_c


def test_refusals_and_the_empty_batch(R, renderer, dev):
    L, E = R.lib(), R._lib
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 8, 8, 1)[0]
    rays = G.camera_rays_dev(renderer, cam, dev)
    rgb = torch.full((65, 3), SENT, dtype=torch.float64, device=dev)
    hits = torch.full((65, 192), 0xA5, dtype=torch.uint8, device=dev)
    perm = torch.full((65,), -7, dtype=torch.int32, device=dev)
    sync()
    pr, pc, ph, pp = (C.c_void_p(t.data_ptr()) for t in (rays, rgb, hits, perm))
    h = renderer.h

    def err():
        return L.rr_last_error().decode()

    def untouched():
        sync()
        return bool((rgb.cpu().numpy() == SENT).all() and (hits.cpu().numpy() == 0xA5).all() and
                    (perm.cpu().numpy() == -7).all())

    for rem in (-1, G.E_MAX_DEPTH + 1):
        assert L.rr_color_at_device_ordered(h, 64, pr, None, rem, 0, 0, pc, None) == E.RR_E_LIMIT and "remaining" in err()
    assert L.rr_ray_order_device(h, 64, None, pp, None) == E.RR_E_ARG and "null" in err()
    assert L.rr_ray_order_device(h, 64, pr, None, None) == E.RR_E_ARG
    assert L.rr_color_at_device_ordered(h, 64, None, None, 5, 0, 0, pc, None) == E.RR_E_ARG and "null" in err()
    assert L.rr_color_at_device_ordered(h, 64, pr, None, 5, 0, 0, None, None) == E.RR_E_ARG
    assert L.rr_hit_at_device_ordered(h, 64, None, None, ph, None) == E.RR_E_ARG
    assert L.rr_hit_at_device_ordered(h, 64, pr, None, None, None) == E.RR_E_ARG
    assert L.rr_ray_order_device(h, -1, pr, pp, None) == E.RR_E_ARG and "negative" in err()
    assert L.rr_color_at_device_ordered(h, -1, pr, pp, 5, 0, 0, pc, None) == E.RR_E_ARG and "negative" in err()
    assert L.rr_hit_at_device_ordered(h, -1, pr, pp, ph, None) == E.RR_E_ARG
    assert L.rr_ray_order_device(h, 2**32, pr, pp, None) == E.RR_E_LIMIT and "2^32" in err()
    assert L.rr_color_at_device_ordered(h, 2**32, pr, pp, 5, 0, 0, pc, None) == E.RR_E_LIMIT and "2^32" in err()
    assert L.rr_hit_at_device_ordered(h, 2**32, pr, pp, ph, None) == E.RR_E_LIMIT
    # n == 0: RR_OK, nothing enqueued, null buffers allowed
    assert L.rr_ray_order_device(h, 0, pr, pp, None) == 0 and L.rr_ray_order_device(h, 0, None, None, None) == 0
    assert L.rr_color_at_device_ordered(h, 0, pr, pp, 5, 0, 0, pc, None) == 0
    assert L.rr_color_at_device_ordered(h, 0, None, None, 5, 0, 0, None, None) == 0
    assert L.rr_hit_at_device_ordered(h, 0, pr, pp, ph, None) == 0
    assert L.rr_hit_at_device_ordered(h, 0, None, None, None, None) == 0
    assert untouched()
    # no scene uploaded: the queries are refused, the order is not
    fresh = R.Renderer(0)
    try:
        assert L.rr_color_at_device_ordered(fresh.h, 64, pr, None, 5, 0, 0, pc, None) == E.RR_E_ARG and "no scene" in err()
        assert L.rr_hit_at_device_ordered(fresh.h, 64, pr, None, ph, None) == E.RR_E_ARG and "no scene" in err()
        assert untouched()
        assert same(order_dev(fresh, rays, 64, dev), want_order(R, rays[:64].cpu().numpy()))
    finally:
        fresh.close()
    # a virtual (multi-device) context: the buffers belong to one device
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert L.rr_ray_order_device(v.h, 64, pr, pp, None) == E.RR_E_ARG and "single-device" in err()
        assert L.rr_color_at_device_ordered(v.h, 64, pr, None, 5, 0, 0, pc, None) == E.RR_E_ARG and "single-device" in err()
        assert L.rr_hit_at_device_ordered(v.h, 64, pr, None, ph, None) == E.RR_E_ARG and "single-device" in err()
    finally:
        v.close()
    assert untouched()
    # the per-level switches: the ordered colour query is served by the in-wave kernels only
    chain, _ = V.chain_scene(R)
    renderer.upload(chain)
    with V.environment(RRAY_NO_CHAIN="1"):
        assert L.rr_color_at_device_ordered(h, 64, pr, None, 5, 0, 0, pc, None) == E.RR_E_ARG and "RRAY_NO_CHAIN" in err()
    assert untouched()
    # and the calls still serve afterwards
    assert same(color_ord(renderer, rays, 64, dev), G.color_dev(renderer, rays, 64, dev))
