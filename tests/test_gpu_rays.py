"""Device-resident ray queries on the GPU (rr_camera_rays_device, rr_color_at_device, rr_hit_at_device,
rr_is_shadowed_device).  The definitions are exact: the camera's rays are the oracle's ray_for_pixel
values, and each query writes what its host entry writes for the same rays, bit for bit — so every comparison is
np.array_equal with NaN equal to NaN and no tolerance, but for the colours against the oracle itself, which take the
colour tests' own gate (tests/test_gpu_parity.py: finite, every channel within 1e-5).  Device buffers are torch
tensors; every output is allocated one ray / row / record longer than needed and prefilled with a sentinel, and the
tail must come back untouched.  A call without a stream runs on the context's own (non-blocking) stream, so the helpers
synchronise the device around it; the stream test passes torch's stream and synchronises once, at its end."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import scene_fuzz as F  # noqa: E402
import test_gpu_views_aov as V  # noqa: E402  its scenes, cameras, VARIANTS and oracle helpers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5  # tests/test_gpu_parity.py's gate
SENT = -12345.5  # sentinel of the f64 outputs; bytes 0xA5 in the records, -7 in the int32 ones
LIGHT = (-5.0, 6.0, 2.0)  # chain_scene's point light
E_MAX_DEPTH = 8  # rray.h RR_MAX_DEPTH


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


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def records_equal(R, got, want, what):
    assert got.dtype == want.dtype == R._lib.hit_dtype() and got.shape == want.shape, what
    bad = [n for n in want.dtype.names if not same(got[n], want[n])]
    for n in bad:
        d = (got[n] != want[n]).reshape(len(got), -1).any(axis=1)
        print(f"{what}: field {n} differs in {int(d.sum())} of {len(got)} records")
    assert not bad, (what, bad)


def sync():
    torch.cuda.synchronize()


def camera_rays_dev(r, cam, dev, stream=None):
    """(n + 1, 6) tensor: the camera's n rays, then the sentinel row"""
    n = cam.hsize * cam.vsize
    t = torch.full((n + 1, 6), SENT, dtype=torch.float64, device=dev)
    sync()
    r.camera_rays_device(cam, t.data_ptr(), stream)
    sync()
    assert (t[n:].cpu().numpy() == SENT).all(), "camera_rays_device wrote past its rays"
    return t


def to_dev(a, dev, rows=1):
    """a host array as a device tensor with `rows` sentinel rows behind it"""
    a = np.ascontiguousarray(a, np.float64)
    pad = np.full((rows,) + a.shape[1:], SENT)
    return torch.from_numpy(np.concatenate([a, pad])).to(dev)


def color_dev(r, rays, n, dev, **kw):
    out = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
    sync()
    r.color_at_device(n, rays.data_ptr(), out.data_ptr(), **kw)
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "color_at_device wrote past its rays"
    return a[:n]


def hit_dev(R, r, rays, n, dev):
    out = torch.full((n + 1, 192), 0xA5, dtype=torch.uint8, device=dev)
    sync()
    r.hit_at_device(n, rays.data_ptr(), out.data_ptr())
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == 0xA5).all(), "hit_at_device wrote past its records"
    return np.ascontiguousarray(a[:n]).reshape(-1).view(R._lib.hit_dtype())


def shadow_dev(r, points, lights, n, dev):
    out = torch.full((n + 1,), -7, dtype=torch.int32, device=dev)
    sync()
    r.is_shadowed_device(n, points.data_ptr(), lights.data_ptr(), out.data_ptr())
    sync()
    a = out.cpu().numpy()
    assert (a[n:] == -7).all(), "is_shadowed_device wrote past its pairs"
    return a[:n]


def host_rays(t, n):
    a = t[:n].cpu().numpy()
    return np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:])


# ---- 1. camera rays against the oracle ----
def test_camera_rays_equal_the_oracles_ray_for_pixel(R, renderer, dev):
    import oracle

    _, cam_like = V.chain_scene(R)
    cams = [V.ring(R, cam_like, 16, 16, 2)[1], V.ring(R, cam_like, 13, 11, 3)[2], V.ring(R, cam_like, 1, 1, 1)[0],
            V.ring(R, cam_like, 13, 11, 2, non_affine_at=1)[1]]
    assert list(cams[3].transform)[12:] == [0.0, 0.02, 0.0, 1.05]
    for cam in cams:  # no scene is needed
        n = cam.hsize * cam.vsize
        got = camera_rays_dev(renderer, cam, dev)[:n].cpu().numpy()
        ocam = oracle.Oracle.camera(cam.hsize, cam.vsize, cam.field_of_view, list(cam.transform))
        want = np.array([list(ro) + list(rd) for ro, rd in V.camera_rays(oracle, ocam)])
        assert same(got, want), (cam.hsize, cam.vsize)


# ---- 2. sizes ----
@pytest.fixture(scope="module")
def chain300(R, dev):
    """chain_scene and the 300 rays of a 20 x 15 camera, with the host entries' answers (computed once)"""
    r = R.Renderer(0)
    try:
        scene, cam_like = V.chain_scene(R)
        r.upload(scene)
        cam = V.ring(R, cam_like, 20, 15, 1)[0]
        rays = camera_rays_dev(r, cam, dev)
        o, d = host_rays(rays, 300)
        hits = r.hit_at(o, d)
        pts = np.ascontiguousarray(hits["over_point"])
        lps = np.tile(np.array(LIGHT), (300, 1))
        ref = {"scene": scene, "rays": rays, "colour": r.color_at(o, d), "hits": hits, "points": pts, "lights": lps,
               "shadow": r.is_shadowed(pts, lps)}
    finally:
        r.close()
    assert (hits["object"] >= 0).any() and (hits["object"] < 0).any()
    assert ref["shadow"].any() and not ref["shadow"].all()
    return ref


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 300])
def test_prefixes_equal_the_host_entries(R, renderer, dev, chain300, n):
    renderer.upload(chain300["scene"])
    rays = chain300["rays"]
    assert same(color_dev(renderer, rays, n, dev), chain300["colour"][:n])
    records_equal(R, hit_dev(R, renderer, rays, n, dev), chain300["hits"][:n], f"n {n}")
    got = shadow_dev(renderer, to_dev(chain300["points"][:n], dev), to_dev(chain300["lights"][:n], dev), n, dev)
    assert got.dtype == np.int32 and set(np.unique(got)) <= {0, 1}
    assert same(got.astype(bool), chain300["shadow"][:n])


# ---- 3. every kernel family ----
FAMILIES = list(V.VARIANTS) + [("chain_reflective", "chain"), ("c5_area_light", "c5_area_light.yaml")]


@pytest.mark.parametrize("name,src", FAMILIES, ids=[v[0] for v in FAMILIES])
def test_every_kernel_family(R, renderer, dev, name, src):
    """Colours equal host color_at and the canvas of render(cam); hits equal host hit_at.  The area-light row proves the
    jitter identity (ray i = sample i of the frame, derived from event_key): as first run on an MI355X, 0 of its 143
    colours differ between the device entry, the host entry and the canvas, as in every other row."""
    kw = {}
    if src is None:
        scene, cam_like = V.csg_scene(R)
    elif src == "chain":
        scene, cam_like = V.chain_scene(R)
    elif isinstance(src, tuple):
        P, spec, _, _ = F.build(src[1])
        scene, cam_like = P.b, F.cameras(P, spec, 16, 16)[0]
    else:
        scene = V.yaml_scene(R, src, 16, 16, 1, GOLDEN if src == "perturbed_pattern.yaml" else SCENES)
        cam_like = scene.camera
    if name == "c5_area_light":
        kw = {"seed": 12345, "jitter_mode": 0}
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 13, 11, 2)[1]
    n = 143
    rays = camera_rays_dev(renderer, cam, dev)
    o, d = host_rays(rays, n)
    got = color_dev(renderer, rays, n, dev, **kw)
    host = renderer.color_at(o, d, **kw)
    frame = renderer.render(cam, canvas=True, **kw)["canvas"].reshape(n, 3)
    print(f"{name}: colours differing from host color_at {int((got != host).any(axis=1).sum())}, from the canvas "
          f"{int((got != frame).any(axis=1).sum())}, host from the canvas {int((host != frame).any(axis=1).sum())} of {n}")
    assert same(got, host), name
    assert same(got, frame), name
    records_equal(R, hit_dev(R, renderer, rays, n, dev), renderer.hit_at(o, d), name)


# ---- 4. the oracle itself ----
def _oracle_default(R, oracle):
    b, o = R.SceneBuilder(), oracle.Oracle()
    b.point_light((-10, 10, -10), (1, 1, 1))
    o.point_light((-10, 10, -10), (1, 1, 1))
    m = (0.1, 0.7, 0.2, 200.0, 0.0, 0.0, 1.0)
    b.sphere(material=m, pattern=b.pattern("solid", color=(0.8, 1.0, 0.6)))
    o.add("sphere", material=m, pattern=o.pattern("solid", color=(0.8, 1.0, 0.6)))
    half = (0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 1)
    b.sphere(transform=half)
    o.add("sphere", transform=half)
    return b, o, R.camera(8, 8, math.pi / 3, oracle.Oracle.mat.view_transform((0, 1.5, -5), (0, 0, 0), (0, 1, 0)))


def _oracle_chain(R, oracle):
    """chain_scene on both sides"""
    b, cam_like = V.chain_scene(R)
    o = oracle.Oracle()
    o.point_light(LIGHT, (1, 1, 1))
    o.add("plane", transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.2, 0.0, 1.0),
          pattern=o.pattern("checker", a=o.pattern("solid", color=(1, 1, 1)), b=o.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9))):
        o.add("sphere", transform=V.scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.4, 0.0, 1.0),
              pattern=o.pattern("solid", color=col))
    return b, o, cam_like


@pytest.mark.parametrize("kind", ["default", "chain"])
def test_records_and_colours_against_the_oracle(R, renderer, dev, kind):
    import oracle

    b, o, cam = (_oracle_default if kind == "default" else _oracle_chain)(R, oracle)
    renderer.upload(b)
    assert (cam.hsize, cam.vsize) == (8, 8)
    rays = camera_rays_dev(renderer, cam, dev)
    ocam = oracle.Oracle.camera(8, 8, cam.field_of_view, list(cam.transform))
    orays = V.camera_rays(oracle, ocam)
    records_equal(R, hit_dev(R, renderer, rays, 64, dev), V.oracle_hits(R, o, orays), kind)  # ids: the order of creation
    got = color_dev(renderer, rays, 64, dev)
    ref = np.array([o.color_at(ro, rd, 5)[:3] for ro, rd in orays])
    err = float(np.max(np.abs(got - ref)))
    print(f"{kind}: colours against the oracle: max|d|={err:.3g} bit-exact={float(np.mean(got == ref)):.6f}")
    assert np.all(np.isfinite(got)), kind
    assert err <= TOL, f"{kind}: max |delta| {err} > {TOL}"


# ---- 5. passes ----
@pytest.mark.parametrize("batch,W,H", [("128", 20, 15), ("1024", 50, 50)], ids=["batch128_n300", "batch1024_n2500"])
def test_passes_under_a_small_batch(R, renderer, dev, batch, W, H):
    """A context created under a small RRAY_BATCH answers like a default one.  rr_create raises a batch below 1024 to
    1024, so the 300 rays under RRAY_BATCH=128 are one pass there; the 2500 rays under 1024 are three passes of the
    records (1024, 1024, 452) and of the colour levels."""
    scene, cam_like = V.chain_scene(R)
    cam = V.ring(R, cam_like, W, H, 1)[0]
    n = W * H
    renderer.upload(scene)
    rays = camera_rays_dev(renderer, cam, dev)
    want_c, want_h = color_dev(renderer, rays, n, dev), hit_dev(R, renderer, rays, n, dev)
    with V.environment(RRAY_BATCH=batch):  # read when a context is created
        r = R.Renderer(0)
    try:
        r.upload(scene)
        assert same(color_dev(r, rays, n, dev), want_c)
        records_equal(R, hit_dev(R, r, rays, n, dev), want_h, f"batch {batch}")
        assert r.last_stats()["samples"] == n
    finally:
        r.close()


# ---- 6. a torch stream, no synchronisation before the end ----
def test_queries_on_a_torch_stream(R, renderer, dev):
    scene, cam_like = V.chain_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 16, 16, 1)[0]
    n = 256
    sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        rays = torch.full((n + 1, 6), SENT, dtype=torch.float64, device=dev)
        rgb = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        hits = torch.full((n + 1, 192), 0xA5, dtype=torch.uint8, device=dev)
        renderer.camera_rays_device(cam, rays.data_ptr(), s.cuda_stream)
        rays[:n, :3] += torch.tensor([0.25, 0.125, -0.5], dtype=torch.float64, device=dev)  # a lens shift, on the stream
        renderer.color_at_device(n, rays.data_ptr(), rgb.data_ptr(), stream=s.cuda_stream)
        renderer.hit_at_device(n, rays.data_ptr(), hits.data_ptr(), stream=s.cuda_stream)
        brightest = rgb[:n].max()
        n_hits = (hits.view(torch.int32)[:n, 0] >= 0).sum()
        nearest = torch.where(hits.view(torch.int32)[:n, 0] >= 0, hits.view(torch.float64)[:n, 1], math.inf).min()
    s.synchronize()
    o, d = host_rays(rays, n)
    assert (rays[n:].cpu().numpy() == SENT).all()
    want_c, want_h = renderer.color_at(o, d), renderer.hit_at(o, d)
    assert same(rgb[:n].cpu().numpy(), want_c) and (rgb[n:].cpu().numpy() == SENT).all()
    a = hits.cpu().numpy()
    assert (a[n:] == 0xA5).all()
    records_equal(R, np.ascontiguousarray(a[:n]).reshape(-1).view(R._lib.hit_dtype()), want_h, "stream")
    assert float(brightest) == float(want_c.max())
    assert int(n_hits) == int((want_h["object"] >= 0).sum()) > 0
    assert float(nearest) == float(want_h["t"][want_h["object"] >= 0].min())


# ---- 7. isolation ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_queries_leave_frames_and_batches_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = V.yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = V.ring(R, scene.camera, 16, 16, 3)

            def queries():
                rays = camera_rays_dev(r, cams[1], dev)
                color_dev(r, rays, 256, dev)
                h = hit_dev(R, r, rays, 256, dev)
                lights = to_dev(np.tile(np.array([-10.0, 10.0, -10.0]), (256, 1)), dev)
                shadow_dev(r, to_dev(h["over_point"], dev), lights, 256, dev)

            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            queries()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            before = r.render_views(cams, max_depth=5)
            queries()
            after = r.render_views(cams, max_depth=5)
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
    finally:
        r.close()


# ---- 8. stats and NaN rays ----
def test_stats_after_the_queries(R, renderer, dev, chain300):
    renderer.upload(chain300["scene"])
    n = 300
    want = chain300["hits"]
    hit_dev(R, renderer, chain300["rays"], n, dev)
    # a shadow query in between leaves the pending stats alone
    shadow_dev(renderer, to_dev(chain300["points"], dev), to_dev(chain300["lights"], dev), n, dev)
    st = renderer.last_stats()
    assert st["rays"] == st["samples"] == n
    assert st["n1n2_scans"] == int((want["object"] >= 0).sum()) > 0
    assert st["shadow_rays"] == st["shade_events"] == 0 and st["nan_rays"] == 0
    assert st["kernel_ms"] > 0
    # colours: the counters of the frame over the same rays (the 20 x 15 camera's), whose samples they are
    color_dev(renderer, chain300["rays"], n, dev)
    st = renderer.last_stats()
    frame = renderer.render(V.ring(R, V.chain_scene(R)[1], 20, 15, 1)[0])["stats"]
    assert st["samples"] == n == frame["samples"] and st["kernel_ms"] > 0
    for k in ("rays", "shadow_rays", "shade_events", "n1n2_scans", "nan_rays"):
        assert st[k] == frame[k], k


def test_nan_rays_are_counted_and_the_device_entries_return_ok(R, renderer, dev):
    """the NaN scene of tests/test_gpu_views_aov.py: every ray of a NaN camera meets two NaN entries"""
    L, E = R.lib(), R._lib
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    b.plane()
    b.plane(transform=(1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 1))
    renderer.upload(b)
    sound = R.camera(8, 8, 1.0, V.translate(0, -0.5, 0))
    nan_cam = R.camera(8, 8, 1.0, tuple([math.nan] * 12 + [0.0, 0.0, 0.0, 1.0]))
    rays = torch.cat([camera_rays_dev(renderer, sound, dev)[:64], camera_rays_dev(renderer, nan_cam, dev)])  # 128 + sentinel
    n = 128
    o, d = host_rays(rays, n)
    assert np.isnan(d[64:]).all() and not np.isnan(d[:64]).any()
    # the host entries: RR_E_NAN after writing, the count in the stats (hits) or the message (colours)
    out_h = np.zeros(n, E.hit_dtype())
    assert L.rr_hit_at(renderer.h, n, o.ctypes.data_as(E._D), d.ctypes.data_as(E._D),
                       out_h.ctypes.data_as(C.POINTER(E.Hit))) == E.RR_E_NAN
    host_nan_hits = renderer.last_stats()["nan_rays"]
    out_c = np.zeros((n, 3))
    assert L.rr_color_at(renderer.h, n, o.ctypes.data_as(E._D), d.ctypes.data_as(E._D), 5, 0, 0,
                         out_c.ctypes.data_as(E._D)) == E.RR_E_NAN
    host_nan_colours = int(L.rr_last_error().decode().split()[0])
    assert host_nan_hits == 64 and host_nan_colours >= 64
    got_h = hit_dev(R, renderer, rays, n, dev)  # returns RR_OK (the mirror raises on anything else)
    assert renderer.last_stats()["nan_rays"] == host_nan_hits
    records_equal(R, got_h, out_h, "nan rays")
    got_c = color_dev(renderer, rays, n, dev)
    assert renderer.last_stats()["nan_rays"] == host_nan_colours
    assert same(got_c, out_c)


# ---- 9. refusals and n == 0 ----
def test_refusals_and_the_empty_batch(R, renderer, dev):
    L, E = R.lib(), R._lib
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 8, 8, 1)[0]
    rays = camera_rays_dev(renderer, cam, dev)
    rgb = torch.full((65, 3), SENT, dtype=torch.float64, device=dev)
    hits = torch.full((65, 192), 0xA5, dtype=torch.uint8, device=dev)
    flags = torch.full((65,), -7, dtype=torch.int32, device=dev)
    sync()
    pr, pc, ph, pf = (C.c_void_p(t.data_ptr()) for t in (rays, rgb, hits, flags))
    h = renderer.h

    def err():
        return L.rr_last_error().decode()

    def untouched():
        sync()
        return bool((rgb.cpu().numpy() == SENT).all() and (hits.cpu().numpy() == 0xA5).all() and
                    (flags.cpu().numpy() == -7).all())

    for rem in (-1, E_MAX_DEPTH + 1):
        assert L.rr_color_at_device(h, 64, pr, rem, 0, 0, pc, None) == E.RR_E_LIMIT and "remaining" in err()
    # null buffers with n > 0, n < 0
    assert L.rr_color_at_device(h, 64, None, 5, 0, 0, pc, None) == E.RR_E_ARG and "null" in err()
    assert L.rr_color_at_device(h, 64, pr, 5, 0, 0, None, None) == E.RR_E_ARG
    assert L.rr_hit_at_device(h, 64, None, ph, None) == E.RR_E_ARG
    assert L.rr_hit_at_device(h, 64, pr, None, None) == E.RR_E_ARG
    assert L.rr_is_shadowed_device(h, 64, None, pr, pf, None) == E.RR_E_ARG
    assert L.rr_is_shadowed_device(h, 64, pr, None, pf, None) == E.RR_E_ARG
    assert L.rr_is_shadowed_device(h, 64, pr, pr, None, None) == E.RR_E_ARG
    assert L.rr_color_at_device(h, -1, pr, 5, 0, 0, pc, None) == E.RR_E_ARG and "negative" in err()
    assert L.rr_hit_at_device(h, -1, pr, ph, None) == E.RR_E_ARG
    assert L.rr_is_shadowed_device(h, -1, pr, pr, pf, None) == E.RR_E_ARG
    # n >= 2^32: the sample index is 32-bit (refused before anything is read)
    assert L.rr_color_at_device(h, 2**32, pr, 5, 0, 0, pc, None) == E.RR_E_LIMIT and "2^32" in err()
    assert L.rr_hit_at_device(h, 2**32, pr, ph, None) == E.RR_E_LIMIT
    assert L.rr_is_shadowed_device(h, 2**32, pr, pr, pf, None) == E.RR_E_LIMIT
    # n == 0: RR_OK, nothing enqueued, null buffers allowed
    assert L.rr_color_at_device(h, 0, pr, 5, 0, 0, pc, None) == 0
    assert L.rr_color_at_device(h, 0, None, 5, 0, 0, None, None) == 0
    assert L.rr_hit_at_device(h, 0, pr, ph, None) == 0 and L.rr_hit_at_device(h, 0, None, None, None) == 0
    assert L.rr_is_shadowed_device(h, 0, pr, pr, pf, None) == 0
    assert untouched()
    # camera rays: null arguments, sizes < 1, 2^32 rays or more
    assert L.rr_camera_rays_device(h, None, pr, None) == E.RR_E_ARG
    assert L.rr_camera_rays_device(h, C.byref(cam), None, None) == E.RR_E_ARG
    for hs, vs, code in ((0, 8, E.RR_E_ARG), (8, 0, E.RR_E_ARG), (-1, 8, E.RR_E_ARG), (65536, 65536, E.RR_E_LIMIT),
                         (2**32, 1, E.RR_E_LIMIT)):
        bad = E.Camera.from_buffer_copy(cam)
        bad.hsize, bad.vsize = hs, vs
        assert L.rr_camera_rays_device(h, C.byref(bad), pr, None) == code, (hs, vs)
    sync()
    assert (rays[64:].cpu().numpy() == SENT).all()
    # no scene uploaded: the queries are refused, the camera's rays are not
    fresh = R.Renderer(0)
    try:
        assert L.rr_color_at_device(fresh.h, 64, pr, 5, 0, 0, pc, None) == E.RR_E_ARG and "no scene" in err()
        assert L.rr_hit_at_device(fresh.h, 64, pr, ph, None) == E.RR_E_ARG and "no scene" in err()
        assert L.rr_is_shadowed_device(fresh.h, 64, pr, pr, pf, None) == E.RR_E_ARG and "no scene" in err()
        assert same(camera_rays_dev(fresh, cam, dev).cpu().numpy(), rays.cpu().numpy())
    finally:
        fresh.close()
    # a virtual (multi-device) context: the buffers belong to one device
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert L.rr_camera_rays_device(v.h, C.byref(cam), pr, None) == E.RR_E_ARG and "single-device" in err()
        assert L.rr_color_at_device(v.h, 64, pr, 5, 0, 0, pc, None) == E.RR_E_ARG and "single-device" in err()
        assert L.rr_hit_at_device(v.h, 64, pr, ph, None) == E.RR_E_ARG and "single-device" in err()
        assert L.rr_is_shadowed_device(v.h, 64, pr, pr, pf, None) == E.RR_E_ARG and "single-device" in err()
    finally:
        v.close()
    assert untouched()
    # and the calls still serve afterwards
    o, d = host_rays(rays, 64)
    assert same(color_dev(renderer, rays, 64, dev), renderer.color_at(o, d))

