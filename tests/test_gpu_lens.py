"""Lens frames on the GPU (rr_lens_rays_device, rr_render_lens, rr_render_lens_device).  The
definitions are exact: the rays are rray_amd.lens_rays' values, and a frame is lens_resolve of what rr_color_at_device
writes for the whole frame's rays — so every comparison is np.array_equal with NaN equal to NaN and no tolerance, but for
the colours against the oracle itself, which take the colour tests' own gate (tests/test_gpu_parity.py: finite, every
channel within 1e-5).  Device buffers are torch tensors with a sentinel row behind every output, as in
tests/test_gpu_rays.py, whose helpers these tests use."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import test_gpu_rays as Q  # noqa: E402  its helpers: same, sync, color_dev, camera_rays_dev, SENT
import test_gpu_views_aov as V  # noqa: E402  its scenes, cameras and environment switch

pytestmark = pytest.mark.gpu
TOL = 1e-5  # tests/test_gpu_parity.py's gate
SENT = Q.SENT
same = Q.same
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


def lens_rays_dev(r, cam, lens, dev, first=0, n=None, stream=None):
    """(n * S + 1, 6) tensor: the window's rays, then the sentinel row"""
    n = cam.hsize * cam.vsize - first if n is None else n
    m = n * lens.samples
    t = torch.full((m + 1, 6), SENT, dtype=torch.float64, device=dev)
    Q.sync()
    r.lens_rays_device(cam, lens, t.data_ptr(), first, n, stream)
    Q.sync()
    assert (t[m:].cpu().numpy() == SENT).all(), "lens_rays_device wrote past its rays"
    return t


def lens_frame_dev(R, r, cam, lens, dev, stream=None, **kw):
    """rr_render_lens_device into a tensor with a sentinel row: (H, W, 3)"""
    n = cam.hsize * cam.vsize
    out = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
    o = R._lib.RenderOpts(1, kw.get("max_depth", 5), kw.get("seed", 0), kw.get("jitter_mode", 0), 0, 1, 8, 0, 0, 0)
    Q.sync()
    r.render_lens_device(cam, o, lens, out.data_ptr(), stream)
    Q.sync()
    a = out.cpu().numpy()
    assert (a[n:] == SENT).all(), "render_lens_device wrote past its image"
    return a[:n].reshape(cam.vsize, cam.hsize, 3)


def composed(R, r, cam, lens, dev, **kw):
    """the definition through the public entries: lens_resolve(color_at_device(lens_rays_device(whole frame)), S), and
    the stats of that one colour call"""
    n = cam.hsize * cam.vsize * lens.samples
    rays = lens_rays_dev(r, cam, lens, dev)
    rgb = Q.color_dev(r, rays, n, dev, remaining=kw.get("max_depth", 5), seed=kw.get("seed", 0),
                      jitter_mode=kw.get("jitter_mode", 0))
    return R.lens_resolve(rgb, lens.samples).reshape(cam.vsize, cam.hsize, 3), r.last_stats()


def glass_scene(R):
    """a glass sphere with an air bubble and a mirror ball over a checker floor: transparency (refraction halves)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.1, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    b.sphere(transform=V.scale_at(1.0, 0.2, 0.0, -4.0), material=(0.05, 0.1, 0.9, 300.0, 0.6, 0.9, 1.5))
    b.sphere(transform=V.scale_at(0.5, 0.2, 0.0, -4.0), material=(0.05, 0.1, 0.9, 300.0, 0.0, 0.9, 1.0))
    b.sphere(transform=V.scale_at(0.6, -1.7, -0.4, -5.0), material=(0.1, 0.6, 0.4, 50.0, 0.5, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.9, 0.7, 0.2)))
    return b, R.camera(8, 8, math.pi / 3, V.translate(0, -0.5, 0))


AREA = ((-3.0, 5.0, 0.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (1.0, 1.0, 1.0), 3)
AREA_SPHERES = ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9)))


def area_scene(R, oracle=None):
    """chain_scene's geometry under a 3 x 3 area light: soft shadows, so every sample's jitter identity shows; with
    `oracle`, the same scene on the oracle's side too"""
    b = R.SceneBuilder()
    b.area_light(*AREA)
    b.plane(transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.2, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in AREA_SPHERES:
        b.sphere(transform=V.scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.4, 0.0, 1.0),
                 pattern=b.pattern("solid", color=col))
    cam = R.camera(8, 8, math.pi / 3, V.translate(0, -0.5, 0))
    if oracle is None:
        return b, cam
    o = oracle.Oracle()
    o.area_light(*AREA)
    o.add("plane", transform=V.translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.2, 0.0, 1.0),
          pattern=o.pattern("checker", a=o.pattern("solid", color=(1, 1, 1)), b=o.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in AREA_SPHERES:
        o.add("sphere", transform=V.scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.4, 0.0, 1.0),
              pattern=o.pattern("solid", color=col))
    return b, cam, o


SCENES = {"flat": V.flat_scene, "chain": V.chain_scene, "csg": V.csg_scene, "glass": glass_scene, "area": area_scene}


# ---- 1. rays against the mirror ----
LENSES = [dict(), dict(pixel_jitter=True, seed=5), dict(aperture=0.3, focal_distance=4.5, seed=6),
          dict(pixel_jitter=True, aperture=0.3, focal_distance=4.5, seed=2**63 + 9)]


@pytest.mark.parametrize("W,H", [(7, 5), (13, 5), (16, 4), (65, 1)], ids=["7x5", "13x5", "16x4", "65x1"])
def test_rays_equal_the_mirror(R, renderer, dev, W, H):
    _, cam_like = V.chain_scene(R)
    cam = V.ring(R, cam_like, W, H, 2)[1]  # no scene is needed
    n = W * H
    for S in (1, 3, 5, 16):  # 64 % 5 != 0: a pixel's samples straddle a wave
        for kw in LENSES:
            lens = R.Lens(samples=S, **kw)
            want = R.lens_rays(cam, lens)
            got = lens_rays_dev(renderer, cam, lens, dev)[:n * S].cpu().numpy()
            assert same(got, want), (W, H, S, kw)
            # windows: starting mid-row, one pixel, 63 pixels (clipped to the frame), the last pixel, none
            for first, m in ((W // 2 + (W if H > 1 else 0), 1), (1, min(63, n - 1)), (n - 1, 1), (2, 0)):
                win = lens_rays_dev(renderer, cam, lens, dev, first, m)[:m * S].cpu().numpy()
                assert same(win, want[first * S:(first + m) * S]), (W, H, S, kw, first, m)
    # the degenerate lens is the camera itself
    assert same(lens_rays_dev(renderer, cam, R.Lens(), dev).cpu().numpy(), Q.camera_rays_dev(renderer, cam, dev).cpu().numpy())


# ---- 2. the frame against the public entries ----
FRAMES = [("flat", 5, 2, 0), ("flat", 0, 16, 0), ("chain", 5, 5, 0), ("chain", 0, 1, 0), ("csg", 5, 2, 0),
          ("glass", 5, 5, 0), ("glass", 0, 2, 0), ("area", 5, 16, 0), ("area", 5, 5, 1), ("area", 0, 2, 0),
          ("chain", 5, 16, 0), ("csg", 0, 1, 0), ("flat", 5, 10, 0), ("chain", 0, 17, 0)]


@pytest.mark.parametrize("name,depth,S,jm", FRAMES, ids=[f"{n}_d{d}_S{s}_jm{j}" for n, d, s, j in FRAMES])
def test_frame_equals_the_composition_of_the_public_entries(R, renderer, dev, name, depth, S, jm):
    scene, cam_like = SCENES[name](R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 13, 11, 2)[1]
    kw = dict(max_depth=depth, seed=12345, jitter_mode=jm)
    for lens in (R.Lens(S, True, 0.2, 4.5, seed=3), R.Lens(S)):
        want, st_want = composed(R, renderer, cam, lens, dev, **kw)
        got = renderer.render_lens(cam, lens, **kw)
        assert same(got["avg"], want), (name, lens)
        assert got["stats"]["samples"] == 143 * S == st_want["samples"]
        for k in ("rays", "shadow_rays", "shade_events", "n1n2_scans", "nan_rays"):
            assert got["stats"][k] == st_want[k], (name, k)
    if S == 1:  # the last lens: one ray through every pixel centre, the plain frame
        plain = renderer.render(cam, **kw)
        assert same(got["avg"], plain["avg"]), name
        for k in ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples", "nan_rays"):
            assert got["stats"][k] == plain["stats"][k], (name, k)


# ---- 3. passes ----
@pytest.mark.parametrize("env", [dict(RRAY_LENS_PASS="64"), dict(RRAY_LENS_PASS="1"), dict(RRAY_BATCH="1024"),
                                 dict(RRAY_LENS_PASS="64", RRAY_BATCH="1024")],
                         ids=["pass64", "pass1_rounds_up", "batch1024", "pass64_batch1024"])
def test_passes_equal_the_default_contexts_frame(R, renderer, dev, env):
    """20 x 10 with S = 3 under RRAY_LENS_PASS=64: passes of 64, 64, 64 and 8 pixels (192, 192, 192 and 24 rays, each
    starting at a multiple of 64 rays); under RRAY_BATCH=1024 with S = 16 the default pass's 3200 rays run as four
    batches of the levels."""
    with V.environment(**env):  # read when a context is created
        r = R.Renderer(0)
    try:
        for name, jm in (("chain", 0), ("area", 0), ("area", 1)):
            scene, cam_like = SCENES[name](R)
            cam = V.ring(R, cam_like, 20, 10, 1)[0]
            renderer.upload(scene)
            r.upload(scene)
            for lens in (R.Lens(3, True, 0.2, 4.5, seed=8), R.Lens(16, True, seed=1)):
                kw = dict(max_depth=5, seed=77, jitter_mode=jm)
                want = renderer.render_lens(cam, lens, **kw)
                got = r.render_lens(cam, lens, **kw)
                assert same(got["avg"], want["avg"]), (env, name, lens)
                for k in ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples", "nan_rays"):
                    assert got["stats"][k] == want["stats"][k], (env, name, k)
                assert same(lens_frame_dev(R, r, cam, lens, dev, **kw), want["avg"])  # the sentinel behind the last pass
    finally:
        r.close()


# ---- 4. the oracle itself ----
def test_a_thin_lens_frame_against_the_oracle(R, renderer, dev):
    import oracle

    scene, cam_like, o = area_scene(R, oracle)
    renderer.upload(scene)
    cam = R.camera(12, 9, cam_like.field_of_view, list(cam_like.transform))
    lens = R.Lens(4, True, 0.15, 4.5, seed=21)
    seed, jm = 4321, 0
    got = renderer.render_lens(cam, lens, max_depth=5, seed=seed, jitter_mode=jm)["avg"]
    rays = R.lens_rays(cam, lens)
    ref = np.zeros((len(rays), 3))
    for i, ray in enumerate(rays):
        o.set_context(seed, jm, sample=i)
        ref[i] = o.color_at(ray[:3].tolist() + [1.0], ray[3:].tolist() + [0.0], 5)[:3]
    want = R.lens_resolve(ref, 4).reshape(9, 12, 3)
    err = float(np.max(np.abs(got - want)))
    print(f"thin-lens frame against the oracle: max|d|={err:.3g} bit-exact={float(np.mean(got == want)):.6f}")
    assert np.all(np.isfinite(got))
    assert err <= TOL, f"max |delta| {err} > {TOL}"


# ---- 5. the device entry ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_device_entry_on_a_torch_stream(R, renderer, dev):
    scene, cam_like = area_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 16, 12, 1)[0]
    lens = R.Lens(5, True, 0.2, 4.5, seed=4)
    n = 192
    want, st_want = composed(R, renderer, cam, lens, dev, seed=9)
    o = R._lib.RenderOpts(1, 5, 9, 0, 0, 1, 8, 0, 0, 0)
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        img = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        renderer.render_lens_device(cam, o, lens, img.data_ptr(), s.cuda_stream)
        brightest = img[:n].max()
        o2 = R._lib.RenderOpts(1, 5, 9, 0, 0, 1, 8, R._lib.RR_NO_FRAME_TIMING, 0, 0)
        img2 = torch.full((n + 1, 3), SENT, dtype=torch.float64, device=dev)
        renderer.render_lens_device(cam, o2, lens, img2.data_ptr(), s.cuda_stream)
    s.synchronize()
    a = img.cpu().numpy()
    assert same(a[:n].reshape(12, 16, 3), want) and (a[n:] == SENT).all()
    assert same(img2.cpu().numpy(), a)
    assert float(brightest) == float(want.max())
    st = renderer.last_stats()
    assert st["kernel_ms"] == 0  # RR_NO_FRAME_TIMING
    assert st["samples"] == n * 5
    for k in ("rays", "shadow_rays", "shade_events", "n1n2_scans", "nan_rays"):
        assert st[k] == st_want[k], k
    lens_frame_dev(R, renderer, cam, lens, dev, seed=9)
    assert renderer.last_stats()["kernel_ms"] > 0


def test_nan_rays_are_counted(R, renderer, dev):
    """two planes: a NaN ray meets two NaN entries (tests/test_gpu_rays.py).  The camera stays affine, so the lens takes
    it; its NaN image plane makes every ray NaN."""
    L, E = R.lib(), R._lib
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    b.plane()
    b.plane(transform=(1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 1))
    renderer.upload(b)
    cam = E.Camera.from_buffer_copy(R.camera(8, 8, 1.0, V.translate(0, -0.5, 0)))
    cam.half_width = math.nan
    lens = R.Lens(3, True, seed=2)
    assert np.isnan(R.lens_rays(cam, lens)[:, 3:]).all()
    want, st_want = composed(R, renderer, cam, lens, dev)
    assert st_want["nan_rays"] >= 192
    got = lens_frame_dev(R, renderer, cam, lens, dev)  # returns RR_OK (the mirror raises on anything else)
    assert renderer.last_stats()["nan_rays"] == st_want["nan_rays"]
    assert same(got, want)
    # the host entry: RR_E_NAN after writing
    o = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, 0, 0, 0)
    d = lens.desc()
    out = np.full((8, 8, 3), SENT)
    st = E.Stats()
    assert L.rr_render_lens(renderer.h, C.byref(cam), C.byref(o), C.byref(d), out.ctypes.data_as(E._D),
                            C.byref(st)) == E.RR_E_NAN
    assert same(out, want) and st.nan_rays == st_want["nan_rays"]


def test_lens_frames_leave_frames_and_batches_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = V.yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = V.ring(R, scene.camera, 16, 16, 3)

            def lens_work():
                r.render_lens(cams[1], R.Lens(3, True, 0.1, 5.0, seed=1))
                lens_frame_dev(R, r, cams[2], R.Lens(2), dev)
                lens_rays_dev(r, cams[0], R.Lens(2, True), dev)

            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            lens_work()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            before = r.render_views(cams, max_depth=5)
            lens_work()
            after = r.render_views(cams, max_depth=5)
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
    finally:
        r.close()


def test_refusals(R, renderer, dev):
    L, E = R.lib(), R._lib
    scene, cam_like = V.flat_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 8, 8, 1)[0]
    rays = torch.full((64 * 2 + 1, 6), SENT, dtype=torch.float64, device=dev)
    img = torch.full((65, 3), SENT, dtype=torch.float64, device=dev)
    host = np.full((8, 8, 3), SENT)
    Q.sync()
    pr, pi, ph = C.c_void_p(rays.data_ptr()), C.c_void_p(img.data_ptr()), host.ctypes.data_as(E._D)
    h, pc = renderer.h, C.byref(cam)

    def err():
        return L.rr_last_error().decode()

    def opts(**kw):
        f = dict(aa=1, max_depth=5, seed=0, jitter_mode=0, part=0, nparts=1, block_rows=8, flags=0, row_begin=0, row_end=0)
        f.update(kw)
        return C.byref(E.RenderOpts(*f.values()))

    def lens(**kw):
        f = dict(samples=2, pixel_jitter=0, aperture=0.0, focal_distance=1.0, seed=0)
        f.update(kw)
        return C.byref(E.LensDesc(*f.values()))

    def frame(o=None, ln=None, cam_=pc, ctx=h):
        """(device entry, host entry) return codes"""
        o, ln = o or opts(), ln or lens()
        return (L.rr_render_lens_device(ctx, cam_, o, ln, pi, None), L.rr_render_lens(ctx, cam_, o, ln, ph, None))

    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    # null pointers
    assert L.rr_render_lens_device(None, pc, opts(), lens(), pi, None) == ARG
    assert L.rr_render_lens_device(h, None, opts(), lens(), pi, None) == ARG
    assert L.rr_render_lens_device(h, pc, None, lens(), pi, None) == ARG
    assert L.rr_render_lens_device(h, pc, opts(), None, pi, None) == ARG
    assert L.rr_render_lens_device(h, pc, opts(), lens(), None, None) == ARG and "null" in err()
    assert L.rr_render_lens(None, pc, opts(), lens(), ph, None) == ARG
    assert L.rr_render_lens(h, None, opts(), lens(), ph, None) == ARG
    assert L.rr_render_lens(h, pc, None, lens(), ph, None) == ARG
    assert L.rr_render_lens(h, pc, opts(), None, ph, None) == ARG
    assert L.rr_render_lens(h, pc, opts(), lens(), None, None) == ARG
    assert L.rr_lens_rays_device(None, pc, lens(), 0, 64, pr, None) == ARG
    assert L.rr_lens_rays_device(h, None, lens(), 0, 64, pr, None) == ARG
    assert L.rr_lens_rays_device(h, pc, None, 0, 64, pr, None) == ARG
    assert L.rr_lens_rays_device(h, pc, lens(), 0, 64, None, None) == ARG
    # the lens
    for kw in (dict(samples=0), dict(samples=-1), dict(samples=E.RR_MAX_LENS_SAMPLES + 1), dict(aperture=-0.1),
               dict(aperture=math.nan), dict(aperture=math.inf), dict(aperture=0.1, focal_distance=0.0),
               dict(aperture=0.1, focal_distance=-1.0), dict(aperture=0.1, focal_distance=math.nan),
               dict(aperture=0.1, focal_distance=math.inf)):
        assert frame(ln=lens(**kw)) == (ARG, ARG), kw
        assert L.rr_lens_rays_device(h, pc, lens(**kw), 0, 64, pr, None) == ARG, kw
    # a pinhole ignores its focal distance
    assert L.rr_lens_rays_device(h, pc, lens(focal_distance=math.nan), 0, 0, pr, None) == 0
    # the options
    for kw in (dict(aa=2), dict(aa=0), dict(part=1, nparts=2), dict(nparts=2), dict(row_begin=0, row_end=4),
               dict(row_begin=2, row_end=4), dict(flags=E.RR_OUT_AVG), dict(flags=E.RR_OUT_CANVAS),
               dict(flags=E.RR_OUT_AVG_F32), dict(flags=E.RR_PART_INTERLEAVE),
               dict(flags=E.RR_NO_FRAME_TIMING | E.RR_OUT_AVG)):
        assert frame(o=opts(**kw)) == (ARG, ARG), kw
    for depth in (-1, E_MAX_DEPTH + 1):
        assert frame(o=opts(max_depth=depth)) == (LIM, LIM) and "max_depth" in err()
    # the window
    for first, n in ((-1, 1), (0, 65), (64, 1), (65, 0), (0, -1), (2**62, 2**62)):
        assert L.rr_lens_rays_device(h, pc, lens(), first, n, pr, None) == ARG and "window" in err(), (first, n)
    for first in (0, 17, 64):  # n_pixels == 0: RR_OK, nothing enqueued
        assert L.rr_lens_rays_device(h, pc, lens(), first, 0, pr, None) == 0
    # W * H * S >= 2^32, sizes < 1
    big = E.Camera.from_buffer_copy(cam)
    big.hsize, big.vsize = 2**16, 2**15
    assert frame(ln=lens(samples=2), cam_=C.byref(big)) == (LIM, LIM) and "2^32" in err()
    assert L.rr_lens_rays_device(h, C.byref(big), lens(samples=2), 0, 1, pr, None) == LIM
    big.hsize, big.vsize = 2**32, 1
    assert frame(cam_=C.byref(big)) == (LIM, LIM)
    for hs, vs in ((0, 8), (8, 0), (-1, 8)):
        big.hsize, big.vsize = hs, vs
        assert frame(cam_=C.byref(big)) == (ARG, ARG)
        assert L.rr_lens_rays_device(h, C.byref(big), lens(), 0, 0, pr, None) == ARG
    # a camera whose inverse is not affine
    na = V.ring(R, cam_like, 8, 8, 2, non_affine_at=1)[1]
    assert frame(cam_=C.byref(na)) == (E.RR_E_NONAFFINE, E.RR_E_NONAFFINE) and "affine" in err()
    assert L.rr_lens_rays_device(h, C.byref(na), lens(), 0, 64, pr, None) == E.RR_E_NONAFFINE
    Q.sync()
    assert (rays.cpu().numpy() == SENT).all() and (img.cpu().numpy() == SENT).all() and (host == SENT).all()
    # no scene uploaded: the frames are refused, the rays are not
    fresh = R.Renderer(0)
    try:
        assert frame(ctx=fresh.h) == (ARG, ARG) and "no scene" in err()
        got = lens_rays_dev(fresh, cam, R.Lens(2, True, 0.1, 3.0), dev)[:128].cpu().numpy()
        assert same(got, R.lens_rays(cam, R.Lens(2, True, 0.1, 3.0)))
    finally:
        fresh.close()
    # a virtual (multi-device) context
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert frame(ctx=v.h) == (ARG, ARG) and "single-device" in err()
        assert L.rr_lens_rays_device(v.h, pc, lens(), 0, 64, pr, None) == ARG and "single-device" in err()
    finally:
        v.close()
    Q.sync()
    assert (rays.cpu().numpy() == SENT).all() and (img.cpu().numpy() == SENT).all() and (host == SENT).all()
    # and the calls still serve afterwards
    assert frame() == (0, 0)
    Q.sync()
    assert same(img[:64].cpu().numpy().reshape(8, 8, 3), host) and (img[64:].cpu().numpy() == SENT).all()
    assert same(host, renderer.render_lens(cam, R.Lens(2))["avg"])


# ---- 6. sanity ----
def test_a_lens_changes_the_picture(R, renderer):
    scene, cam_like = V.chain_scene(R)
    renderer.upload(scene)
    cam = V.ring(R, cam_like, 32, 24, 1)[0]
    pin = renderer.render(cam)["avg"]
    assert same(renderer.render_lens(cam, R.Lens(2))["avg"], pin)  # two equal samples: (c + c) / 2 == c exactly
    thin = renderer.render_lens(cam, R.Lens(8, False, 0.3, 4.0, seed=1))["avg"]
    other = renderer.render_lens(cam, R.Lens(8, False, 0.3, 4.0, seed=2))["avg"]
    jit = renderer.render_lens(cam, R.Lens(8, True, seed=1))["avg"]
    assert np.all(np.isfinite(thin)) and np.all(np.isfinite(jit))
    assert np.abs(thin - pin).max() > 0.05 and np.abs(jit - pin).max() > 0.01
    assert not same(thin, other)
    assert same(thin, renderer.render_lens(cam, R.Lens(8, False, 0.3, 4.0, seed=1))["avg"])  # repeatable
    # blur: the thin-lens frame has less pixel-to-pixel contrast than the pinhole frame
    assert np.abs(np.diff(thin, axis=1)).mean() < np.abs(np.diff(pin, axis=1)).mean()
