"""The edge-avoiding denoiser on the GPU (rray.h RR_HAS_DENOISE): rr_denoise_device and rr_denoise
against the numpy mirror rray_amd.denoise_filter bit for bit over the frames, channel counts, level counts and term
combinations of tests/denoise_cases.py (the host test's own list), the device entry on a torch stream, isolation from
the frames' state, the refusals that need a context, and the two end-to-end checks: a K = 4 occlusion plane and an
S = 2 lens frame come closer to their converged planes when filtered."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import denoise_cases as D  # noqa: E402
import test_gpu_ao as A  # noqa: E402  its ground scene
import test_gpu_lens as LN  # noqa: E402  its area-light scene
import test_gpu_rays as Q  # noqa: E402  its helpers: sync, SENT
import test_gpu_views_aov as V  # noqa: E402  its scenes and cameras

pytestmark = pytest.mark.gpu
SENT = Q.SENT
PLANES = ("depth", "normal", "object", "albedo")


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


def to_dev(a, dev):
    """a host array as a flat device tensor of its own type with one sentinel element behind it"""
    a = np.ascontiguousarray(a)
    flat = np.concatenate([a.reshape(-1), np.array([-7 if a.dtype == np.int32 else SENT], a.dtype)])
    return torch.from_numpy(flat).to(dev)


def denoise_dev(r, dn, img, planes, dev, stream=None, tensors=None):
    """rr_denoise_device over host arrays (or their device tensors), the output with a sentinel behind it"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    Cn = 1 if img.ndim == 2 else img.shape[2]
    t = tensors or {k: to_dev(v, dev) for k, v in dict(planes, img=img).items()}
    out = torch.full((H * W * Cn + 1,), SENT, dtype=torch.float64, device=dev)
    Q.sync()
    r.denoise_device(dn, W, H, Cn, t["img"].data_ptr(), out.data_ptr(), stream=stream,
                     **{"d_" + k: t[k].data_ptr() for k in planes})
    Q.sync()
    a = out.cpu().numpy()
    assert a[-1] == SENT, "denoise_device wrote past its image"
    return a[:-1].reshape(img.shape)


# ---- 1. both entries against the mirror ----
@pytest.mark.parametrize("W,H", D.FRAMES, ids=[f"{w}x{h}" for w, h in D.FRAMES])
def test_entries_equal_the_filter(R, renderer, dev, W, H):
    """Exact equality.  32 x 8 tiles: 65 x 1 and 1 x 65 have a partial last tile and a partial last wave, 64 x 4 whole
    tiles' width and half a tile's height, 70 x 37 several tiles in both directions with partial ones at both edges;
    iterations = 6 reaches holes of 32 pixels, wider than every frame but 65 x 1, 64 x 4 and 70 x 37."""
    f = D.frame(W, H)
    tensors = {k: to_dev(f[k], dev) for k in PLANES}
    imgs = {1: to_dev(f["img1"], dev), 3: to_dev(f["img3"], dev)}
    n = 0
    for (w, h, Cn, I, name) in D.cases():
        if (w, h) != (W, H):
            continue
        img, dn, planes = D.arguments(R, W, H, Cn, I, name)
        want = D.expected(W, H, Cn, I, name)
        got = denoise_dev(renderer, dn, img, planes, dev, tensors=dict(tensors, img=imgs[Cn]))
        assert D.same_bits(got, want), ("denoise_device", W, H, Cn, I, name, float(np.nanmax(np.abs(got - want))))
        host = renderer.denoise(img, dn, **planes)
        assert host.shape == img.shape and D.same_bits(host, want), ("denoise", W, H, Cn, I, name)
        n += 1
    assert n == len(D.CHANNELS) * len(D.ITERATIONS) * len(D.COMBOS)
    for t in list(tensors.values()) + list(imgs.values()):
        assert t[-1].item() in (SENT, -7)  # the inputs are left alone


@pytest.mark.parametrize("lds", ["0", "1", "2"])
def test_the_lds_tiled_levels_equal_the_filter(R, dev, lds):
    """RRAY_DENOISE_LDS=<pixels> (read at context creation) runs the levels with holes up to that size in the LDS-tiled
    kernel and the wider ones in the direct kernel: with 0 every level is direct, with 1 the hand-over lies behind level
    0, with 2 behind level 1 (the default context takes 2 for one channel and 1 for three).
    70 x 37 is more than one 32 x 8 tile in both directions with partial tiles at both edges, so halos lie inside
    the frame, across its border and (65 x 1, 1 x 65, 3 x 2) wholly outside it."""
    with V.environment(RRAY_DENOISE_LDS=lds):
        r = R.Renderer(0)
    try:
        for (W, H) in ((70, 37), (65, 1), (1, 65), (3, 2), (64, 4)):
            f = D.frame(W, H)
            tensors = {k: to_dev(f[k], dev) for k in PLANES}
            for Cn in D.CHANNELS:
                tensors["img"] = to_dev(f["img1" if Cn == 1 else "img3"], dev)
                for I in D.ITERATIONS:
                    for name in ("all", "none", "colour"):
                        img, dn, planes = D.arguments(R, W, H, Cn, I, name)
                        got = denoise_dev(r, dn, img, planes, dev, tensors=tensors)
                        assert D.same_bits(got, D.expected(W, H, Cn, I, name)), (lds, W, H, Cn, I, name)
    finally:
        r.close()


def test_nan_colours_and_denormal_guides(R, renderer, dev):
    f = D.frame(13, 5)
    img = f["img1"].copy()
    img[2, 6] = math.nan
    stays = R.Denoise(2, sigma_color=0.5, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    spreads = R.Denoise(2, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    for dn in (stays, spreads):
        want = R.denoise_filter(img, dn)
        assert D.same_bits(denoise_dev(renderer, dn, img, {}, dev), want) and D.same_bits(renderer.denoise(img, dn), want)
    assert np.isnan(R.denoise_filter(img, stays)).sum() == 1 and np.isnan(R.denoise_filter(img, spreads)).sum() > 9
    # guides below the smallest normal float stay denormal floats, on the device as in numpy
    depth, albedo = f["depth"] * 1e-40, f["albedo"] * 1e-41
    dn = R.Denoise(2, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.05, sigma_albedo=1e-41)
    planes = dict(depth=depth, albedo=albedo)
    want = R.denoise_filter(f["img3"], dn, **planes)
    assert not D.same_bits(want, R.denoise_filter(f["img3"], R.Denoise(2, 0.0, 0.0, 0.0, 0.0)))  # the terms cut taps
    assert D.same_bits(denoise_dev(renderer, dn, f["img3"], planes, dev), want)


# ---- 2. the device entry on a stream ----
def test_device_entry_on_a_torch_stream(R, renderer, dev):
    """Two calls with different parameters (and channel counts) back to back on one torch stream, consumed on that
    stream with no synchronisation in between: each gives its own exact result, so the second call's use of the
    scratch images and records is ordered behind the first call's."""
    W, H = 70, 37
    f = D.frame(W, H)
    a = D.arguments(R, W, H, 3, 6, "all")
    b = D.arguments(R, W, H, 1, 2, "normal")
    denoise_dev(renderer, a[1], a[0], a[2], dev)  # the scratch has its size before the stream's calls
    t = {k: to_dev(f[k], dev) for k in PLANES + ("img1", "img3")}
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        out_a = torch.full((H * W * 3 + 1,), SENT, dtype=torch.float64, device=dev)
        out_b = torch.full((H * W + 1,), SENT, dtype=torch.float64, device=dev)
        renderer.denoise_device(a[1], W, H, 3, t["img3"].data_ptr(), out_a.data_ptr(), stream=s.cuda_stream,
                                **{"d_" + k: t[k].data_ptr() for k in a[2]})
        renderer.denoise_device(b[1], W, H, 1, t["img1"].data_ptr(), out_b.data_ptr(), stream=s.cuda_stream,
                                **{"d_" + k: t[k].data_ptr() for k in b[2]})
        # a call that feeds on the first one's output, as a pipeline would
        out_c = torch.full((H * W * 3 + 1,), SENT, dtype=torch.float64, device=dev)
        renderer.denoise_device(a[1], W, H, 3, out_a.data_ptr(), out_c.data_ptr(), stream=s.cuda_stream,
                                **{"d_" + k: t[k].data_ptr() for k in a[2]})
        largest = out_b[:-1].max()
    s.synchronize()
    want_a, want_b = D.expected(W, H, 3, 6, "all"), D.expected(W, H, 1, 2, "normal")
    ga, gb, gc = out_a.cpu().numpy(), out_b.cpu().numpy(), out_c.cpu().numpy()
    assert ga[-1] == SENT and gb[-1] == SENT and gc[-1] == SENT
    assert D.same_bits(ga[:-1].reshape(H, W, 3), want_a) and D.same_bits(gb[:-1].reshape(H, W), want_b)
    assert float(largest) == float(want_b.max())
    assert D.same_bits(gc[:-1].reshape(H, W, 3), R.denoise_filter(want_a, a[1], **a[2]))


# ---- 3. isolation ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_denoise_leaves_frames_and_stats_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        scene = V.yaml_scene(R, "c4_teapot.yaml", 64, 32)
        r.upload(scene)
        img, dn, planes = D.arguments(R, 70, 37, 3, 2, "all")
        before = r.render(scene.camera, max_depth=5)
        launch = r.resident_launch()
        st = r.last_stats()
        denoise_dev(r, dn, img, planes, dev)
        r.denoise(img, dn, **planes)
        assert r.last_stats() == st and r.resident_launch() == launch
        after = r.render(scene.camera, max_depth=5)
        assert Q.same(before["avg"], after["avg"])
        assert _without_time(before["stats"]) == _without_time(after["stats"])
    finally:
        r.close()


# ---- 4. refusals ----
def test_refusals_that_need_a_context(R, renderer, dev):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    f = D.frame(W, H)
    t = {k: to_dev(f[k], dev) for k in PLANES + ("img3",)}
    out = torch.full((W * H * 3 + 1,), SENT, dtype=torch.float64, device=dev)
    host_out = np.full((H, W, 3), SENT)
    Q.sync()
    h = renderer.h
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    hp = {k: f[k].ctypes.data_as(E._I if k == "object" else E._D) for k in PLANES + ("img3",)}

    def err():
        return L.rr_last_error().decode()

    def desc(**kw):
        fields = dict(iterations=2, flags=1, sigma_color=0.5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
        fields.update(kw)
        return C.byref(E.DenoiseDesc(*fields.values()))

    def call(d=None, ctx=h, w=W, hh=H, c=3, skip=(), src="img3", dst=None, nodesc=False):
        """(device entry, host entry) return codes"""
        d = None if nodesc else (d or desc())
        dp = [None if k in skip else ptr[k] for k in PLANES]
        pp = [None if k in skip else hp[k] for k in PLANES]
        o_dev = C.c_void_p(out.data_ptr()) if dst is None else dst[0]
        o_host = host_out.ctypes.data_as(E._D) if dst is None else dst[1]
        return (L.rr_denoise_device(ctx, d, w, hh, c, ptr[src] if src else None, *dp, o_dev, None),
                L.rr_denoise(ctx, d, w, hh, c, hp[src] if src else None, *pp, o_host))

    assert call(ctx=None) == (ARG, ARG) and call(nodesc=True) == (ARG, ARG) and call(src=None) == (ARG, ARG)
    assert call(dst=(None, None)) == (ARG, ARG)
    for c in (0, 2, 4):
        assert call(c=c) == (ARG, ARG)
    for w, hh in ((0, 5), (7, 0), (-1, 5)):
        assert call(w=w, hh=hh) == (ARG, ARG)
    for kw in (dict(iterations=0), dict(iterations=E.RR_MAX_DENOISE_ITERATIONS + 1), dict(flags=2), dict(flags=-1),
               dict(sigma_color=-1.0), dict(sigma_normal=math.nan), dict(sigma_depth=math.inf), dict(sigma_albedo=-0.5)):
        assert call(desc(**kw)) == (ARG, ARG), kw
    # a term that is on needs its plane; with the term off the plane may go
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert call(skip=(k,)) == (ARG, ARG) and "plane" in err(), k
        assert call(desc(**off), skip=(k,)) == (0, 0), k
    # out overlapping an input
    assert call(dst=(ptr["img3"], hp["img3"])) == (ARG, ARG) and "overlap" in err()
    inside = (C.c_void_p(t["normal"].data_ptr() + 64), C.cast(C.c_void_p(f["normal"].ctypes.data + 64), E._D))
    assert call(dst=inside) == (ARG, ARG) and "overlap" in err()
    assert call(w=2**16, hh=2**15) == (LIM, LIM) and "2^31" in err()
    # a virtual (multi-device) context
    v = R.Renderer.virtual(0, 2)
    try:
        assert call(ctx=v.h) == (ARG, ARG) and "single-device" in err()
    finally:
        v.close()
    # no scene is needed, and the calls serve after the refusals
    fresh = R.Renderer(0)
    try:
        assert call(ctx=fresh.h) == (0, 0)
    finally:
        fresh.close()
    assert call() == (0, 0)
    Q.sync()
    want = R.denoise_filter(f["img3"], R.Denoise(2, 0.5, 0.25, 0.05, 0.1, object=True), **{k: f[k] for k in PLANES})
    got = out.cpu().numpy()
    assert got[-1] == SENT and D.same_bits(got[:-1].reshape(H, W, 3), want) and D.same_bits(host_out, want)


# ---- 5. end to end ----
def _ratio(filtered, raw, ref, mask):
    e1, e0 = (filtered - ref)[mask], (raw - ref)[mask]
    return float((e1 * e1).mean() / (e0 * e0).mean())


def test_a_noisy_occlusion_plane_comes_closer_to_the_converged_one(R, renderer, oracle_mod):
    """48 x 32 of test_gpu_ao.py's plane + sphere + cube scene: the K = 4 plane, filtered with the same camera's
    first-hit planes, against the K = 1024 plane over the samples that hit.  Measured on an MI355X: see DESIGN.md §3.22."""
    b, _, view = A.ground_scene(R, oracle_mod)
    renderer.upload(b)
    cam = R.camera(48, 32, math.pi / 3, view)
    raw = renderer.render_ao(cam, R.Ao(4, 1.0, seed=11))["ao"]
    ref = renderer.render_ao(cam, R.Ao(1024, 1.0, seed=12))["ao"]
    g = renderer.render_aov(cam)
    hit = g["object"] >= 0
    assert 200 < hit.sum() < 48 * 32  # some sky: a miss region
    for I in (1, 3, 5):
        dn = R.Denoise(I, object=True)
        out = renderer.denoise(raw, dn, **{k: g[k] for k in PLANES})
        assert D.same_bits(out, R.denoise_filter(raw, dn, **{k: g[k] for k in PLANES}))
        ratio = _ratio(out, raw, ref, hit)
        print(f"denoise AO 48x32 K=4 against K=1024, iterations {I}: mse ratio {ratio:.4f}")
        assert ratio < 1.0
        assert D.same_bits(out[~hit], raw[~hit])  # the sky is void


def test_a_noisy_lens_frame_comes_closer_to_the_converged_one(R, renderer):
    """48 x 32 of test_gpu_lens.py's area-light scene: S = 2 with pixel jitter, filtered with the pinhole camera's
    first-hit planes, against S = 512 over the pixels that hit."""
    b, _ = LN.area_scene(R)
    renderer.upload(b)
    cam = R.camera(48, 32, math.pi / 3, V.translate(0, -0.5, 0))  # area_scene's camera at 48 x 32
    raw = renderer.render_lens(cam, R.Lens(2, pixel_jitter=True, seed=3), max_depth=5, seed=7, jitter_mode=0)["avg"]
    ref = renderer.render_lens(cam, R.Lens(512, pixel_jitter=True, seed=4), max_depth=5, seed=8, jitter_mode=0)["avg"]
    g = renderer.render_aov(cam)
    hit = g["object"] >= 0
    assert 200 < hit.sum() < 48 * 32
    for I in (1, 2, 3):
        dn = R.Denoise(I, sigma_color=0.5, object=True)
        out = renderer.denoise(raw, dn, **{k: g[k] for k in PLANES})
        assert D.same_bits(out, R.denoise_filter(raw, dn, **{k: g[k] for k in PLANES}))
        ratio = _ratio(out, raw, ref, hit)
        print(f"denoise lens 48x32 S=2 against S=512, iterations {I}: mse ratio {ratio:.4f}")
        assert ratio < 1.0
