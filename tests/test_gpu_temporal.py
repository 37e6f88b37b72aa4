"""Temporal accumulation on the GPU (rray.h RR_HAS_TEMPORAL): rr_temporal and rr_temporal_device against
rr_temporal_reference bit for bit over the case product of tests/temporal_cases.py (the host test's own list) and on
real first-hit planes with occlusion and indirect images, both lane maps, the device entry on a torch stream behind a
producer, three calls ping-ponging two histories, isolation from the frames' state, the refusals that need a context,
and the two end-to-end checks: accumulated occlusion planes come closer to the converged plane under a fixed camera and
along a small arc of cameras."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import temporal_cases as T  # noqa: E402
import test_gpu_ao as A  # noqa: E402  its ground scene
import test_gpu_lens as LN  # noqa: E402  its area-light scene
import test_gpu_rays as Q  # noqa: E402  its helpers: sync, SENT
import test_gpu_views_aov as V  # noqa: E402  its scenes, cameras and environment switch

pytestmark = pytest.mark.gpu
SENT = Q.SENT
KEYS = ("image", "depth", "normal", "object", "count", "m2")


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


def outputs(H, W, Cn, moments, dev):
    """(out, n, m2) device tensors, a sentinel behind each"""
    return (torch.full((H * W * Cn + 1,), SENT, dtype=torch.float64, device=dev),
            torch.full((H * W + 1,), -7, dtype=torch.int32, device=dev),
            torch.full((H * W * Cn + 1,), SENT, dtype=torch.float64, device=dev) if moments else None)


def fetch(o, shape, H, W):
    """the host result of device outputs, their sentinels checked"""
    out, n, m2 = (None if t is None else t.cpu().numpy() for t in o)
    assert out[-1] == SENT and n[-1] == -7 and (m2 is None or m2[-1] == SENT), "temporal_device wrote past an output"
    return {"out": out[:-1].reshape(shape), "n": n[:-1].reshape(H, W), "m2": None if m2 is None else m2[:-1].reshape(shape)}


def frames_of(args, kwargs):
    """host arrays of a case as the two rr_temporal_frame dicts"""
    img, _, _, _, depth = args
    prev = kwargs["prev"]
    cur = dict(image=img, depth=depth, normal=kwargs["normal"], object=kwargs["object"])
    hist = dict(image=prev["out"], depth=prev["depth"], normal=prev.get("normal"), object=prev.get("object"), count=prev["n"],
                m2=prev.get("m2") if kwargs["moments"] else None)
    return cur, hist


def temporal_dev(r, args, kwargs, dev, stream=None, cache=None):
    """rr_temporal_device over a case's host arrays; cache: id(host array) -> device tensor, shared between cases"""
    img, tp, cam, prev_cam, _ = args
    shape = np.shape(img)
    H, W = shape[:2]
    Cn = 1 if len(shape) == 2 else shape[2]
    cache = {} if cache is None else cache

    def put(a):
        if a is None:
            return None
        if id(a) not in cache:
            cache[id(a)] = (a, to_dev(a, dev))  # the array is kept so that its id stays its own
        return cache[id(a)][1].data_ptr()

    cur, hist = ({k: put(v) for k, v in f.items()} for f in frames_of(args, kwargs))
    o = outputs(H, W, Cn, kwargs["moments"], dev)
    Q.sync()
    r.temporal_device(tp, W, H, Cn, cam, prev_cam, cur, hist, o[0].data_ptr(), o[1].data_ptr(),
                      None if o[2] is None else o[2].data_ptr(), stream=stream)
    Q.sync()
    return fetch(o, shape, H, W)


def check_case(R, r, args, kwargs, dev, what, cache=None, host=True):
    want = R.temporal_reference(*args, **kwargs)
    got = temporal_dev(r, args, kwargs, dev, cache=cache)
    assert T.same_result(got, want), ("temporal_device",) + what
    if host:
        h = r.temporal(*args, **kwargs)
        assert h["out"].shape == np.shape(args[0]) and T.same_result(h, want), ("temporal",) + what
        for k in ("depth", "normal", "object"):  # a valid `prev` for the next call
            assert (h[k] is None) == (kwargs.get(k) is None and k != "depth")
    return want


# ---- 1. both entries against the reference ----
@pytest.mark.parametrize("W,H", T.FRAMES, ids=[f"{w}x{h}" for w, h in T.FRAMES])
def test_entries_equal_the_reference(R, renderer, dev, W, H):
    """Exact equality over the host test's whole product.  32 x 8 tiles: 1 x 1 is one lane, 7 x 5 part of a tile, 13 x 9
    crosses a tile's lower edge, 65 x 3 crosses a wave's run and two tile edges in x."""
    cache = {}
    for case in T.cases(W, H):
        args, kwargs = T.arguments(R, W, H, *case)
        want = check_case(R, renderer, args, kwargs, dev, (W, H) + case, cache)
        assert T.same_result(want, T.expected(W, H, *case))
    for _, t in cache.values():
        assert t[-1].item() in (SENT, -7)  # the inputs are left alone


@pytest.mark.parametrize("rows", ["0", "1"])
def test_both_lane_maps_equal_the_reference(R, dev, rows):
    """RRAY_TEMPORAL_ROWS=<0|1> (read at context creation) picks the 32 x 8 tile or the row-major map of 256 x 1 blocks.
    261 x 3 is wider than a row-major block and nine tiles wide; 13 x 9 and 65 x 3 have partial blocks under both."""
    with V.environment(RRAY_TEMPORAL_ROWS=rows):
        r = R.Renderer(0)
    try:
        for (W, H) in ((261, 3), (13, 9), (65, 3), (1, 1)):
            cache = {}
            for Cn in T.CHANNELS:
                for moments in T.MOMENTS:
                    for cam in T.CAMERAS:
                        case = (Cn, "all" if cam != "large" else "plane", moments, 0.2, 4, cam)
                        args, kwargs = T.arguments(R, W, H, *case)
                        check_case(R, r, args, kwargs, dev, (rows, W, H) + case, cache, host=False)
    finally:
        r.close()


# ---- 2. real planes ----
def _moved(R, cam, W, H, k=1):
    """the camera turned a little about its y axis and shifted, at W x H"""
    a = 0.02 * k
    rot = np.array([[math.cos(a), 0, math.sin(a), 0.05 * k], [0, 1, 0, -0.02 * k], [-math.sin(a), 0, math.cos(a), 0.01 * k],
                    [0, 0, 0, 1]])
    M = rot @ np.array(list(cam.transform), np.float64).reshape(4, 4)
    return R.camera(W, H, cam.field_of_view, [float(v) for v in M.reshape(-1)])


def _scenes(R):
    W, H = 41, 30
    flat, cam = V.flat_scene(R)
    yield "flat", flat, R.camera(W, H, cam.field_of_view, list(cam.transform)), True
    teapot = V.yaml_scene(R, "c4_teapot.yaml", W, H)
    yield "teapot", teapot, teapot.camera, False  # a mesh: every triangle is an object
    area, cam = LN.area_scene(R)
    yield "area", area, R.camera(W, H, cam.field_of_view, list(cam.transform)), True


def test_real_planes_with_occlusion_and_indirect_images(R, renderer, dev):
    """41 x 30 on the flat, teapot and area-light scenes: three frames along a small camera move, each an occlusion
    plane (C = 1) and an indirect plane (C = 3, moments on) accumulated over the previous one with render_aov's planes."""
    W, H = 41, 30
    for name, scene, cam0, by_object in _scenes(R):
        renderer.upload(scene)
        tp = R.Temporal(object=by_object)
        hist = {1: None, 3: None}
        prev_cam = cam0
        for k in range(3):
            cam = _moved(R, cam0, W, H, k)
            g = renderer.render_aov(cam, planes=("depth", "normal", "object"))
            imgs = {1: renderer.render_ao(cam, R.Ao(4, 1.0, seed=20 + k))["ao"],
                    3: renderer.render_indirect(cam, R.Indirect(4, 1, seed=30 + k), seed=k)["indirect"]}
            for Cn in (1, 3):
                args = (imgs[Cn], tp, cam, prev_cam, g["depth"])
                kwargs = dict(normal=g["normal"], object=g["object"], prev=hist[Cn], moments=Cn == 3)
                want = R.temporal_reference(*args, **kwargs)
                got = renderer.temporal(*args, **kwargs)
                assert T.same_result(got, want), (name, k, Cn)
                if hist[Cn] is not None:
                    assert T.same_result(temporal_dev(renderer, args, kwargs, dev), want), (name, k, Cn, "device")
                    hit = g["object"] >= 0
                    kept = (want["n"] > 1)[hit].mean()
                    print(f"{name} frame {k} C={Cn}: {int(hit.sum())} hits, reuse share {kept:.3f}")
                    assert kept > 0.25 and (want["n"][~hit] == 1).all()
                hist[Cn] = got
            prev_cam = cam


# ---- 3. the device entry on a stream ----
def test_device_entry_on_a_torch_stream_behind_a_producer(R, renderer, dev, oracle_mod):
    """render_aov_device and render_ao_device produce the frame on a torch stream, rr_temporal_device consumes it on
    that stream and a reduction consumes its output, with no synchronisation in between."""
    b, _, view = A.ground_scene(R, oracle_mod)
    renderer.upload(b)
    W, H = 48, 32
    cam0 = R.camera(W, H, math.pi / 3, view)
    cam1 = _moved(R, cam0, W, H)
    tp, ao = R.Temporal(), R.Ao(4, 1.0, seed=5)
    g0, g1 = (renderer.render_aov(c, planes=("depth", "normal", "object")) for c in (cam0, cam1))
    first = renderer.temporal(renderer.render_ao(cam0, ao)["ao"], tp, cam0, cam0, g0["depth"], normal=g0["normal"],
                              object=g0["object"])
    want = R.temporal_reference(renderer.render_ao(cam1, ao)["ao"], tp, cam1, cam0, g1["depth"], normal=g1["normal"],
                                object=g1["object"], prev=first)
    hist = {k: to_dev(v, dev) for k, v in dict(image=first["out"], depth=first["depth"], normal=first["normal"],
                                               object=first["object"], count=first["n"]).items()}
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        depth = torch.full((H * W + 1,), SENT, dtype=torch.float64, device=dev)
        normal = torch.full((H * W * 3 + 1,), SENT, dtype=torch.float64, device=dev)
        obj = torch.full((H * W + 1,), -7, dtype=torch.int32, device=dev)
        img = torch.full((H * W + 1,), SENT, dtype=torch.float64, device=dev)
        o = outputs(H, W, 1, False, dev)
        renderer.render_aov_device(cam1, opts, ("depth", "normal", "object"), d_depth=depth.data_ptr(),
                                   d_normal=normal.data_ptr(), d_object=obj.data_ptr(), stream=s.cuda_stream)
        renderer.render_ao_device(cam1, opts, ao, img.data_ptr(), stream=s.cuda_stream)
        cur = dict(image=img.data_ptr(), depth=depth.data_ptr(), normal=normal.data_ptr(), object=obj.data_ptr())
        renderer.temporal_device(tp, W, H, 1, cam1, cam0, cur, {k: v.data_ptr() for k, v in hist.items()}, o[0].data_ptr(),
                                 o[1].data_ptr(), stream=s.cuda_stream)
        total, longest = o[0][:-1].sum(), o[1][:-1].max()
    s.synchronize()
    got = fetch(o, (H, W), H, W)
    assert T.same_result(got, want) and (want["n"] == 2).mean() > 0.5
    assert int(longest) == 2 and abs(float(total) - want["out"].sum()) <= 1e-9 * want["out"].sum()
    assert depth[-1].item() == SENT and img[-1].item() == SENT and obj[-1].item() == -7


def test_three_calls_ping_ponging_two_histories(R, renderer, dev):
    """Two sets of history buffers on the device, each call reading one and writing the other, back to back on one
    stream: call k sees exactly call k - 1's outputs."""
    W, H, Cn = 65, 3, 3
    f = T.frame(W, H)
    tp = R.Temporal(max_history=8, alpha=0.0, sigma_plane=0.0, sigma_normal=0.0, object=False)
    cam, _ = T.cameras(R, W, H, "static")
    _, moved = T.cameras(R, W, H, "small")
    cams = (cam, moved, cam)
    rng = np.random.default_rng(3)
    imgs = [rng.random((H, W, Cn)) for _ in range(3)]
    depth = to_dev(f["depth"], dev)
    d_imgs = [to_dev(a, dev) for a in imgs]
    sets = [outputs(H, W, Cn, True, dev) for _ in range(2)]
    zero = (torch.zeros(H * W * Cn, dtype=torch.float64, device=dev), torch.zeros(H * W, dtype=torch.int32, device=dev),
            torch.zeros(H * W * Cn, dtype=torch.float64, device=dev))
    Q.sync()
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        for k in range(3):
            src = zero if k == 0 else sets[(k - 1) & 1]
            dst = sets[k & 1]
            renderer.temporal_device(tp, W, H, Cn, cams[k], cams[k - 1] if k else cams[0],
                                     dict(image=d_imgs[k].data_ptr(), depth=depth.data_ptr()),
                                     dict(image=src[0].data_ptr(), depth=depth.data_ptr(), count=src[1].data_ptr(),
                                          m2=src[2].data_ptr()),
                                     dst[0].data_ptr(), dst[1].data_ptr(), dst[2].data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    hist = None
    for k in range(3):
        hist = R.temporal_reference(imgs[k], tp, cams[k], cams[k - 1] if k else cams[0], f["depth"], prev=hist, moments=True)
        if k == 1:
            second = hist
    assert T.same_result(fetch(sets[0], (H, W, Cn), H, W), hist) and hist["n"].max() == 3
    assert T.same_result(fetch(sets[1], (H, W, Cn), H, W), second) and second["n"].max() == 2


# ---- 4. isolation ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_temporal_leaves_frames_and_stats_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        scene = V.yaml_scene(R, "c4_teapot.yaml", 64, 32)
        r.upload(scene)
        args, kwargs = T.arguments(R, 13, 9, 3, "all", True, 0.0, 4, "small")
        before = r.render(scene.camera, max_depth=5)
        launch = r.resident_launch()
        st = r.last_stats()
        temporal_dev(r, args, kwargs, dev)
        r.temporal(*args, **kwargs)
        assert r.last_stats() == st and r.resident_launch() == launch
        after = r.render(scene.camera, max_depth=5)
        assert Q.same(before["avg"], after["avg"])
        assert _without_time(before["stats"]) == _without_time(after["stats"])
    finally:
        r.close()


# ---- 5. refusals ----
def test_refusals_that_need_a_context(R, renderer, dev):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    args, kwargs = T.arguments(R, W, H, 3, "all", True, 0.0, 4, "small")
    cur_h, prev_h = frames_of(args, kwargs)
    cam, pcam = args[2], args[3]
    keep = [to_dev(v, dev) for f in (cur_h, prev_h) for v in f.values() if v is not None]
    it = iter(keep)
    cur_d = {k: (None if v is None else next(it)) for k, v in cur_h.items()}
    prev_d = {k: (None if v is None else next(it)) for k, v in prev_h.items()}
    o = outputs(H, W, 3, True, dev)
    ho = (np.full((H, W, 3), SENT), np.full((H, W), -7, np.int32), np.full((H, W, 3), SENT))
    Q.sync()

    def err():
        return L.rr_last_error().decode()

    def desc(**kw):
        fields = dict(flags=1, max_history=4, alpha=0.0, sigma_plane=0.004, sigma_normal=0.02)
        fields.update(kw)
        return E.TemporalDesc(*fields.values())

    def frame(d, host, skip):
        ptr = (lambda a: C.c_void_p(a.ctypes.data)) if host else (lambda t: C.c_void_p(t.data_ptr()))
        return E.TemporalFrame(*[None if d.get(k) is None or k in skip else ptr(d[k]) for k in KEYS])

    def call(d=None, ctx=renderer.h, w=W, hh=H, c=3, skip=(), pskip=(), outs=None, m2=True, cams=(cam, pcam)):
        """(device entry, host entry) return codes"""
        d = d or desc()
        od = outs[0] if outs else [C.c_void_p(t.data_ptr()) for t in o]
        oh = outs[1] if outs else [C.c_void_p(a.ctypes.data) for a in ho]
        if not m2:
            od, oh = od[:2] + [None], oh[:2] + [None]
        res = []
        for host, dd in ((False, (cur_d, prev_d, od)), (True, (cur_h, prev_h, oh))):
            fc, fp = frame(dd[0], host, skip), frame(dd[1], host, pskip)
            common = (ctx, C.byref(d), w, hh, c, C.byref(cams[0]), C.byref(fc), C.byref(cams[1]), C.byref(fp), *dd[2])
            res.append(L.rr_temporal(*common) if host else L.rr_temporal_device(*common, None))
        return tuple(res)

    assert call(ctx=None) == (ARG, ARG)
    for c in (0, 2, 4):
        assert call(c=c) == (ARG, ARG)
    for w, hh in ((0, 5), (7, 0), (-1, 5)):
        assert call(w=w, hh=hh) == (ARG, ARG)
    other = R.camera(W, H + 1, T.FOV, T.BASE)
    assert call(cams=(other, pcam)) == (ARG, ARG) and call(cams=(cam, other)) == (ARG, ARG) and "camera" in err()
    for kw in (dict(flags=2), dict(max_history=0), dict(max_history=2**20 + 1), dict(alpha=-0.1), dict(alpha=math.nan),
               dict(sigma_plane=-1.0), dict(sigma_normal=math.inf)):
        assert call(desc(**kw)) == (ARG, ARG), kw
    for k in ("image", "depth"):
        assert call(skip=(k,)) == (ARG, ARG) and call(pskip=(k,)) == (ARG, ARG) and "required" in err()
    assert call(pskip=("count",)) == (ARG, ARG)
    assert call(skip=("normal",)) == (ARG, ARG) and "planes" in err() and call(pskip=("object",)) == (ARG, ARG)
    assert call(desc(flags=0, sigma_normal=0.0), pskip=("object", "normal")) == (0, 0)
    assert call(m2=False) == (ARG, ARG) and "m2" in err() and call(pskip=("m2",)) == (ARG, ARG)
    assert call(m2=False, pskip=("m2",)) == (0, 0)
    # an output overlapping an input
    inside = ([C.c_void_p(prev_d["normal"].data_ptr() + 64)] + [C.c_void_p(t.data_ptr()) for t in o[1:]],
              [C.c_void_p(prev_h["normal"].ctypes.data + 64)] + [C.c_void_p(a.ctypes.data) for a in ho[1:]])
    assert call(outs=inside) == (ARG, ARG) and "overlap" in err()
    big = (R.camera(2**16, 2**15, T.FOV, T.BASE),) * 2
    assert call(w=2**16, hh=2**15, cams=big) == (LIM, LIM) and "2^31" in err()
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
    for a in ho:
        a[...] = -7 if a.dtype == np.int32 else SENT
    assert call() == (0, 0)
    Q.sync()
    want = R.temporal_reference(*args, **kwargs)
    assert T.same_result(fetch(o, (H, W, 3), H, W), want)
    assert T.same_result({"out": ho[0], "n": ho[1], "m2": ho[2]}, want)


# ---- 6. end to end ----
def test_accumulating_under_a_fixed_camera_approaches_the_converged_plane(R, renderer, oracle_mod):
    """48 x 32 of test_gpu_ao.py's ground scene: eight K = 4 occlusion planes with seeds 0..7, accumulated under a fixed
    camera.  The mean of eight independent K = 4 estimates is a K = 32 estimate, so the expected squared-error ratio
    against the K = 1024 plane is 1/8; asserted below 0.5 of one frame's."""
    b, _, view = A.ground_scene(R, oracle_mod)
    renderer.upload(b)
    cam = R.camera(48, 32, math.pi / 3, view)
    g = renderer.render_aov(cam, planes=("depth", "normal", "object"))
    ref = renderer.render_ao(cam, R.Ao(1024, 1.0, seed=99))["ao"]
    hit = g["object"] >= 0
    assert 200 < hit.sum() < 48 * 32
    tp = R.Temporal()
    hist, frames = None, []
    for seed in range(8):
        frames.append(renderer.render_ao(cam, R.Ao(4, 1.0, seed=seed))["ao"])
        hist = renderer.temporal(frames[-1], tp, cam, cam, g["depth"], normal=g["normal"], object=g["object"], prev=hist,
                                 moments=True)
    assert (hist["n"][hit] == 8).all() and (hist["n"][~hit] == 1).all()
    one = float(((frames[-1] - ref)[hit] ** 2).sum())
    acc = float(((hist["out"] - ref)[hit] ** 2).sum())
    print(f"static camera, eight K = 4 occlusion planes against K = 1024 over {int(hit.sum())} hits: squared error "
          f"{one:.4g} one frame, {acc:.4g} accumulated: ratio {acc / one:.4f} (expected 1/8)")
    assert acc < 0.5 * one
    # the accumulated image is the running mean, and the moments give the frames' variance
    mean = np.mean(frames, axis=0)
    assert np.abs(hist["out"] - mean)[hit].max() < 1e-12
    var = R.temporal_variance(hist["out"], hist["m2"])
    assert np.abs(var - np.var(frames, axis=0))[hit].max() < 1e-12


def test_accumulating_along_a_small_arc_lowers_the_error(R, renderer, oracle_mod):
    """Four cameras on a small arc around the ground scene, a K = 4 occlusion plane each: the accumulated error at the
    last camera is below that frame's own."""
    b, _, view = A.ground_scene(R, oracle_mod)
    renderer.upload(b)
    W, H = 48, 32
    cam0 = R.camera(W, H, math.pi / 3, view)
    tp = R.Temporal()
    hist, prev_cam = None, cam0
    for k in range(4):
        cam = _moved(R, cam0, W, H, k)
        g = renderer.render_aov(cam, planes=("depth", "normal", "object"))
        raw = renderer.render_ao(cam, R.Ao(4, 1.0, seed=40 + k))["ao"]
        hist = renderer.temporal(raw, tp, cam, prev_cam, g["depth"], normal=g["normal"], object=g["object"], prev=hist)
        prev_cam = cam
    ref = renderer.render_ao(cam, R.Ao(1024, 1.0, seed=98))["ao"]
    hit = g["object"] >= 0
    one = float(((raw - ref)[hit] ** 2).sum())
    acc = float(((hist["out"] - ref)[hit] ** 2).sum())
    share = float((hist["n"] > 1)[hit].mean())
    print(f"four cameras on an arc, K = 4 occlusion planes against K = 1024 over {int(hit.sum())} hits: squared error "
          f"{one:.4g} last frame, {acc:.4g} accumulated: ratio {acc / one:.4f}; reuse share {share:.3f}, "
          f"mean history {hist['n'][hit].mean():.2f}")
    assert acc < one
