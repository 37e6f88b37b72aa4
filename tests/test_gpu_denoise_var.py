"""Variance-guided denoising on the GPU (rray.h RR_HAS_DENOISE_VAR): rr_variance, rr_variance_device,
rr_denoise_var and rr_denoise_var_device against the numpy mirrors rray_amd.variance_estimate and
rray_amd.denoise_var_filter bit for bit over the cases of tests/denoise_var_cases.py (the host test's own list), the
chain temporal -> variance -> denoise_var on a torch stream, isolation from the frames' state, the refusals that need a
context, the shared scratch left fit for rr_denoise_device, and the end-to-end checks on accumulated occlusion planes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import denoise_cases as D  # noqa: E402
import denoise_var_cases as V  # noqa: E402
import test_gpu_ao as A  # noqa: E402  its ground scene
import test_gpu_rays as Q  # noqa: E402  its helpers: sync, SENT
import test_gpu_views_aov as VA  # noqa: E402  its scenes

pytestmark = pytest.mark.gpu
SENT = Q.SENT
PLANES = ("depth", "normal", "object", "albedo")
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


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


def blank(n, dev):
    return torch.full((n + 1,), SENT, dtype=torch.float64, device=dev)


def fetch(t, shape):
    a = t.cpu().numpy()
    assert a[-1] == SENT, "an entry wrote past its buffer"
    return a[:-1].reshape(shape)


def variance_dev(r, vr, W, H, Cn, t, given, history, dev, stream=None):
    """rr_variance_device over the device tensors `t` -> the (H, W) plane"""
    var = blank(H * W, dev)
    Q.sync()
    kw = {"d_" + k: t[k].data_ptr() for k in given}
    if history:
        kw.update(d_m2=t[f"m2_{Cn}"].data_ptr(), d_count=t["count"].data_ptr())
    r.variance_device(vr, W, H, Cn, t[f"img{Cn}"].data_ptr(), var.data_ptr(), stream=stream, **kw)
    Q.sync()
    return fetch(var, (H, W))


def filter_dev(r, dv, W, H, Cn, t, given, dev, with_var=True, stream=None):
    """rr_denoise_var_device over the device tensors `t` -> (image, variance plane or None)"""
    out, vout = blank(H * W * Cn, dev), blank(H * W, dev)
    Q.sync()
    r.denoise_var_device(dv, W, H, Cn, t[f"img{Cn}"].data_ptr(), t["var"].data_ptr(), out.data_ptr(),
                         vout.data_ptr() if with_var else None, stream=stream, **{"d_" + k: t[k].data_ptr() for k in given})
    Q.sync()
    v = fetch(vout, (H, W))
    if not with_var:
        assert (v == SENT).all(), "var_out was NULL"
    return fetch(out, (H, W) if Cn == 1 else (H, W, Cn)), v if with_var else None


# ---- 1. the four entries against the mirrors ----
@pytest.mark.parametrize("W,H", V.FRAMES, ids=[f"{w}x{h}" for w, h in V.FRAMES])
def test_entries_equal_the_mirrors(R, renderer, dev, W, H):
    """Exact equality.  32 x 8 tiles: 65 x 1 and 1 x 65 have a partial last tile and a partial last wave, 33 x 9 one pixel
    past a tile on both axes, 70 x 37 several tiles with partial ones at both edges; 7 x 5 is smaller than the variance
    window on one axis; iterations = 1 uses no scratch, 6 reaches holes of 32 pixels."""
    f = V.frame(W, H)
    keys = PLANES + ("img1", "img3", "m2_1", "m2_3", "count", "var")
    t = {k: to_dev(f[k], dev) for k in keys}
    n = 0
    for case in V.variance_cases():
        if case[:2] != (W, H):
            continue
        _, _, Cn, g, h = case
        img, vr, args = V.variance_arguments(R, *case)
        want = V.variance_expected(*case)
        got = variance_dev(renderer, vr, W, H, Cn, t, V.GUIDES[g][1], h != "absent", dev)
        assert V.same_bits(got, want), ("variance_device", case)
        assert V.same_bits(renderer.variance(img, vr, **args), want), ("variance", case)
        n += 1
    assert n == 42
    n = 0
    for case in V.filter_cases():
        if case[:2] != (W, H):
            continue
        _, _, Cn, I, g, c = case
        img, var, dv, planes = V.filter_arguments(R, *case)
        want, want_v = V.filter_expected(*case)
        got, got_v = filter_dev(renderer, dv, W, H, Cn, t, V.GUIDES[g][1], dev)
        assert V.same_bits(got, want) and V.same_bits(got_v, want_v), ("denoise_var_device", case)
        got, _ = filter_dev(renderer, dv, W, H, Cn, t, V.GUIDES[g][1], dev, with_var=False)
        assert V.same_bits(got, want), ("denoise_var_device without var_out", case)
        host, host_v = renderer.denoise_var(img, var, dv, return_var=True, **planes)
        assert host.shape == img.shape and V.same_bits(host, want) and V.same_bits(host_v, want_v), ("denoise_var", case)
        if I == 2:
            assert V.same_bits(renderer.denoise_var(img, var, dv, **planes), want), ("denoise_var without var_out", case)
        n += 1
    assert n == 84
    for k, v in t.items():
        assert v[-1].item() in (SENT, -7), k  # the inputs are left alone


# ---- 2. the chain on a stream ----
def _chain_host(R, imgs, tp, vr, dv, cam, g):
    hist = None
    for img in imgs:
        hist = R.temporal_filter(img, tp, cam, cam, g["depth"], normal=g["normal"], object=g["object"], prev=hist, moments=True)
    var = R.variance_estimate(hist["out"], vr, m2=hist["m2"], count=hist["n"], **g)
    out, vout = R.denoise_var_filter(hist["out"], var, dv, return_var=True, **g)
    return hist, var, out, vout


def _chain_dev(R, r, imgs, tp, vr, dv, cam, g, W, H, Cn, dev, s):
    """On the current stream `s`: torch kernels produce the frames, two rr_temporal_device calls accumulate them,
    rr_variance_device and rr_denoise_var_device follow, and a reduction consumes the result; nothing synchronises."""
    n = H * W
    host = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).pin_memory() for a in imgs]
    planes = {k: to_dev(g[k], dev) for k in g}
    zero = (torch.zeros(n * Cn, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
            torch.zeros(n * Cn, dtype=torch.float64, device=dev))
    sets = [(blank(n * Cn, dev), torch.full((n + 1,), -7, dtype=torch.int32, device=dev), blank(n * Cn, dev)) for _ in imgs]
    var, out, vout = blank(n, dev), blank(n * Cn, dev), blank(n, dev)
    gp = {k: v.data_ptr() for k, v in planes.items()}
    src = zero
    for k, h in enumerate(host):
        frame = h.to(dev, non_blocking=True) * 1.0  # the producer: a copy and a kernel on this stream
        cur = dict(image=frame.data_ptr(), depth=gp["depth"], normal=gp["normal"], object=gp["object"])
        prev = dict(image=src[0].data_ptr(), depth=gp["depth"], normal=gp["normal"], object=gp["object"],
                    count=src[1].data_ptr(), m2=src[2].data_ptr())
        r.temporal_device(tp, W, H, Cn, cam, cam, cur, prev, sets[k][0].data_ptr(), sets[k][1].data_ptr(),
                          sets[k][2].data_ptr(), stream=s.cuda_stream)
        src = sets[k]
    kw = {"d_" + k: gp[k] for k in gp}
    r.variance_device(vr, W, H, Cn, src[0].data_ptr(), var.data_ptr(), d_m2=src[2].data_ptr(), d_count=src[1].data_ptr(),
                      stream=s.cuda_stream, **kw)
    r.denoise_var_device(dv, W, H, Cn, src[0].data_ptr(), var.data_ptr(), out.data_ptr(), vout.data_ptr(),
                         stream=s.cuda_stream, **kw)
    total = torch.nan_to_num(out[:-1]).sum()  # the consumer
    return dict(hist=src, var=var, out=out, vout=vout, total=total, keep=(host, planes, zero, sets))


def _chain_check(R, got, want, shape, H, W):
    hist, var, out, vout = want
    assert V.same_bits(fetch(got["hist"][0], shape), hist["out"]) and V.same_bits(fetch(got["hist"][2], shape), hist["m2"])
    assert np.array_equal(got["hist"][1].cpu().numpy()[:-1].reshape(H, W), hist["n"])
    assert V.same_bits(fetch(got["var"], (H, W)), var)
    assert V.same_bits(fetch(got["out"], shape), out) and V.same_bits(fetch(got["vout"], (H, W)), vout)
    assert abs(float(got["total"]) - np.nan_to_num(out).sum()) <= 1e-9 * np.abs(np.nan_to_num(out)).sum()


def test_the_chain_on_a_torch_stream_and_a_scratch_that_grows_mid_stream(R, dev):
    """temporal_device -> variance_device -> denoise_var_device -> a reduction, back to back on one torch stream behind
    torch producers, against the same chain in numpy; first on 33 x 9, then — in the same context and on the same stream,
    with nothing synchronised in between — on 70 x 37, so the records, images and variance planes grow while the first
    chain may still be running."""
    r = R.Renderer(0)  # a fresh context: its scratch starts empty
    try:
        tp = R.Temporal(max_history=8, alpha=0.0, sigma_plane=0.0, sigma_normal=0.0, object=False)
        vr = R.Variance(min_history=2, object=True)
        dv = R.DenoiseVar(3, object=True, sigma_albedo=0.0)
        rng = np.random.default_rng(17)
        runs = []
        for (W, H, Cn) in ((33, 9, 3), (70, 37, 1)):
            f = D.frame(W, H)
            g = {k: f[k] for k in ("depth", "normal", "object")}
            shape = (H, W) if Cn == 1 else (H, W, Cn)
            imgs = [0.5 + 0.3 * rng.random(shape) for _ in range(2)]
            cam = R.camera(W, H, math.pi / 3, IDENTITY)
            runs.append((W, H, Cn, shape, imgs, cam, g))
        Q.sync()
        s = torch.cuda.Stream(dev)
        got = []
        with torch.cuda.stream(s):
            for (W, H, Cn, shape, imgs, cam, g) in runs:
                got.append(_chain_dev(R, r, imgs, tp, vr, dv, cam, g, W, H, Cn, dev, s))
        s.synchronize()
        for (W, H, Cn, shape, imgs, cam, g), o in zip(runs, got):
            want = _chain_host(R, imgs, tp, vr, dv, cam, g)
            assert (want[0]["n"] == 2).mean() > 0.5 and (want[1] > 0.0).mean() > 0.5
            _chain_check(R, o, want, shape, H, W)
    finally:
        r.close()


# ---- 3. isolation, and the scratch shared with rr_denoise_device ----
def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_the_entries_leave_frames_stats_and_the_denoiser_alone(R, dev):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        scene = VA.yaml_scene(R, "c4_teapot.yaml", 64, 32)
        r.upload(scene)
        W, H = 70, 37
        f = V.frame(W, H)
        t = {k: to_dev(f[k], dev) for k in PLANES + ("img3", "m2_3", "count", "var")}
        before = r.render(scene.camera, max_depth=5)
        launch = r.resident_launch()
        st = r.last_stats()
        img, vr, args = V.variance_arguments(R, W, H, 3, "all", "mixed")
        assert V.same_bits(variance_dev(r, vr, W, H, 3, t, PLANES, True, dev), V.variance_expected(W, H, 3, "all", "mixed"))
        r.variance(img, vr, **args)
        img, var, dv, planes = V.filter_arguments(R, W, H, 3, 6, "all", "colour")
        assert V.same_bits(filter_dev(r, dv, W, H, 3, t, PLANES, dev)[0], V.filter_expected(W, H, 3, 6, "all", "colour")[0])
        r.denoise_var(img, var, dv, **planes)
        assert r.last_stats() == st and r.resident_launch() == launch
        after = r.render(scene.camera, max_depth=5)
        assert Q.same(before["avg"], after["avg"])
        assert _without_time(before["stats"]) == _without_time(after["stats"])
        # rr_denoise_device shares the records and the two images: a fixed case of its own still gives denoise_filter's bits
        dimg, dn, dplanes = D.arguments(R, W, H, 3, 6, "all")
        td = {k: to_dev(D.frame(W, H)[k], dev) for k in PLANES + ("img3",)}
        out = blank(H * W * 3, dev)
        Q.sync()
        r.denoise_device(dn, W, H, 3, td["img3"].data_ptr(), out.data_ptr(), **{"d_" + k: td[k].data_ptr() for k in dplanes})
        Q.sync()
        assert D.same_bits(fetch(out, (H, W, 3)), D.expected(W, H, 3, 6, "all"))
        assert D.same_bits(r.denoise(dimg, dn, **dplanes), D.expected(W, H, 3, 6, "all"))
    finally:
        r.close()


# ---- 4. refusals ----
def test_refusals_that_need_a_context(R, renderer, dev):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    f = V.frame(W, H)
    keys = PLANES + ("img3", "m2_3", "count", "var")
    t = {k: to_dev(f[k], dev) for k in keys}
    d_var, d_out, d_vout = blank(W * H, dev), blank(W * H * 3, dev), blank(W * H, dev)
    h_var, h_out, h_vout = np.full((H, W), SENT), np.full((H, W, 3), SENT), np.full((H, W), SENT)
    Q.sync()
    h = renderer.h
    ptr = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    hp = {k: f[k].ctypes.data_as(E._I if k in ("object", "count") else E._D) for k in keys}
    pd = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    ph = lambda a: a.ctypes.data_as(E._D)  # noqa: E731

    def err():
        return L.rr_last_error().decode()

    def vdesc(**kw):
        fields = dict(flags=1, min_history=4, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
        fields.update(kw)
        return C.byref(E.VarianceDesc(*fields.values()))

    def vcall(d=None, ctx=h, w=W, hh=H, c=3, skip=(), src="img3", dst=None, nodesc=False):
        """(device entry, host entry) return codes of rr_variance"""
        d = None if nodesc else (d or vdesc())
        names = ("m2_3", "count") + PLANES
        o_dev, o_host = (pd(d_var), ph(h_var)) if dst is None else dst
        return (L.rr_variance_device(ctx, d, w, hh, c, ptr[src] if src else None, *[None if k in skip else ptr[k] for k in names],
                                     o_dev, None),
                L.rr_variance(ctx, d, w, hh, c, hp[src] if src else None, *[None if k in skip else hp[k] for k in names], o_host))

    assert vcall(ctx=None) == (ARG, ARG) and vcall(nodesc=True) == (ARG, ARG) and vcall(src=None) == (ARG, ARG)
    assert vcall(dst=(None, None)) == (ARG, ARG)
    for c in (0, 2, 4):
        assert vcall(c=c) == (ARG, ARG)
    for w, hh in ((0, 5), (7, 0), (-1, 5)):
        assert vcall(w=w, hh=hh) == (ARG, ARG)
    for kw in (dict(flags=2), dict(flags=-1), dict(min_history=-1), dict(min_history=E.RR_MAX_TEMPORAL_HISTORY + 1),
               dict(sigma_normal=math.nan), dict(sigma_depth=math.inf), dict(sigma_albedo=-0.5)):
        assert vcall(vdesc(**kw)) == (ARG, ARG), kw
    assert vcall(skip=("m2_3",)) == (ARG, ARG) and "go together" in err() and vcall(skip=("count",)) == (ARG, ARG)
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert vcall(skip=(k,)) == (ARG, ARG) and "plane" in err(), k
        assert vcall(vdesc(**off), skip=(k,)) == (0, 0), k
    assert vcall(dst=(ptr["img3"], hp["img3"])) == (ARG, ARG) and "overlap" in err()
    inside = (C.c_void_p(t["m2_3"].data_ptr() + 64), C.cast(C.c_void_p(f["m2_3"].ctypes.data + 64), E._D))
    assert vcall(dst=inside) == (ARG, ARG) and "overlap" in err()
    assert vcall(w=2**16, hh=2**15) == (LIM, LIM) and "2^31" in err()

    def desc(**kw):
        fields = dict(iterations=2, flags=1, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1,
                      epsilon=1e-12)
        fields.update(kw)
        return C.byref(E.DenoiseVarDesc(*fields.values()))

    def call(d=None, ctx=h, w=W, hh=H, c=3, skip=(), src="img3", var="var", dst=None, vdst=None, nodesc=False):
        """(device entry, host entry) return codes of rr_denoise_var"""
        d = None if nodesc else (d or desc())
        o_dev, o_host = (pd(d_out), ph(h_out)) if dst is None else dst
        v_dev, v_host = (pd(d_vout), ph(h_vout)) if vdst is None else vdst
        return (L.rr_denoise_var_device(ctx, d, w, hh, c, ptr[src] if src else None, ptr[var] if var else None,
                                        *[None if k in skip else ptr[k] for k in PLANES], o_dev, v_dev, None),
                L.rr_denoise_var(ctx, d, w, hh, c, hp[src] if src else None, hp[var] if var else None,
                                 *[None if k in skip else hp[k] for k in PLANES], o_host, v_host))

    assert call(ctx=None) == (ARG, ARG) and call(nodesc=True) == (ARG, ARG) and call(src=None) == (ARG, ARG)
    assert call(dst=(None, None)) == (ARG, ARG) and call(var=None) == (ARG, ARG) and "var" in err()
    for c in (0, 2, 4):
        assert call(c=c) == (ARG, ARG)
    for w, hh in ((0, 5), (7, 0), (-1, 5)):
        assert call(w=w, hh=hh) == (ARG, ARG)
    for kw in (dict(iterations=0), dict(iterations=E.RR_MAX_DENOISE_ITERATIONS + 1), dict(flags=2), dict(flags=-1),
               dict(sigma_color=-1.0), dict(sigma_normal=math.nan), dict(sigma_depth=math.inf), dict(sigma_albedo=-0.5),
               dict(epsilon=0.0), dict(epsilon=-1.0), dict(epsilon=math.nan), dict(epsilon=math.inf)):
        assert call(desc(**kw)) == (ARG, ARG), kw
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert call(skip=(k,)) == (ARG, ARG) and "plane" in err(), k
        assert call(desc(**off), skip=(k,)) == (0, 0), k
    # an output overlapping an input or the other output
    assert call(dst=(ptr["img3"], hp["img3"])) == (ARG, ARG) and "overlap" in err()
    assert call(dst=(ptr["var"], hp["var"])) == (ARG, ARG) and "overlap" in err()
    assert call(vdst=(ptr["var"], hp["var"])) == (ARG, ARG) and "overlap" in err()
    inside = (C.c_void_p(t["normal"].data_ptr() + 64), C.cast(C.c_void_p(f["normal"].ctypes.data + 64), E._D))
    assert call(dst=inside) == (ARG, ARG) and call(vdst=inside) == (ARG, ARG) and "overlap" in err()
    both = (C.c_void_p(d_out.data_ptr() + 64), C.cast(C.c_void_p(h_out.ctypes.data + 64), E._D))
    assert call(vdst=both) == (ARG, ARG) and "overlap" in err()
    assert call(w=2**16, hh=2**15) == (LIM, LIM) and "2^31" in err()
    # a virtual (multi-device) context
    v = R.Renderer.virtual(0, 2)
    try:
        assert call(ctx=v.h) == (ARG, ARG) and "single-device" in err()
        assert vcall(ctx=v.h) == (ARG, ARG) and "single-device" in err()
    finally:
        v.close()
    # no scene is needed, and the calls serve after the refusals
    fresh = R.Renderer(0)
    try:
        assert call(ctx=fresh.h) == (0, 0) and vcall(ctx=fresh.h) == (0, 0)
    finally:
        fresh.close()
    assert call() == (0, 0) and vcall() == (0, 0)
    Q.sync()
    planes = {k: f[k] for k in PLANES}
    want = R.variance_estimate(f["img3"], R.Variance(object=True, sigma_albedo=0.1), m2=f["m2_3"], count=f["count"], **planes)
    assert V.same_bits(fetch(d_var, (H, W)), want) and V.same_bits(h_var, want)
    want, want_v = R.denoise_var_filter(f["img3"], f["var"], R.DenoiseVar(2, object=True), return_var=True, **planes)
    assert V.same_bits(fetch(d_out, (H, W, 3)), want) and V.same_bits(h_out, want)
    assert V.same_bits(fetch(d_vout, (H, W)), want_v) and V.same_bits(h_vout, want_v)


# ---- 5. end to end ----
def _sq(a, ref, mask):
    e = (a - ref)[mask]
    return float((e * e).sum())


def test_accumulated_occlusion_planes_come_closer_to_the_converged_one(R, renderer, oracle_mod):
    """48 x 32 of test_gpu_ao.py's plane + sphere + cube scene.  Eight K = 4 occlusion planes accumulated under a fixed
    camera with moments, then variance + denoise_var at their defaults, against the K = 1024 plane over the hits: the
    result's squared error is below the accumulated plane's.  The same with no history: one K = 4 plane, the spatial
    branch everywhere.  The ratios printed here, and the plain denoise's on the same inputs, are recorded in DESIGN.md
    §3.25."""
    b, _, view = A.ground_scene(R, oracle_mod)
    renderer.upload(b)
    cam = R.camera(48, 32, math.pi / 3, view)
    g = renderer.render_aov(cam)
    planes = {k: g[k] for k in PLANES}
    ref = renderer.render_ao(cam, R.Ao(1024, 1.0, seed=99))["ao"]
    hit = g["object"] >= 0
    assert 200 < hit.sum() < 48 * 32
    tp, hist, first = R.Temporal(), None, None
    for seed in range(8):
        frame = renderer.render_ao(cam, R.Ao(4, 1.0, seed=seed))["ao"]
        first = frame if first is None else first
        hist = renderer.temporal(frame, tp, cam, cam, g["depth"], normal=g["normal"], object=g["object"], prev=hist, moments=True)
    assert (hist["n"][hit] == 8).all()
    I = 3
    vr, dv, dn = R.Variance(), R.DenoiseVar(I), R.Denoise(I)
    for name, img, kw, branch in (("eight frames accumulated", hist["out"], dict(m2=hist["m2"], count=hist["n"]), "temporal"),
                                  ("one frame, no history", first, {}, "spatial")):
        var = renderer.variance(img, vr, **kw, **planes)
        assert V.same_bits(var, R.variance_estimate(img, vr, **kw, **planes))
        assert (var[~hit] == 0.0).all() and (var[hit] > 0.0).any()
        out = renderer.denoise_var(img, var, dv, **planes)
        assert V.same_bits(out, R.denoise_var_filter(img, var, dv, **planes)) and V.same_bits(out[~hit], img[~hit])
        plain = renderer.denoise(img, dn, **planes)
        before, after, after_plain = _sq(img, ref, hit), _sq(out, ref, hit), _sq(plain, ref, hit)
        print(f"denoise_var AO 48x32 K=4 against K=1024, {name} ({branch} branch), {I} levels: squared error ratio "
              f"{after / before:.4f}; plain denoise at its defaults {after_plain / before:.4f}")
        assert after < before, (name, after / before)
