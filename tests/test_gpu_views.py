"""Batches of views on the GPU (rr_render_views).  The feature has an exact definition — view k of a
batch is the frame render(cams[k], ...) returns, bit for bit — so every reference is a call the rest of the suite
already pins to the oracle, and every comparison is np.array_equal: no tolerance applies anywhere.  The counters that
do not depend on the culling bundles (rays, shadow_rays, shade_events, n1n2_scans, samples, nan_rays) are the sums of
the single frames' values."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import scene_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")
COUNTERS = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples", "nan_rays")


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


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def translate(x, y, z):
    return [1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1]


def scale_at(s, x, y, z):
    return [s, 0, 0, x, 0, s, 0, y, 0, 0, s, z, 0, 0, 0, 1]


def ring(R, cam_like, hs, vs, n, non_affine_at=None):
    """n cameras of hs x vs around cam_like's view: each turned about the camera's y axis, shifted and with a field of
    view of its own.  non_affine_at: that camera's transform gets a last row other than (0, 0, 0, 1)."""
    T = np.array(list(cam_like.transform), np.float64).reshape(4, 4)
    out = []
    for k in range(n):
        a = 0.05 * k - 0.04
        rot = np.array([[math.cos(a), 0, math.sin(a), 0.03 * k], [0, 1, 0, -0.02 * k], [-math.sin(a), 0, math.cos(a), 0],
                        [0, 0, 0, 1]])
        M = rot @ T
        if k == non_affine_at:
            M[3] = [0.0, 0.02, 0.0, 1.05]
        out.append(R.camera(hs, vs, cam_like.field_of_view * (1.0 - 0.06 * k), [float(v) for v in M.reshape(-1)]))
    return out


def singles(renderer, cams, aa, depth, seed=0, jitter_mode=0):
    return [renderer.render(c, aa=aa, max_depth=depth, seed=seed, jitter_mode=jitter_mode, canvas=True) for c in cams]


def check_batch(renderer, cams, aa, depth, what, seed=0, jitter_mode=0, refs=None):
    """the batch (canvas and avg) against the single frames; returns (batch, single frames)"""
    refs = refs or singles(renderer, cams, aa, depth, seed, jitter_mode)
    got = renderer.render_views(cams, aa=aa, max_depth=depth, seed=seed, jitter_mode=jitter_mode, canvas=True)
    n, vs, hs = len(cams), cams[0].vsize, cams[0].hsize
    assert got["avg"].shape == (n, vs // aa, hs // aa, 3) and got["canvas"].shape == (n, vs, hs, 3), what
    for k, ref in enumerate(refs):
        bad_c = int((got["canvas"][k] != ref["canvas"]).any(axis=2).sum())
        bad_a = int((got["avg"][k] != ref["avg"]).any(axis=2).sum())
        print(f"{what}: view {k}: {bad_c} of {vs * hs} samples and {bad_a} of {vs * hs // (aa * aa)} pixels differ")
        assert same(got["canvas"][k], ref["canvas"]), (what, k)
        assert same(got["avg"][k], ref["avg"]), (what, k)
    for c in COUNTERS:
        assert got["stats"][c] == sum(r["stats"][c] for r in refs), (what, c)
    only_avg = renderer.render_views(cams, aa=aa, max_depth=depth, seed=seed, jitter_mode=jitter_mode)
    assert only_avg["canvas"] is None and same(only_avg["avg"], got["avg"]), what  # the image without the caller's canvas
    return got, refs


def flat_scene(R):
    """a checker floor and three matt spheres: no secondary rays (fused level 0)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9))):
        b.sphere(transform=scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.0, 0.0, 1.0),
                 pattern=b.pattern("solid", color=col))
    return b, R.camera(8, 8, math.pi / 3, translate(0, -0.5, 0))


def chain_scene(R):
    """the same with reflective spheres and floor: reflection chains inside the camera waves"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.2, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9))):
        b.sphere(transform=scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.4, 0.0, 1.0),
                 pattern=b.pattern("solid", color=col))
    return b, R.camera(8, 8, math.pi / 3, translate(0, -0.5, 0))


def csg_scene(R):
    """a lens and a cube minus a sphere over a checker floor: the general kernels (G = 2)"""
    b = R.SceneBuilder()
    b.point_light((-6, 8, 4), (1, 1, 1))
    b.plane(transform=translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(0.9, 0.9, 0.9)), b=b.pattern("solid", color=(0.1, 0.1, 0.1))))
    c = b.csg("intersection", transform=translate(-1.2, 0, -5))
    b.sphere(transform=translate(-0.4, 0, 0), material=(0.1, 0.8, 0.3, 50.0, 0.0, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.9, 0.2, 0.2)), parent=c)
    b.sphere(transform=translate(0.4, 0, 0), material=(0.1, 0.8, 0.3, 50.0, 0.0, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.2, 0.9, 0.2)), parent=c)
    d = b.csg("difference", transform=translate(1.3, 0, -5))
    b.cube(transform=scale_at(0.8, 0, 0, 0), material=(0.1, 0.8, 0.3, 50.0, 0.0, 0.0, 1.0),
           pattern=b.pattern("solid", color=(0.2, 0.3, 0.9)), parent=d)
    b.sphere(material=(0.1, 0.8, 0.3, 50.0, 0.0, 0.0, 1.0), pattern=b.pattern("solid", color=(0.9, 0.8, 0.1)), parent=d)
    return b, R.camera(8, 8, math.pi / 3, translate(0, -0.3, 0))


def yaml_scene(R, name, W, H, aa=1, root=SCENES):
    return R.YamlScene(open(os.path.join(root, name)).read(), W, H, aa, obj_root=root)


# (W, H per view, aa, N): full tiles; ragged (143 samples: the last wave of each view short); a 16 x 16 canvas at aa 2
# (the waves average); a ragged 15 x 12 canvas at aa 3 (stacked canvases through the box average)
SHAPES = [(16, 16, 1, 1), (16, 16, 1, 2), (16, 16, 1, 5), (13, 11, 1, 2), (13, 11, 1, 5), (8, 8, 2, 3), (5, 4, 3, 3)]


@pytest.mark.parametrize("W,H,aa,n", SHAPES, ids=[f"{w}x{h}_aa{a}_n{n}" for w, h, a, n in SHAPES])
@pytest.mark.parametrize("kind", ["level0", "chain"])
def test_shapes_equal_their_single_frames(R, renderer, kind, W, H, aa, n):
    scene, cam_like = flat_scene(R) if kind == "level0" else chain_scene(R)
    renderer.upload(scene)
    check_batch(renderer, ring(R, cam_like, W * aa, H * aa, n), aa, 5, f"{kind} {W}x{H} aa {aa} n {n}")


# (id, scene, max_depth): one row per kernel family and variant of the production dispatch
FAMILIES = [
    ("c2_flat_global_culls", "c2_s1024.yaml", 5),
    ("fuzz_flat_lds_culls", ("build", 0), None),
    ("c3_chain", "c3_s1024_reflect.yaml", 5),
    ("c4_groups", "c4_teapot.yaml", 5),
    ("c1_tree", "c1_readme.yaml", 5),
    ("csg_general", None, 5),
    ("perturbed_pattern_cp", "perturbed_pattern.yaml", 5),
]


@pytest.mark.parametrize("name,src,depth", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_kernel_family_and_variant(R, renderer, name, src, depth):
    if src is None:
        scene, cam_like = csg_scene(R)
    elif isinstance(src, tuple):
        P, spec, depth, _ = F.build(src[1])
        scene, cam_like = P.b, F.cameras(P, spec, 16, 16)[0]
    else:
        scene = yaml_scene(R, src, 16, 16, 1, GOLDEN if src == "perturbed_pattern.yaml" else SCENES)
        cam_like = scene.camera
    renderer.upload(scene)
    for W, H in ((16, 16), (13, 11)):
        check_batch(renderer, ring(R, cam_like, W, H, 3), 1, depth, f"{name} {W}x{H}")


def test_area_light_jitter_is_the_single_frames(R, renderer):
    """a sample's jitter identity is py * hsize + px within its own view, whatever the view's place in the batch"""
    scene = yaml_scene(R, "c5_area_light.yaml", 16, 16)
    P, spec, mix_depth, _ = F.build_area_mix(8)
    for what, sc, cam_like, depth in (("c5", scene, scene.camera, 5), ("mix-8", P.b, F.cameras(P, spec, 16, 16)[0], mix_depth)):
        renderer.upload(sc)
        for W, H in ((16, 16), (13, 11)):
            cams = ring(R, cam_like, W, H, 3)
            for seed in (3, 12345):
                check_batch(renderer, cams, 1, depth, f"{what} {W}x{H} seed {seed}", seed=seed, jitter_mode=0)
            twice = [cams[1], cams[0], cams[1]]
            got = renderer.render_views(twice, max_depth=depth, seed=3, jitter_mode=0, canvas=True)
            assert same(got["canvas"][0], got["canvas"][2]) and same(got["avg"][0], got["avg"][2]), what
            assert not same(got["canvas"][0], got["canvas"][1]), what


def test_a_batch_against_the_oracle_itself(R, renderer):
    P, spec, depth, cat = F.build(5)
    renderer.upload(P.b)
    base, _ = F.cameras(P, spec, 16, 16)
    cams = ring(R, base, 16, 16, 3)
    got = renderer.render_views(cams, max_depth=depth, canvas=True)
    import oracle

    for k, c in enumerate(cams):
        ocam = oracle.Oracle.camera(16, 16, c.field_of_view, list(c.transform))
        canvas_cr, st_cr = F.oracle_frame(P, ocam, depth)
        one = renderer.render(c, max_depth=depth, canvas=True)  # the counters are per batch: the view's own from its frame
        F.check_frame({"canvas": got["canvas"][k], "stats": one["stats"]}, P, f"seed 5 ({cat}) view {k}", canvas_cr, st_cr)
    want = [F.oracle_counts(F.oracle_frame(P, oracle.Oracle.camera(16, 16, c.field_of_view, list(c.transform)), depth)[1])
            for c in cams]
    for key in ("rays", "shadow_rays", "shade_events"):
        assert got["stats"][key] == sum(w[key] for w in want), key


@contextlib.contextmanager
def environment(**kv):
    """the switches the library reads from the environment (RRAY_BATCH at context creation, the per-level switches at
    every call), restored afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_passes_of_whole_views_under_a_small_batch(R):
    with environment(RRAY_BATCH="1024"):  # read when a context is created
        r = R.Renderer(0)
    try:
        scene, cam_like = chain_scene(R)
        r.upload(scene)
        cams = ring(R, cam_like, 16, 16, 9)
        refs = singles(r, cams, 1, 5)
        r.kernel_profile(True)
        try:
            got = r.render_views(cams, canvas=True)
            launches = r.kernel_times()["chain"][1]
        finally:
            r.kernel_profile(False)
        assert launches == 3, launches  # 9 views of 256 events in passes of 4, 4 and 1
        check_batch(r, cams, 1, 5, "9 views in 3 passes", refs=refs)
        assert same(got["canvas"], np.stack([x["canvas"] for x in refs]))
        # ragged views: 192 events each, 5 per pass
        check_batch(r, ring(R, cam_like, 13, 11, 7), 1, 5, "7 ragged views in 2 passes")
        big = ring(R, cam_like, 40, 32, 2)
        with pytest.raises(R.RRError) as e:
            r.render_views(big)
        assert e.value.code == R._lib.RR_E_LIMIT and "one pass" in str(e.value)
        assert r.render(big[0])["avg"].shape == (32, 40, 3)  # such a view is rr_render's
    finally:
        r.close()


def test_a_non_affine_camera_between_affine_ones(R, renderer):
    for kind in (flat_scene, chain_scene):
        scene, cam_like = kind(R)
        renderer.upload(scene)
        for W, H in ((16, 16), (13, 11)):
            cams = ring(R, cam_like, W, H, 3, non_affine_at=1)
            assert list(cams[1].transform)[12:] != [0.0, 0.0, 0.0, 1.0]
            check_batch(renderer, cams, 1, 5, f"{kind.__name__} non-affine {W}x{H}")


def test_device_entry_point_on_torch_streams(R, renderer):
    W, H, n = 16, 16, 3
    scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    cams_a = ring(R, cam_like, W, H, n)
    cams_b = list(reversed(ring(R, cam_like, W, H, n + 2)))[:n]
    ref_a = np.stack([renderer.render(c)["avg"] for c in cams_a])
    ref_b = np.stack([renderer.render(c)["avg"] for c in cams_b])
    assert not same(ref_a, ref_b)
    dev = torch.device("cuda", 0)
    o = R._lib.RenderOpts(1, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG, 0, 0)
    a = torch.full((n, H, W, 3), -1.0, dtype=torch.float64, device=dev)
    b = torch.full((n, H, W, 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    # two batches back to back, no synchronise between them: each keeps its own cameras
    renderer.render_views_device(cams_a, o, None, a.data_ptr(), stream.cuda_stream)
    renderer.render_views_device(cams_b, o, None, b.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert same(a.cpu().numpy(), ref_a) and same(b.cpu().numpy(), ref_b)
    # canvas and image together, on a stream that lags behind: work queued on it before the call
    oc = R._lib.RenderOpts(1, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG | R._lib.RR_OUT_CANVAS, 0, 0)
    lag = torch.cuda.Stream(dev)
    img = torch.full((n, H, W, 3), -1.0, dtype=torch.float64, device=dev)
    cnv = torch.full((n, H, W, 3), -1.0, dtype=torch.float64, device=dev)
    busy = torch.ones((2048, 2048), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(lag):
        for _ in range(8):
            busy = busy @ busy * 1e-4
        img.fill_(-2.0)  # ordered before the render on this stream: the render must overwrite it
    renderer.render_views_device(cams_a, oc, cnv.data_ptr(), img.data_ptr(), lag.cuda_stream)
    lag.synchronize()
    assert same(img.cpu().numpy(), ref_a) and same(cnv.cpu().numpy(), ref_a)  # aa 1: the canvas is the image
    st = renderer.last_stats()
    assert st["samples"] == n * W * H


def test_a_batch_leaves_the_single_frame_state_alone(R):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H, depth in (("c2_s1024.yaml", 512, 512, 5), ("c4_teapot.yaml", 64, 32, 5), ("c3_s1024_reflect.yaml", 48, 24, 5)):
            scene = yaml_scene(R, src, W, H)
            r.upload(scene)
            before = r.render(scene.camera, max_depth=depth)
            launch = r.resident_launch()
            mid = r.render_views(ring(R, scene.camera, 16, 16, 3), max_depth=depth)
            assert r.resident_launch() == (0, 0), src
            after = r.render(scene.camera, max_depth=depth)
            assert r.resident_launch() == launch, src
            assert mid["stats"]["samples"] == 3 * 256
            assert same(before["avg"], after["avg"]), src
            sa, sb = dict(before["stats"]), dict(after["stats"])
            sa.pop("kernel_ms"), sb.pop("kernel_ms")
            assert sa == sb, src  # prim_tests and wave_visits too: the cached bundles and the order are untouched
    finally:
        r.close()


def test_no_views_and_depth_zero(R, renderer):
    L, E = R.lib(), R._lib
    scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    cams = ring(R, cam_like, 16, 16, 2)
    arr = (E.Camera * 2)(*cams)
    o = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_OUT_CANVAS, 0, 0)
    avg, cnv = np.full((2, 16, 16, 3), -3.0), np.full((2, 16, 16, 3), -4.0)
    assert L.rr_render_views(renderer.h, arr, 0, C.byref(o), cnv.ctypes.data_as(E._D), avg.ctypes.data_as(E._D), None) == 0
    assert (avg == -3.0).all() and (cnv == -4.0).all()
    empty = renderer.render_views([])
    assert empty["avg"].shape == (0, 0, 0, 3)
    # depth 0 on the reflective scene: the fused level-0 family
    renderer.kernel_profile(True)
    try:
        check_batch(renderer, ring(R, cam_like, 13, 11, 3), 1, 0, "chain scene at depth 0")
        kt = {k: v[1] for k, v in renderer.kernel_times().items() if v[1]}
    finally:
        renderer.kernel_profile(False)
    assert "chain" not in kt and kt["trace_shade"] >= 1, kt


def test_refusals_on_a_live_context(R, renderer):
    L, E = R.lib(), R._lib
    scene, cam_like = flat_scene(R)
    renderer.upload(scene)
    cams = ring(R, cam_like, 16, 16, 2)
    arr = (E.Camera * 2)(*cams)
    avg = np.zeros((2, 16, 16, 3))
    p = avg.ctypes.data_as(E._D)

    def call(h, opts, a=arr, n=2, out=p):
        return L.rr_render_views(h, a, n, C.byref(opts), None, out, None)

    ok = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 0, 0)
    assert call(renderer.h, ok) == 0
    assert call(renderer.h, ok, out=None) == E.RR_E_ARG and "null image buffer" in L.rr_last_error().decode()
    assert call(renderer.h, E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_OUT_CANVAS, 0, 0)) == E.RR_E_ARG
    assert "null canvas buffer" in L.rr_last_error().decode()
    assert call(renderer.h, E.RenderOpts(3, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 0, 0)) == E.RR_E_ARG  # 16 is no multiple of 3
    assert "multiple of aa" in L.rr_last_error().decode()
    assert call(renderer.h, E.RenderOpts(1, 99, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 0, 0)) == E.RR_E_LIMIT  # as rr_render
    assert call(renderer.h, E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_NO_FRAME_TIMING, 0, 0)) == 0
    assert renderer.last_stats()["kernel_ms"] == 0.0
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert call(v.h, ok) == E.RR_E_ARG and "single-device" in L.rr_last_error().decode()
    finally:
        v.close()
    fresh = R.Renderer(0)
    try:
        assert call(fresh.h, ok) == E.RR_E_ARG and "no scene" in L.rr_last_error().decode()
    finally:
        fresh.close()


@pytest.mark.parametrize("switch,kind", [("RRAY_UNFUSED", "chain"), ("RRAY_NO_CHAIN", "chain"), ("RRAY_NO_TREE", "tree")])
def test_per_level_switches_are_refused(R, renderer, switch, kind):
    if kind == "tree":
        scene = yaml_scene(R, "c1_readme.yaml", 16, 16)
        cam_like = scene.camera
    else:
        scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    cams = ring(R, cam_like, 16, 16, 2)
    with environment(**{switch: "1"}):
        with pytest.raises(R.RRError) as e:
            renderer.render_views(cams)
    assert e.value.code == R._lib.RR_E_ARG and "per-level" in str(e.value)
    check_batch(renderer, cams, 1, 5, f"after {switch}")  # and the context is as good as before
