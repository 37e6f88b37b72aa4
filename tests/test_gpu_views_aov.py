"""First-hit planes of batches of views on the GPU (rr_render_views_aov).  The definition is exact —
slice k of each requested plane is what render_aov(cams[k], ...) writes, bit for bit — so every reference is a
render_aov call that tests/test_gpu_hit.py already pins to the oracle, and every comparison is np.array_equal with
equal_nan: no tolerance applies anywhere.  rays and samples are n_views * hsize * vsize, nan_rays is the sum of the
single frames' values, and the shading counters are zero."""
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
PLANES = ("depth", "normal", "object", "albedo")
VEC = ("point", "eyev", "normalv", "over_point", "under_point", "reflectv")


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
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


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


def flat_scene(R):
    """a checker floor and three matt spheres"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    for x, z, s, col in ((0.3, -4, 1.0, (0.9, 0.3, 0.2)), (-1.6, -5, 0.7, (0.2, 0.8, 0.3)), (1.7, -3.5, 0.5, (0.2, 0.3, 0.9))):
        b.sphere(transform=scale_at(s, x, s - 1.0, z), material=(0.1, 0.7, 0.3, 100.0, 0.0, 0.0, 1.0),
                 pattern=b.pattern("solid", color=col))
    return b, R.camera(8, 8, math.pi / 3, translate(0, -0.5, 0))


def chain_scene(R):
    """the same with reflective spheres and floor"""
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


def singles(renderer, cams, aa=1, planes=PLANES):
    return [renderer.render_aov(c, aa=aa, planes=planes) for c in cams]


def check_batch(renderer, cams, aa, what, planes=PLANES, refs=None):
    """the batch's planes against the single frames', and the counters; returns (batch, single frames)"""
    refs = refs or singles(renderer, cams, aa, planes)
    got = renderer.render_views_aov(cams, aa=aa, planes=planes)
    n, vs, hs = len(cams), cams[0].vsize, cams[0].hsize
    assert sorted(got) == sorted(planes + ("stats",)), what  # unrequested planes are not returned
    for p in planes:
        assert got[p].shape == (n, vs, hs) + ((3,) if p in ("normal", "albedo") else ()), (what, p)
        assert got[p].dtype == (np.int32 if p == "object" else np.float64), (what, p)
        for k, ref in enumerate(refs):
            d = got[p][k] != ref[p]
            if p != "object":
                d &= ~(np.isnan(got[p][k]) & np.isnan(ref[p]))
            print(f"{what}: view {k}: plane {p}: {int(d.reshape(vs * hs, -1).any(axis=1).sum())} of {vs * hs} samples differ")
            assert same(got[p][k], ref[p]), (what, p, k)
    st = got["stats"]
    assert st["rays"] == st["samples"] == n * hs * vs, (what, st)
    assert st["shadow_rays"] == st["shade_events"] == st["n1n2_scans"] == 0, (what, st)
    assert st["nan_rays"] == sum(r["stats"]["nan_rays"] for r in refs), (what, st)
    return got, refs


# (W, H per view, aa, N): full tiles; ragged (143 samples: the last wave of each view has idle lanes, inside the launch
# for every view but the last); a 16 x 16 canvas at aa 2 and a ragged 15 x 12 one at aa 3 (aa only has to divide)
SHAPES = [(16, 16, 1, 1), (16, 16, 1, 2), (16, 16, 1, 5), (13, 11, 1, 2), (13, 11, 1, 5), (8, 8, 2, 3), (5, 4, 3, 3)]


@pytest.mark.parametrize("W,H,aa,n", SHAPES, ids=[f"{w}x{h}_aa{a}_n{n}" for w, h, a, n in SHAPES])
def test_shapes_equal_their_single_frames(R, renderer, W, H, aa, n):
    scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    got, _ = check_batch(renderer, ring(R, cam_like, W * aa, H * aa, n), aa, f"{W}x{H} aa {aa} n {n}")
    assert (got["object"] >= 0).any() and (got["object"] < 0).any()  # hits and sky in view: the planes say something


# one row per variant of the first-hit kernel's dispatch (G, LC, CP)
VARIANTS = [
    ("c2_flat_global_culls", "c2_s1024.yaml"),
    ("fuzz_flat_lds_culls", ("build", 0)),
    ("c4_groups", "c4_teapot.yaml"),
    ("c1_glass", "c1_readme.yaml"),
    ("csg_general", None),
    ("perturbed_pattern_cp", "perturbed_pattern.yaml"),
]


@pytest.mark.parametrize("name,src", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_kernel_variant(R, renderer, name, src):
    if src is None:
        scene, cam_like = csg_scene(R)
    elif isinstance(src, tuple):
        P, spec, _, _ = F.build(src[1])
        scene, cam_like = P.b, F.cameras(P, spec, 16, 16)[0]
    else:
        scene = yaml_scene(R, src, 16, 16, 1, GOLDEN if src == "perturbed_pattern.yaml" else SCENES)
        cam_like = scene.camera
    renderer.upload(scene)
    for W, H in ((16, 16), (13, 11)):
        check_batch(renderer, ring(R, cam_like, W, H, 3), 1, f"{name} {W}x{H}")


def _device_planes(n, V, Hs, dev):
    return {"depth": torch.full((n, V, Hs), -1.0, dtype=torch.float64, device=dev),
            "normal": torch.full((n, V, Hs, 3), -1.0, dtype=torch.float64, device=dev),
            "object": torch.full((n, V, Hs), -7, dtype=torch.int32, device=dev),
            "albedo": torch.full((n, V, Hs, 3), -1.0, dtype=torch.float64, device=dev)}


def test_plane_subsets_leave_the_other_planes_alone(R, renderer):
    scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    n, Hs, V = 3, 13, 11
    cams = ring(R, cam_like, Hs, V, n)
    full = renderer.render_views_aov(cams)
    for p in PLANES:  # the host entry: each plane alone
        got, _ = check_batch(renderer, cams, 1, f"only {p}", planes=(p,))
        assert same(got[p], full[p]), p
    dev = torch.device("cuda", 0)
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    stream = torch.cuda.Stream(dev)
    for want in [(p,) for p in PLANES] + [("depth", "object"), ("normal", "albedo")]:  # the device entry
        t = _device_planes(n, V, Hs, dev)
        torch.cuda.synchronize(dev)
        # every pointer is passed: an unrequested plane's is ignored
        renderer.render_views_aov_device(cams, opts, want, t["depth"].data_ptr(), t["normal"].data_ptr(),
                                         t["object"].data_ptr(), t["albedo"].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        for p in PLANES:
            host = t[p].cpu().numpy()
            if p in want:
                assert same(host, full[p]), (want, p)
            else:
                assert (host == (-7 if p == "object" else -1.0)).all(), (want, p)


def oracle_hits(R, o, rays, to_builder=None):
    """hit() + prepare_computations of every ray from the oracle, as an array of rr_hit records (as
    tests/test_gpu_hit.py).  rays: [(origin3, direction3)]; to_builder: oracle object id -> rr_scene_desc id."""
    out = np.zeros(len(rays), R._lib.hit_dtype())
    out["object"] = -1
    for i, (ro, rd) in enumerate(rays):
        xs = o.intersect(ro, rd)
        hit = next((k for k, x in enumerate(xs) if x[0] >= 0.0), None)  # intersection.rs hit(): first t >= 0
        if hit is None:
            continue
        c = o.prepare_computations(ro, rd, xs, hit)
        rec = out[i]
        rec["object"] = xs[hit][1] if to_builder is None else to_builder[xs[hit][1]]
        rec["inside"] = int(c["inside"])
        rec["t"], rec["u"], rec["v"] = c["t"], xs[hit][2], xs[hit][3]
        for name in VEC:
            rec[name] = c[name][:3]
        rec["n1"], rec["n2"] = c["n1"], c["n2"]
    return out


def camera_rays(oracle, ocam):
    """every sample's ray_for_pixel (camera.rs:75-93), row-major"""
    rays = []
    for y in range(ocam.vsize):
        for x in range(ocam.hsize):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            rays.append((ro[:3], rd[:3]))
    return rays


def planes_of(records, V, Hs):
    """the depth / normal / object planes an AOV frame holds for these per-sample records"""
    miss = records["object"] < 0
    depth = np.where(miss, np.inf, records["t"]).reshape(V, Hs)
    return depth, records["normalv"].reshape(V, Hs, 3), records["object"].reshape(V, Hs)


def test_a_batch_against_the_oracle_itself(R, renderer):
    import oracle

    P, spec, _, cat = F.build(5)
    renderer.upload(P.b)
    base, _ = F.cameras(P, spec, 16, 16)
    cams = ring(R, base, 16, 16, 3)
    got = renderer.render_views_aov(cams, planes=("depth", "normal", "object"))
    to_builder = {v: k for k, v in P.ids.items()}
    try:
        for k, c in enumerate(cams):
            ocam = oracle.Oracle.camera(16, 16, c.field_of_view, list(c.transform))
            want = oracle_hits(R, P.o, camera_rays(oracle, ocam), to_builder)
            depth, normal, obj = planes_of(want, 16, 16)
            assert same(got["object"][k], obj.astype(np.int32)), f"seed 5 ({cat}) view {k}: object plane"
            assert same(got["depth"][k], depth), f"seed 5 ({cat}) view {k}: depth plane"
            assert same(got["normal"][k], normal), f"seed 5 ({cat}) view {k}: normal plane"
    except AssertionError:
        print("\n".join(P.log))
        raise


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
        # 9 views of 256 events: passes of 4, 4 and 1; 7 ragged views of 192 events: passes of 5 and 2
        check_batch(r, ring(R, cam_like, 16, 16, 9), 1, "9 views in 3 passes")
        check_batch(r, ring(R, cam_like, 13, 11, 7), 1, "7 ragged views in 2 passes")
        big = ring(R, cam_like, 40, 32, 2)
        with pytest.raises(R.RRError) as e:
            r.render_views_aov(big)
        assert e.value.code == R._lib.RR_E_LIMIT and "one pass" in str(e.value) and "rr_render_aov" in str(e.value)
        assert r.render_aov(big[0])["depth"].shape == (32, 40)  # such a view is rr_render_aov's
    finally:
        r.close()


def test_a_non_affine_camera_between_affine_ones(R, renderer):
    for kind in (flat_scene, chain_scene):
        scene, cam_like = kind(R)
        renderer.upload(scene)
        for W, H in ((16, 16), (13, 11)):
            cams = ring(R, cam_like, W, H, 3, non_affine_at=1)
            assert list(cams[1].transform)[12:] != [0.0, 0.0, 0.0, 1.0]
            check_batch(renderer, cams, 1, f"{kind.__name__} non-affine {W}x{H}")


def test_device_entry_point_on_a_torch_stream(R, renderer):
    P, spec, _, _ = F.build(3)  # a group scene
    renderer.upload(P.b)
    n, Hs, V = 3, 16, 16
    base, _ = F.cameras(P, spec, Hs, V)
    cams_a = ring(R, base, Hs, V, n)
    cams_b = list(reversed(ring(R, base, Hs, V, n + 2)))[:n]
    ref_a, ref_b = singles(renderer, cams_a), singles(renderer, cams_b)
    assert not same(np.stack([r["depth"] for r in ref_a]), np.stack([r["depth"] for r in ref_b]))
    dev = torch.device("cuda", 0)
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    a, b = _device_planes(n, V, Hs, dev), _device_planes(n, V, Hs, dev)
    assert a["object"].dtype == torch.int32 and a["normal"].shape == (n, V, Hs, 3)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    # two batches back to back, no synchronise between them: each keeps its own cameras
    for t, cams in ((a, cams_a), (b, cams_b)):
        renderer.render_views_aov_device(cams, opts, PLANES, t["depth"].data_ptr(), t["normal"].data_ptr(),
                                         t["object"].data_ptr(), t["albedo"].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for t, refs in ((a, ref_a), (b, ref_b)):
        for p in PLANES:
            assert same(t[p].cpu().numpy(), np.stack([r[p] for r in refs])), p
    st = renderer.last_stats()
    assert st["rays"] == st["samples"] == n * Hs * V and st["kernel_ms"] > 0


def _without_time(stats):
    s = dict(stats)
    s.pop("kernel_ms")
    return s


def test_a_batch_leaves_frames_and_colour_batches_alone(R):
    r = R.Renderer(0)  # a fresh context: its caches see only these frames
    try:
        for src, W, H in (("c2_s1024.yaml", 512, 512), ("c4_teapot.yaml", 64, 32)):
            scene = yaml_scene(R, src, W, H)
            r.upload(scene)
            cams = ring(R, scene.camera, 16, 16, 3)

            def batch():
                got = r.render_views_aov(cams)
                assert got["stats"]["samples"] == 3 * 256, src

            # rr_render: image, every counter (prim_tests and wave_visits too: the cached bundles and the order are
            # untouched) and the resident launch
            before = r.render(scene.camera, max_depth=5)
            launch = r.resident_launch()
            batch()
            assert r.resident_launch() == launch, src  # left as it was
            after = r.render(scene.camera, max_depth=5)
            assert r.resident_launch() == launch, src
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            # rr_render_aov: the frame's cached bundles serve it too
            before = r.render_aov(scene.camera)
            batch()
            after = r.render_aov(scene.camera)
            for p in PLANES:
                assert same(before[p], after[p]), (src, p)
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
            # rr_render_views: the colour batch shares the camera table with this one
            before = r.render_views(cams, max_depth=5)
            batch()
            after = r.render_views(cams, max_depth=5)
            assert same(before["avg"], after["avg"]), src
            assert _without_time(before["stats"]) == _without_time(after["stats"]), src
    finally:
        r.close()


def test_nan_rays_are_summed_and_the_host_entry_returns_rr_e_nan(R, renderer):
    """the NaN scene of tests/test_gpu_hit.py: every ray of a NaN camera meets two NaN entries.  One such camera between
    two sound ones: the planes are written, nan_rays is the NaN frame's, the host entry returns RR_E_NAN and the device
    entry reports through the stats."""
    L, E = R.lib(), R._lib
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    b.plane()
    b.plane(transform=(1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 1))
    renderer.upload(b)
    sound = ring(R, R.camera(8, 8, 1.0, translate(0, -0.5, 0)), 8, 8, 2)
    nan_cam = R.camera(8, 8, 1.0, tuple([math.nan] * 12 + [0.0, 0.0, 0.0, 1.0]))
    cams = [sound[0], nan_cam, sound[1]]
    opts = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    mask = E.RR_AOV_DEPTH | E.RR_AOV_NORMAL | E.RR_AOV_OBJECT | E.RR_AOV_ALBEDO

    def planes(n):
        return (np.full((n, 8, 8), -1.0), np.full((n, 8, 8, 3), -1.0), np.full((n, 8, 8), -7, np.int32),
                np.full((n, 8, 8, 3), -1.0))

    def pointers(p):
        return p[0].ctypes.data_as(E._D), p[1].ctypes.data_as(E._D), p[2].ctypes.data_as(E._I), p[3].ctypes.data_as(E._D)

    refs, nans = [], []
    for c in cams:  # the single frames, through the ABI: the NaN frame's planes are written before RR_E_NAN too
        one, st = planes(1), E.Stats()
        rc = L.rr_render_aov(renderer.h, C.byref(c), C.byref(opts), mask, *pointers(one), C.byref(st))
        assert rc in (0, E.RR_E_NAN)
        refs.append(one)
        nans.append(st.nan_rays)
    assert nans == [0, 64, 0]
    got, st = planes(3), E.Stats()
    arr = (E.Camera * 3)(*cams)
    rc = L.rr_render_views_aov(renderer.h, arr, 3, C.byref(opts), mask, *pointers(got), C.byref(st))
    assert rc == E.RR_E_NAN
    assert st.nan_rays == 64 and st.rays == st.samples == 3 * 64
    assert st.shadow_rays == st.shade_events == st.n1n2_scans == 0
    for k in range(3):
        for j in range(4):
            assert same(got[j][k], refs[k][j][0]), (k, PLANES[j])
    # the device entry returns RR_OK and reports the NaN rays through the stats
    dev = torch.device("cuda", 0)
    t = _device_planes(3, 8, 8, dev)
    torch.cuda.synchronize(dev)
    renderer.render_views_aov_device(cams, opts, PLANES, t["depth"].data_ptr(), t["normal"].data_ptr(),
                                     t["object"].data_ptr(), t["albedo"].data_ptr())
    assert renderer.last_stats()["nan_rays"] == 64
    assert same(t["depth"].cpu().numpy(), got[0])
    with pytest.raises(R.RRError) as e:  # and the Python mirror of the host entry raises
        renderer.render_views_aov(cams)
    assert e.value.code == E.RR_E_NAN


def test_refusals_and_the_empty_batch(R, renderer):
    L, E = R.lib(), R._lib
    scene, cam_like = flat_scene(R)
    renderer.upload(scene)
    cams = ring(R, cam_like, 16, 16, 2)
    arr = (E.Camera * 2)(*cams)
    mixed = (E.Camera * 2)(cams[0], R.camera(16, 8, 1.0))
    depth, normal = np.full((2, 16, 16), -3.0), np.full((2, 16, 16, 3), -3.0)
    obj, albedo = np.full((2, 16, 16), -7, np.int32), np.full((2, 16, 16, 3), -3.0)
    pd, pn, po, pa = depth.ctypes.data_as(E._D), normal.ctypes.data_as(E._D), obj.ctypes.data_as(E._I), albedo.ctypes.data_as(E._D)
    ALL = E.RR_AOV_DEPTH | E.RR_AOV_NORMAL | E.RR_AOV_OBJECT | E.RR_AOV_ALBEDO
    ok = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)

    def host(h, a, n, o, planes=ALL, bufs=(pd, pn, po, pa)):
        return L.rr_render_views_aov(h, a, n, C.byref(o) if o is not None else None, planes, *bufs, None)

    def dev(h, a, n, o, planes=ALL, bufs=(pd, pn, po, pa)):
        p = [C.cast(b, C.c_void_p) if b is not None else None for b in bufs]
        return L.rr_render_views_aov_device(h, a, n, C.byref(o) if o is not None else None, planes, *p, None)

    def err():
        return L.rr_last_error().decode()

    # an empty batch: RR_OK, nothing written
    assert host(renderer.h, arr, 0, ok) == 0
    assert (depth == -3.0).all() and (normal == -3.0).all() and (obj == -7).all() and (albedo == -3.0).all()
    empty = renderer.render_views_aov([])
    assert empty["depth"].shape == (0, 0, 0) and empty["object"].dtype == np.int32
    # the host-buffer entry refuses before anything is launched; the device entry takes the same checks (its buffer
    # arguments are only looked at for null here)
    for f in (host, dev):
        assert f(None, arr, 2, ok) == E.RR_E_ARG and "null context" in err()
        assert f(renderer.h, None, 2, ok) == E.RR_E_ARG and "null camera array" in err()
        assert f(renderer.h, arr, 2, None) == E.RR_E_ARG and "null options" in err()
        assert f(renderer.h, arr, -1, ok) == E.RR_E_ARG and "negative" in err()
        assert f(renderer.h, arr, 2, ok, planes=0) == E.RR_E_ARG and "RR_AOV_" in err()
        assert f(renderer.h, arr, 2, ok, planes=16) == E.RR_E_ARG and "RR_AOV_" in err()
        assert f(renderer.h, arr, 2, ok, planes=E.RR_AOV_DEPTH | E.RR_AOV_OBJECT, bufs=(pd, None, None, None)) == E.RR_E_ARG
        assert "null buffer" in err()
        assert f(renderer.h, mixed, 2, ok) == E.RR_E_ARG and "share hsize and vsize" in err()
        assert f(renderer.h, arr, 2, E.RenderOpts(3, 0, 0, 0, 0, 1, 8, 0, 0, 0)) == E.RR_E_ARG  # 16 is no multiple of 3
        assert "multiple of aa" in err()
        for bad in (E.RenderOpts(1, 0, 0, 0, 1, 2, 8, 0, 0, 0), E.RenderOpts(1, 0, 0, 0, 0, 2, 8, 0, 0, 0),
                    E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 4), E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 2, 4)):
            assert f(renderer.h, arr, 2, bad) == E.RR_E_ARG and "part 0 of 1, no band" in err()
    # an unrequested plane's pointer is ignored; max_depth, seed, jitter_mode and flags are ignored
    assert host(renderer.h, arr, 2, ok, planes=E.RR_AOV_DEPTH, bufs=(pd, None, None, None)) == 0
    assert (obj == -7).all() and not (depth == -3.0).any()
    ref = depth.copy()
    odd = E.RenderOpts(1, 99, 7, 1, 0, 1, 8, E.RR_OUT_AVG | E.RR_OUT_AVG_F32, 0, 0)
    depth[:] = -3.0
    assert host(renderer.h, arr, 2, odd, planes=E.RR_AOV_DEPTH, bufs=(pd, None, None, None)) == 0
    assert same(depth, ref)
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        for f in (host, dev):
            assert f(v.h, arr, 2, ok) == E.RR_E_ARG and "single-device" in err()
    finally:
        v.close()
    fresh = R.Renderer(0)
    try:
        for f in (host, dev):
            assert f(fresh.h, arr, 2, ok) == E.RR_E_ARG and "no scene" in err()
    finally:
        fresh.close()


@pytest.mark.parametrize("switch", ["RRAY_UNFUSED", "RRAY_NO_TREE", "RRAY_NO_CHAIN"])
def test_per_level_switches_do_not_concern_the_first_hit_kernel(R, renderer, switch):
    scene, cam_like = chain_scene(R)
    renderer.upload(scene)
    cams = ring(R, cam_like, 13, 11, 3)
    plain = renderer.render_views_aov(cams)
    with environment(**{switch: "1"}):
        served = renderer.render_views_aov(cams)
    for p in PLANES:
        assert same(served[p], plain[p]), (switch, p)
    assert _without_time(served["stats"]) == _without_time(plain["stats"]), switch
