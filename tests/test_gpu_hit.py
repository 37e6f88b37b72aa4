"""First-hit queries on the GPU (ABI 11): Renderer.hit_at and Renderer.render_aov against the reference's
Scene::intersect -> hit -> prepare_computations (scene.rs:97-106,128-136; intersection.rs:50-92), through the oracle's
`intersect` / `prepare_computations` entry points.  Every field of every record must equal the oracle's bit for bit
(np.array_equal; NaNs equal NaNs): the colour frames of the same scenes are bit-exact from the same intermediate
values (tests/test_gpu_fuzz.py), so no tolerance applies and no sample is left out."""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library: torch ships its own HIP runtime, which the library then shares (as
#               in bench.py); loaded after it, torch finds no device (test_device_planes_on_a_torch_stream uses both)

import scene_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu
EPSILON = 0.00001  # main.rs:10
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
    """bit-for-bit in the sense of the reference's values: equal, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_records_equal(got, want, what):
    bad = [n for n in want.dtype.names if not same(got[n], want[n])]
    if bad:
        for n in bad:
            d = got[n] != want[n]
            if got[n].dtype.kind == "f":
                d &= ~(np.isnan(got[n]) & np.isnan(want[n]))
            k = int(np.argwhere(d.reshape(len(got), -1).any(axis=1))[0, 0])
            print(f"{what}: field {n} differs in {int(d.reshape(len(got), -1).any(axis=1).sum())} records; first {k}: "
                  f"gpu {got[n][k].tolist()} oracle {want[n][k].tolist()}")
    assert not bad, (what, bad)


def oracle_hits(R, o, rays, to_builder=None):
    """hit() + prepare_computations of every ray from the oracle, as an array of rr_hit records.  rays: [(origin3,
    direction3)]; to_builder: oracle object id -> rr_scene_desc id (identity when None)."""
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
        for n in VEC:
            rec[n] = c[n][:3]
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


def batch(rays):
    return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


def planes_of(records, V, Hs):
    """the depth / normal / object planes an AOV frame holds for these per-sample records"""
    miss = records["object"] < 0
    depth = np.where(miss, np.inf, records["t"]).reshape(V, Hs)
    return depth, records["normalv"].reshape(V, Hs, 3), records["object"].reshape(V, Hs)


def default_scene(R):
    """Scene::default (scene.rs:79-92)"""
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    s1 = b.sphere(material=(0.1, 0.7, 0.2, 200.0, 0.0, 0.0, 1.0), pattern=b.pattern("solid", color=(0.8, 1.0, 0.6)))
    s2 = b.sphere(transform=(0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 1))
    return b, s1, s2


def test_known_answers_of_the_reference_unit_tests(R, renderer):
    b, s1, _ = default_scene(R)
    renderer.upload(b)
    h = renderer.hit_at([(0, 0, -5), (0, 0, -5)], [(0, 0, 1), (0, 1, 0)])
    a = h[0]  # intersection.rs: precomputing the state of an intersection; the hit should offset the point
    assert a["t"] == 4.0 and a["object"] == s1 and a["inside"] == 0
    assert a["point"].tolist() == [0, 0, -1] and a["eyev"].tolist() == [0, 0, -1] and a["normalv"].tolist() == [0, 0, -1]
    assert a["over_point"][2] < -EPSILON / 2 and a["point"][2] > a["over_point"][2]
    assert a["under_point"][2] > a["point"][2]
    assert a["reflectv"].tolist() == [0, 0, -1] and a["n1"] == 1.0 and a["n2"] == 1.0
    m = h[1]  # scene.rs: the colour when a ray misses
    assert m["object"] == -1
    assert all(not np.any(m[n]) for n in m.dtype.names if n != "object"), m
    st = renderer.last_stats()
    assert (st["rays"], st["samples"], st["n1n2_scans"], st["shadow_rays"], st["shade_events"]) == (2, 2, 1, 0, 0)
    b = R.SceneBuilder()  # intersection.rs: the hit, when an intersection occurs on the inside
    b.point_light((-10, 10, -10), (1, 1, 1))
    s = b.sphere()
    renderer.upload(b)
    i = renderer.hit_at([(0, 0, 0)], [(0, 0, 1)])[0]
    assert i["t"] == 1.0 and i["object"] == s and i["inside"] == 1
    assert i["point"].tolist() == [0, 0, 1] and i["eyev"].tolist() == [0, 0, -1] and i["normalv"].tolist() == [0, 0, -1]


def test_n1_n2_at_every_boundary_of_three_glass_spheres(R, renderer):
    """intersection.rs finding_n1_and_n2_at_various_intersections: A (scale 2, 1.5) holds B (z - 0.25, 2.0) and C
    (z + 0.25, 2.5).  The rays start between the surfaces, so the entries behind each origin (t < 0) must still count
    as containers: the two-sided walk."""
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    ids = []
    for tr, ri in (((2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 1), 1.5),
                   ((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.25, 0, 0, 0, 1), 2.0),
                   ((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.25, 0, 0, 0, 1), 2.5)):
        ids.append(b.sphere(transform=tr, material=(0.1, 0.9, 0.9, 200.0, 0.0, 1.0, ri)))
    renderer.upload(b)
    zs = [-4.0, -1.5, -1.0, -0.5, 0.8, 1.5]
    want = [(1.0, 1.5), (1.5, 2.0), (2.0, 2.5), (2.5, 2.5), (2.5, 1.5), (1.5, 1.0)]
    h = renderer.hit_at([(0, 0, z) for z in zs], [(0, 0, 1)] * len(zs))
    assert [(float(r["n1"]), float(r["n2"])) for r in h] == want
    assert h["object"].tolist() == [ids[0], ids[1], ids[2], ids[1], ids[2], ids[0]]
    assert h["inside"].tolist() == [0, 0, 0, 1, 1, 1]
    assert renderer.last_stats()["n1n2_scans"] == len(zs)


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_scene_hits_equal_the_oracle(R, renderer, seed):
    """scene_fuzz.build(seed), every category three times (flat, LDS and global culls, groups, general shapes,
    glass, far cameras), 33 x 17 samples (partial tiles on both edges): hit_at on the camera's rays and the
    render_aov planes against the oracle's hit + prepare_computations of every sample."""
    import oracle

    P, spec, _, cat = F.build(seed)
    Hs, V = 33, 17
    cam, ocam = F.cameras(P, spec, Hs, V)
    renderer.upload(P.b)
    rays = camera_rays(oracle, ocam)
    want = oracle_hits(R, P.o, rays, {v: k for k, v in P.ids.items()})
    got = renderer.hit_at(*batch(rays))
    st = renderer.last_stats()
    try:
        assert_records_equal(got, want, f"seed {seed} ({cat}) hit_at")
        hits = int((want["object"] >= 0).sum())
        assert (st["rays"], st["samples"], st["n1n2_scans"]) == (Hs * V, Hs * V, hits), st
        assert st["shadow_rays"] == 0 and st["shade_events"] == 0 and st["nan_rays"] == 0
        aov = renderer.render_aov(cam, planes=("depth", "normal", "object"))
        depth, normal, obj = planes_of(want, V, Hs)
        assert same(aov["object"], obj), f"seed {seed} ({cat}): object plane"
        assert same(aov["depth"], depth), f"seed {seed} ({cat}): depth plane"
        assert same(aov["normal"], normal), f"seed {seed} ({cat}): normal plane"
        s2 = aov["stats"]
        assert (s2["rays"], s2["samples"], s2["n1n2_scans"], s2["shadow_rays"], s2["shade_events"]) == \
            (Hs * V, Hs * V, 0, 0, 0), s2
    except AssertionError:
        print("\n".join(P.log))
        raise


@pytest.mark.parametrize("seed", range(24))
def test_general_fuzz_scene_hits_equal_the_oracle(R, renderer, seed):
    """scene_fuzz.build_general(seed), every family four times (cones, tori, CSG, patterns, textures, mixed), 33 x 17
    samples: hit_at on the camera's rays and the render_aov planes against the oracle's hit + prepare_computations
    of every sample.  Seeds 1 and 19 hold the reference's spurious far-torus roots."""
    import oracle

    P, spec, _, cat = F.build_general(seed)
    Hs, V = 33, 17
    cam, ocam = F.cameras(P, spec, Hs, V)
    renderer.upload(P.b)
    rays = camera_rays(oracle, ocam)
    want = oracle_hits(R, P.o, rays, {v: k for k, v in P.ids.items()})
    got = renderer.hit_at(*batch(rays))
    st = renderer.last_stats()
    try:
        assert_records_equal(got, want, f"general seed {seed} ({cat}) hit_at")
        hits = int((want["object"] >= 0).sum())
        assert (st["rays"], st["samples"], st["n1n2_scans"]) == (Hs * V, Hs * V, hits), st
        assert st["shadow_rays"] == 0 and st["shade_events"] == 0 and st["nan_rays"] == 0
        aov = renderer.render_aov(cam, planes=("depth", "normal", "object"))
        depth, normal, obj = planes_of(want, V, Hs)
        assert same(aov["object"], obj), f"seed {seed} ({cat}): object plane"
        assert same(aov["depth"], depth), f"seed {seed} ({cat}): depth plane"
        assert same(aov["normal"], normal), f"seed {seed} ({cat}): normal plane"
        s2 = aov["stats"]
        assert (s2["rays"], s2["samples"], s2["n1n2_scans"], s2["shadow_rays"], s2["shade_events"]) == \
            (Hs * V, Hs * V, 0, 0, 0), s2
    except AssertionError:
        print("\n".join(P.log))
        raise


def _albedo_pair(R):
    """A checker floor, a striped transformed sphere inside a scaled group and a solid sphere, through the product's
    SceneBuilder and the oracle side by side -> (builder, oracle, camera transform, {builder id: oracle id},
    {builder id: oracle pattern id})."""
    import oracle

    M = oracle.Oracle.mat
    b, o = R.SceneBuilder(), oracle.Oracle()
    b.point_light((-10, 10, -10), (1, 1, 1))
    o.point_light((-10, 10, -10), (1, 1, 1))
    ids, pats = {}, {}
    mat = (0.1, 0.9, 0.9, 200.0, 0.0, 0.0, 1.0)
    white, black, red = (1, 1, 1), (0.1, 0.1, 0.1), (0.9, 0.2, 0.1)
    grey = (0.7, 0.7, 0.7)
    # floor: checker with a scaled, rotated pattern transform
    pt = M.multiply(M.rotate("y", 0.3), M.scale(0.7, 0.7, 0.7))
    ft = M.translate(0, -1.0, 0)
    bp = b.pattern("checker", a=b.pattern("solid", color=grey), b=b.pattern("solid", color=black), transform=pt)
    op = o.pattern("checker", a=o.pattern("solid", color=grey), b=o.pattern("solid", color=black), transform=pt)
    bid = b.plane(transform=ft, material=mat, pattern=bp)
    ids[bid], pats[bid] = o.add("plane", transform=ft, material=mat, pattern=op), op
    # a striped sphere, itself transformed, inside a scaled group
    gt = M.multiply(M.translate(-0.8, 0.2, 0.5), M.scale(1.5, 0.8, 1.2))
    bg = b.group(transform=gt)
    og = o.add("group", transform=gt)
    ids[bg] = og
    st = M.multiply(M.translate(0.1, 0.5, 0.0), M.multiply(M.rotate("z", 0.4), M.scale(0.9, 1.1, 0.8)))
    spt = M.multiply(M.rotate("z", 0.7), M.scale(0.25, 0.25, 0.25))
    bp = b.pattern("stripe", a=b.pattern("solid", color=red), b=b.pattern("solid", color=white), transform=spt)
    op = o.pattern("stripe", a=o.pattern("solid", color=red), b=o.pattern("solid", color=white), transform=spt)
    bid = b.sphere(transform=st, material=mat, pattern=bp, parent=bg)
    ids[bid], pats[bid] = o.add("sphere", parent=og, transform=st, material=mat, pattern=op), op
    # a solid sphere
    t3 = M.multiply(M.translate(1.4, 0.0, -0.3), M.scale(0.7, 0.7, 0.7))
    bp = b.pattern("solid", color=(0.2, 0.4, 0.8))
    op = o.pattern("solid", color=(0.2, 0.4, 0.8))
    bid = b.sphere(transform=t3, material=mat, pattern=bp)
    ids[bid], pats[bid] = o.add("sphere", transform=t3, material=mat, pattern=op), op
    cam_t = M.view_transform((0.3, 1.5, -6.0), (0, 0.2, 0), (0, 1, 0))
    return b, o, cam_t, ids, pats


def test_albedo_plane_equals_the_oracle_pattern(R, renderer):
    """The albedo plane is material.pattern_at_object(object, over_point) as shade_hit's lighting reads it
    (material.rs:77-80): per sample, oracle.pattern_at(pattern, world_to_object(object, over_point)) — the oracle's
    pattern_at takes the object-space point and applies the pattern's own transform, like Pattern::pattern_at."""
    import oracle

    b, o, cam_t, ids, pats = _albedo_pair(R)
    renderer.upload(b)
    Hs, V = 24, 16
    cam = R.camera(Hs, V, math.pi / 3, cam_t)
    ocam = oracle.Oracle.camera(Hs, V, math.pi / 3, cam_t)
    want = oracle_hits(R, o, camera_rays(oracle, ocam), {v: k for k, v in ids.items()})
    albedo = np.zeros((V * Hs, 3))
    for i, rec in enumerate(want):
        if rec["object"] >= 0:
            p = o.world_to_object(ids[int(rec["object"])], rec["over_point"].tolist())
            albedo[i] = o.pattern_at(pats[int(rec["object"])], p[:3])
    got = renderer.render_aov(cam)
    depth, normal, obj = planes_of(want, V, Hs)
    assert same(got["object"], obj) and same(got["depth"], depth) and same(got["normal"], normal)
    assert len(set(obj.reshape(-1).tolist())) == 4  # the floor, both spheres and the sky are in view
    assert same(got["albedo"], albedo.reshape(V, Hs, 3))
    assert len({tuple(c) for c in albedo.tolist()}) >= 6  # both colours of each pattern, the solid, the sky's zeros


def test_batch_sizes_around_a_wave(R, renderer):
    """1, 63, 64, 65 and 257 copies of one ray (a short wave, a full one, one lane more, more than a block): the
    same record every time."""
    b, _, _ = default_scene(R)
    renderer.upload(b)
    o, d = (0.1, 0.2, -5.0), (0.0, 0.0, 1.0)
    one = renderer.hit_at([o], [d])
    assert one["object"][0] >= 0
    for n in (63, 64, 65, 257):
        h = renderer.hit_at([o] * n, [d] * n)
        assert len(h) == n
        assert_records_equal(h, np.repeat(one, n), f"{n} copies")
    assert len(renderer.hit_at(np.zeros((0, 3)), np.zeros((0, 3)))) == 0


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (9, 7), (24, 16)])
def test_small_and_partial_frames(R, renderer, size):
    """Frames of one sample, one full tile, partial tiles on both edges and several full tiles (the tile-bundle path):
    the planes equal hit_at on the oracle's camera rays."""
    import oracle

    b, _, _ = default_scene(R)
    renderer.upload(b)
    Hs, V = size
    t = oracle.Oracle.mat.view_transform((0.5, 1.0, -4.0), (0, 0, 0), (0, 1, 0))
    cam, ocam = R.camera(Hs, V, 1.0, t), oracle.Oracle.camera(Hs, V, 1.0, t)
    h = renderer.hit_at(*batch(camera_rays(oracle, ocam)))
    aov = renderer.render_aov(cam, planes=("depth", "normal", "object"))
    depth, normal, obj = planes_of(h, V, Hs)
    assert aov["depth"].shape == (V, Hs) and aov["normal"].shape == (V, Hs, 3) and aov["object"].dtype == np.int32
    assert same(aov["object"], obj) and same(aov["depth"], depth) and same(aov["normal"], normal)
    assert sorted(aov) == ["depth", "normal", "object", "stats"]  # unrequested planes are not returned


def _group_scene(R):
    """a group scene of more than 8 nodes: the bundle walk and, for full tiles, the cached tile bundles"""
    P, spec, _, _ = F.build(3)  # "groups"
    return P, spec


@pytest.mark.parametrize("seed", [1, 3, 6, 7])
def test_full_tile_frames_walk_with_the_cached_bundles(R, renderer, seed):
    """24 x 16 samples are six full 8 x 8 tiles: one wave per tile, culled with the context's cached tile bundles (a far
    camera, groups, global culls, general shapes).  The planes must equal hit_at on the same rays — the batch path,
    which builds its bundles in the walk and is held to the oracle above — and the hits the oracle finds."""
    import oracle

    P, spec, _, cat = F.build(seed)
    Hs, V = 24, 16
    cam, ocam = F.cameras(P, spec, Hs, V)
    renderer.upload(P.b)
    rays = camera_rays(oracle, ocam)
    h = renderer.hit_at(*batch(rays))
    assert_records_equal(h, oracle_hits(R, P.o, rays, {v: k for k, v in P.ids.items()}), f"seed {seed} ({cat})")
    for _ in range(2):  # the second frame reuses the cached table
        aov = renderer.render_aov(cam, planes=("depth", "normal", "object"))
        depth, normal, obj = planes_of(h, V, Hs)
        assert same(aov["object"], obj) and same(aov["depth"], depth) and same(aov["normal"], normal), (seed, cat)


def test_nan_rays_return_rr_e_nan(R, renderer):
    """A ray with a NaN direction against two planes has two NaN entries, where the reference's sort panics
    (scene.rs:104): RR_E_NAN, with the rays counted, from the batch and from a frame through a NaN camera."""
    b = R.SceneBuilder()
    b.point_light((-10, 10, -10), (1, 1, 1))
    b.plane()
    b.plane(transform=(1, 0, 0, 0, 0, 1, 0, -1, 0, 0, 1, 0, 0, 0, 0, 1))
    renderer.upload(b)
    with pytest.raises(R.RRError) as e:
        renderer.hit_at([(0, 1, -5), (0, 1, -5)], [(0, -1, 1), (0, math.nan, 1)])
    assert e.value.code == R._lib.RR_E_NAN
    st = renderer.last_stats()
    assert st["nan_rays"] == 1 and st["rays"] == 2
    nan_cam = R.camera(8, 8, 1.0, tuple([math.nan] * 12 + [0.0, 0.0, 0.0, 1.0]))
    with pytest.raises(R.RRError) as e:
        renderer.render_aov(nan_cam, planes=("depth",))
    assert e.value.code == R._lib.RR_E_NAN
    assert renderer.last_stats()["nan_rays"] == 64


def test_aa_only_has_to_divide_the_camera(R, renderer):
    P, spec = _group_scene(R)
    renderer.upload(P.b)
    cam, _ = F.cameras(P, spec, 24, 16)
    a = renderer.render_aov(cam, aa=2)  # a 12 x 8 image's samples
    b = renderer.render_aov(cam, aa=1)
    for k in ("depth", "normal", "object", "albedo"):
        assert a[k].shape[:2] == (16, 24) and same(a[k], b[k]), k
    with pytest.raises(R.RRError) as e:
        renderer.render_aov(cam, aa=5)
    assert e.value.code == R._lib.RR_E_ARG


def test_device_planes_on_a_torch_stream(R, renderer):
    """rr_render_aov_device into torch tensors on a non-default stream, synchronised, equals the host call."""
    P, spec = _group_scene(R)
    renderer.upload(P.b)
    Hs, V = 40, 24
    cam, _ = F.cameras(P, spec, Hs, V)
    ref = renderer.render_aov(cam)
    dev = torch.device("cuda", 0)
    depth = torch.full((V, Hs), -1.0, dtype=torch.float64, device=dev)
    normal = torch.full((V, Hs, 3), -1.0, dtype=torch.float64, device=dev)
    obj = torch.full((V, Hs), -7, dtype=torch.int32, device=dev)
    albedo = torch.full((V, Hs, 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    renderer.render_aov_device(cam, opts, ("depth", "normal", "object", "albedo"), depth.data_ptr(), normal.data_ptr(),
                               obj.data_ptr(), albedo.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert same(depth.cpu().numpy(), ref["depth"]) and same(normal.cpu().numpy(), ref["normal"])
    assert same(obj.cpu().numpy(), ref["object"]) and same(albedo.cpu().numpy(), ref["albedo"])
    st = renderer.last_stats()
    assert st["rays"] == st["samples"] == Hs * V and st["kernel_ms"] > 0
    # an unrequested plane's pointer is ignored: nothing is written there
    obj.fill_(-7)
    torch.cuda.synchronize(dev)
    renderer.render_aov_device(cam, opts, R._lib.RR_AOV_DEPTH, depth.data_ptr(), None, obj.data_ptr(), None,
                               stream.cuda_stream)
    stream.synchronize()
    assert bool((obj == -7).all().item()) and same(depth.cpu().numpy(), ref["depth"])


def test_colour_frames_are_undisturbed_by_queries(R, renderer):
    """A colour render before and after an AOV frame and a hit batch: identical canvases and counters (the queries
    count into their own buffer and reuse the cached tile bundles without changing them)."""
    P, spec = _group_scene(R)
    renderer.upload(P.b)
    cam, _ = F.cameras(P, spec, 32, 24)
    first = renderer.render(cam, aa=1, max_depth=3, canvas=True)
    again = renderer.render(cam, aa=1, max_depth=3, canvas=True)
    renderer.render_aov(cam)
    renderer.hit_at([(0, 0, -5)], [(0, 0, 1)])
    after = renderer.render(cam, aa=1, max_depth=3, canvas=True)
    assert same(first["canvas"], again["canvas"]) and same(first["canvas"], after["canvas"])
    assert same(first["avg"], after["avg"])
    keys = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples", "prim_tests")
    assert [after["stats"][k] for k in keys] == [again["stats"][k] for k in keys]


def test_virtual_multi_device_context_answers_like_one(R, renderer):
    P, spec = _group_scene(R)
    o = [(0.0, 1.0, -25.0)] * 70
    d = [tuple(v) for v in (np.array([[x, -0.05, 1.0] for x in np.linspace(-0.3, 0.3, 70)]))]
    renderer.upload(P.b)
    want = renderer.hit_at(o, d)
    m = R.Renderer.virtual(0, 2)
    try:
        m.upload(P.b)
        got = m.hit_at(o, d)
        cam, _ = F.cameras(P, spec, 16, 8)
        aov = m.render_aov(cam, planes=("object",))
    finally:
        m.close()
    assert_records_equal(got, want, "virtual context")
    assert same(aov["object"], renderer.render_aov(cam, planes=("object",))["object"])


def test_refused_arguments(R, renderer):
    b, _, _ = default_scene(R)
    renderer.upload(b)
    cam = R.camera(16, 8, 1.0)
    for kw in ({"part": 1, "nparts": 2}, {"band": (0, 4)}, {"nparts": 2}):
        with pytest.raises(R.RRError) as e:
            renderer.render_aov(cam, **kw)
        assert e.value.code == R._lib.RR_E_ARG, kw
    L, D = R.lib(), R._lib._D
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    depth = np.zeros((8, 16))
    args = (renderer.h, ctypes.byref(cam), ctypes.byref(opts))
    # a requested plane with a null buffer; an unrequested one may be null
    assert L.rr_render_aov(*args, R._lib.RR_AOV_DEPTH | R._lib.RR_AOV_OBJECT, depth.ctypes.data_as(D), None, None, None,
                           None) == R._lib.RR_E_ARG
    assert L.rr_render_aov(*args, R._lib.RR_AOV_DEPTH, depth.ctypes.data_as(D), None, None, None, None) == 0
    assert L.rr_render_aov(*args, 0, None, None, None, None, None) == R._lib.RR_E_ARG
    assert L.rr_render_aov(*args, 16, None, None, None, None, None) == R._lib.RR_E_ARG
    with pytest.raises(R.RRError) as e:
        renderer.render_aov_device(cam, opts, ("normal",))
    assert e.value.code == R._lib.RR_E_ARG
    # max_depth is ignored, even out of a colour frame's range
    deep = R._lib.RenderOpts(1, 99, 0, 0, 0, 1, 8, 0, 0, 0)
    assert L.rr_render_aov(renderer.h, ctypes.byref(cam), ctypes.byref(deep), R._lib.RR_AOV_DEPTH,
                           depth.ctypes.data_as(D), None, None, None, None) == 0
    # no scene: nothing is launched
    fresh = R.Renderer(0)
    try:
        with pytest.raises(R.RRError) as e:
            fresh.hit_at([(0, 0, -5)], [(0, 0, 1)])
        assert e.value.code == R._lib.RR_E_ARG and "no scene" in str(e.value)
        with pytest.raises(R.RRError) as e:
            fresh.render_aov(cam)
        assert e.value.code == R._lib.RR_E_ARG and "no scene" in str(e.value)
        with pytest.raises(R.RRError) as e:
            fresh.render_aov_device(cam, opts, ("depth",))
        assert e.value.code == R._lib.RR_E_ARG and "no scene" in str(e.value)
    finally:
        fresh.close()
