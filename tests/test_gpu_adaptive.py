"""Adaptive anti-aliasing on the GPU (rr_render_adaptive).  The feature has an exact definition, so
every test builds its reference from calls the rest of the suite already pins to the oracle:

    F1 = render(camera(W, H), aa=1)["avg"]          the probe
    FN = render(camera(W*aa, H*aa), aa)["avg"]      the full frame
    M  = adaptive_mask(F1, thr)                     the criterion, in numpy

and asserts, bit for bit (np.array_equal, NaN equal to NaN): frame == where(M, FN, F1), mask == M, n_refined == M.sum().
No tolerance applies anywhere."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")
COUNTERS = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples")


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
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def cameras(R, cam_like, W, H, aa):
    """(the aa 1 probe camera, the full camera) of one view"""
    t = list(cam_like.transform)
    return R.camera(W, H, cam_like.field_of_view, t), R.camera(W * aa, H * aa, cam_like.field_of_view, t)


def references(R, renderer, cam_like, W, H, aa, max_depth=5, seed=0):
    c1, cn = cameras(R, cam_like, W, H, aa)
    f1 = renderer.render(c1, aa=1, max_depth=max_depth, seed=seed)
    fn = renderer.render(cn, aa=aa, max_depth=max_depth, seed=seed)
    return cn, f1, fn


def check_identity(R, got, f1, fn, thr, what, partial=False):
    """got == where(M, FN, F1) with the mask and the count; returns the mask"""
    M = R.adaptive_mask(f1["avg"], thr)
    frac = M.mean()
    print(f"{what}: thr {thr}: {int(M.sum())} of {M.size} pixels refined ({frac:.3f}); "
          f"differing pixels {int((~(got['avg'] == np.where(M[..., None], fn['avg'], f1['avg']))).any(axis=2).sum())}")
    assert same(got["mask"], M.astype(np.uint8)), what
    assert got["n_refined"] == int(M.sum()), what
    assert same(got["avg"], np.where(M[..., None], fn["avg"], f1["avg"])), what
    assert got["stats"]["samples"] == f1["stats"]["samples"] + (fn["stats"]["samples"] // M.size) * int(M.sum()), what
    if partial:  # a mask that is empty or full proves only half
        assert 0 < got["n_refined"] < M.size, (what, got["n_refined"])
    return M


def yaml_scene(R, name, W, H, aa, root=SCENES):
    return R.YamlScene(open(os.path.join(root, name)).read(), W, H, aa, obj_root=root)


def translate(x, y, z):
    return [1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1]


def scale_at(s, x, y, z):
    return [s, 0, 0, x, 0, s, 0, y, 0, 0, s, z, 0, 0, 0, 1]


def csg_scene(R):
    """a lens (the intersection of two spheres) and a cube minus a sphere over a checker floor: general kernels (G = 2)"""
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


def checker_scene(R):
    """a two-colour checker plane and one reflective sphere (flat scene, reflection chains)"""
    b = R.SceneBuilder()
    b.point_light((-5, 6, 2), (1, 1, 1))
    b.plane(transform=translate(0, -1, 0), material=(0.1, 0.9, 0.0, 200.0, 0.0, 0.0, 1.0),
            pattern=b.pattern("checker", a=b.pattern("solid", color=(1, 1, 1)), b=b.pattern("solid", color=(0, 0, 0))))
    b.sphere(transform=translate(0.3, 0, -4), material=(0.1, 0.7, 0.3, 100.0, 0.4, 0.0, 1.0),
             pattern=b.pattern("solid", color=(0.9, 0.3, 0.2)))
    return b, R.camera(8, 8, math.pi / 3, translate(0, -0.5, 0))


# (id, scene source, W, H, aa, max_depth, seed): one row per kernel family of the production dispatch
FAMILIES = [
    ("c2_flat_fused_level0", "c2_s1024.yaml", 96, 54, 2, 5, 0),
    ("c3_chain_aa3_pixel_waves", "c3_s1024_reflect.yaml", 96, 54, 3, 5, 0),
    ("c1_tree", "c1_readme.yaml", 40, 30, 2, 5, 0),
    ("c4_groups", "c4_teapot.yaml", 64, 36, 2, 5, 0),
    ("c5_area_light_jitter", "c5_area_light.yaml", 32, 16, 2, 5, 12345),
    ("cube_general", "objects_cube.yaml", 40, 30, 2, 5, 0),
    ("csg_general", None, 40, 30, 2, 5, 0),
    ("c3_depth0_fused_level0", "c3_s1024_reflect.yaml", 96, 54, 3, 0, 0),
]


@pytest.mark.parametrize("name,src,W,H,aa,depth,seed", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_selection_identity_per_kernel_family(R, renderer, name, src, W, H, aa, depth, seed):
    thr = 0.25
    if src is None:
        scene, cam_like = csg_scene(R)
    else:
        scene = yaml_scene(R, src, W, H, aa, GOLDEN if src == "objects_cube.yaml" else SCENES)
        cam_like = scene.camera
    renderer.upload(scene)
    cn, f1, fn = references(R, renderer, cam_like, W, H, aa, depth, seed)
    got = renderer.render_adaptive(cn, aa, thr, max_depth=depth, seed=seed, jitter_mode=0)
    check_identity(R, got, f1, fn, thr, name, partial=True)


def test_extremes_refine_all_and_none(R, renderer):
    scene = yaml_scene(R, "c3_s1024_reflect.yaml", 48, 27, 3)
    renderer.upload(scene)
    cn, f1, fn = references(R, renderer, scene.camera, 48, 27, 3)
    every = renderer.render_adaptive(cn, 3, -1.0)
    assert same(every["avg"], fn["avg"]) and every["mask"].all() and every["n_refined"] == 48 * 27
    for k in COUNTERS:  # the probe's plus the refine pass's, which is the full frame's work
        assert every["stats"][k] == f1["stats"][k] + fn["stats"][k], k
    none = renderer.render_adaptive(cn, 3, math.inf)
    assert same(none["avg"], f1["avg"]) and not none["mask"].any() and none["n_refined"] == 0
    for k in COUNTERS:
        assert none["stats"][k] == f1["stats"][k], k


@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1), (7, 5), (67, 3)])
def test_shapes_where_index_arithmetic_breaks(R, renderer, W, H):
    scene, cam_like = checker_scene(R)
    renderer.upload(scene)
    c1 = cameras(R, cam_like, W, H, 1)[0]
    f1 = renderer.render(c1, aa=1)
    for aa in (1, 2, 3, 4, 5, 8, 9):
        cn = cameras(R, cam_like, W, H, aa)[1]
        fn = renderer.render(cn, aa=aa)
        for thr in (-1.0, 0.25):
            got = renderer.render_adaptive(cn, aa, thr)
            check_identity(R, got, f1, fn if aa > 1 else f1, thr, f"{W}x{H} aa {aa}")


def test_compaction_across_blocks(R, renderer):
    """C2 at 160 x 90: 57 scan blocks.  The oracle's aa 1 frame of this view lists 9024 pixels at thr 0.25 (a multiple of
    64) and 9803 at thr 0.2 (no multiple of 7, 16 or 64): the second is the ragged list."""
    W, H, aa = 160, 90, 2
    scene = yaml_scene(R, "c2_s1024.yaml", W, H, aa)
    renderer.upload(scene)
    cn, f1, fn = references(R, renderer, scene.camera, W, H, aa)
    assert W * H > 32 * 256
    for thr in (0.25, 0.2):
        got = renderer.render_adaptive(cn, aa, thr)
        M = check_identity(R, got, f1, fn, thr, "c2 160x90", partial=True)
    n = int(M.sum())
    assert all(n % k for k in (7, 16, 64)), n


def test_determinism_of_frame_mask_and_stats(R, renderer):
    scene = yaml_scene(R, "c4_teapot.yaml", 64, 36, 2)
    renderer.upload(scene)
    a = renderer.render_adaptive(scene.camera, 2, 0.25)
    b = renderer.render_adaptive(scene.camera, 2, 0.25)
    assert same(a["avg"], b["avg"]) and same(a["mask"], b["mask"]) and a["n_refined"] == b["n_refined"] > 0
    sa, sb = dict(a["stats"]), dict(b["stats"])
    sa.pop("kernel_ms"), sb.pop("kernel_ms")
    assert sa == sb  # prim_tests and wave_visits too: the refine pass's waves hold the same samples


def test_context_hygiene_around_an_adaptive_frame(R):
    r = R.Renderer(0)  # a fresh context: its workspace and caches see only these three frames
    try:
        scene = yaml_scene(R, "c3_s1024_reflect.yaml", 48, 27, 3)
        r.upload(scene)
        before = r.render(scene.camera, aa=3)
        mid = r.render_adaptive(scene.camera, 3, 0.25)
        after = r.render(scene.camera, aa=3)
        assert 0 < mid["n_refined"] < 48 * 27
        assert same(before["avg"], after["avg"])
        sa, sb = dict(before["stats"]), dict(after["stats"])
        sa.pop("kernel_ms"), sb.pop("kernel_ms")
        assert sa == sb
    finally:
        r.close()


def test_device_variant_on_a_torch_stream(R, renderer):
    W, H, aa, thr = 64, 36, 2, 0.25
    scene = yaml_scene(R, "c4_teapot.yaml", W, H, aa)
    renderer.upload(scene)
    host = renderer.render_adaptive(scene.camera, aa, thr)
    dev = torch.device("cuda", 0)
    avg = torch.full((H, W, 3), -1.0, dtype=torch.float64, device=dev)
    mask = torch.full((H, W), 7, dtype=torch.uint8, device=dev)
    n = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    o = R._lib.RenderOpts(aa, 5, 0, 0, 0, 1, 8, 0, 0, 0)
    renderer.render_adaptive_device(scene.camera, o, thr, avg.data_ptr(), mask.data_ptr(), n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert same(avg.cpu().numpy(), host["avg"]) and same(mask.cpu().numpy(), host["mask"])
    assert int(n.item()) == host["n_refined"] > 0
    st = renderer.last_stats()
    assert st["samples"] == W * H + aa * aa * host["n_refined"]
    # the optional outputs left out
    avg2 = torch.full((H, W, 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    renderer.render_adaptive_device(scene.camera, o, thr, avg2.data_ptr(), None, None, stream.cuda_stream)
    stream.synchronize()
    assert same(avg2.cpu().numpy(), host["avg"])


def test_refusals_on_a_live_context(R, renderer):
    L, E = R.lib(), R._lib
    scene = yaml_scene(R, "c1_readme.yaml", 16, 8, 2)
    renderer.upload(scene)
    cam = scene.camera
    avg = np.zeros((8, 16, 3))
    D = E._D

    def call(h, opts, thr=0.25, out=avg):
        return L.rr_render_adaptive(h, C.byref(cam), C.byref(opts), thr, out.ctypes.data_as(D) if out is not None else None,
                                    None, None, None)

    ok = E.RenderOpts(2, 5, 0, 0, 0, 1, 8, 0, 0, 0)
    assert call(renderer.h, ok) == 0
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 1, 2, 8, 0, 0, 0)) == E.RR_E_ARG  # a part
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 0, 2, 8, 0, 0, 0)) == E.RR_E_ARG
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 0, 1, 8, 0, 0, 4)) == E.RR_E_ARG  # a band
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_CANVAS, 0, 0)) == E.RR_E_ARG
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG_F32, 0, 0)) == E.RR_E_ARG
    assert call(renderer.h, E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_NO_FRAME_TIMING, 0, 0)) == 0
    assert call(renderer.h, ok, thr=math.nan) == E.RR_E_ARG
    assert call(renderer.h, ok, out=None) == E.RR_E_ARG
    assert call(renderer.h, E.RenderOpts(2, 99, 0, 0, 0, 1, 8, 0, 0, 0)) == E.RR_E_LIMIT  # as rr_render
    v = R.Renderer.virtual(0, 2)
    try:
        v.upload(scene)
        assert call(v.h, ok) == E.RR_E_ARG
        assert "single-device" in L.rr_last_error().decode()
    finally:
        v.close()
    empty = R.Renderer(0)
    try:
        assert call(empty.h, ok) == E.RR_E_ARG
        assert "no scene" in L.rr_last_error().decode()
    finally:
        empty.close()
