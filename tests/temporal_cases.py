"""Frames, cameras and parameter sets shared by the temporal accumulation's host and GPU tests (test_temporal_host.py,
test_gpu_temporal.py): the same case product on both sides, each frame and each expectation built once per process.
Also the small oracle helpers of the geometry tests (first-hit planes of a camera from prepare_computations)."""
import functools
import itertools
import math

import numpy as np

# (W, H): one pixel; smaller than a tile; odd sizes that cross a tile's edge in y (9 > 8 rows); a row longer than a
# wave's run of 64 with a partial last tile
FRAMES = ((1, 1), (7, 5), (13, 9), (65, 3))
CHANNELS = (1, 3)
MOMENTS = (False, True)
ALPHAS = (0.0, 0.2)
HISTORIES = (1, 4, 2**20)
CAMERAS = ("static", "small", "large", "rotated", "away")
# name -> (Temporal keywords, the optional planes passed in (current, previous)).  Each optional plane on and off: no
# plane at all; the object planes as void markers only and as a term; the current normal alone (the plane term); both
# normals (plane and normal terms); everything.
COMBOS = {
    "none": (dict(sigma_plane=0.0, sigma_normal=0.0, object=False), ((), ())),
    "object_void": (dict(sigma_plane=0.0, sigma_normal=0.0, object=False), (("object",), ("object",))),
    "object": (dict(sigma_plane=0.0, sigma_normal=0.0, object=True), (("object",), ("object",))),
    "plane": (dict(sigma_plane=0.004, sigma_normal=0.0, object=False), (("normal",), ())),
    "normal": (dict(sigma_plane=0.0, sigma_normal=0.02, object=False), (("normal",), ("normal",))),
    "all": (dict(sigma_plane=0.004, sigma_normal=0.02, object=True), (("normal", "object"), ("normal", "object"))),
}
FOV = math.pi / 3


def _matmul(*ms):
    out = np.eye(4)
    for m in ms:
        out = out @ np.array(m, np.float64).reshape(4, 4)
    return [float(v) for v in out.reshape(-1)]


def translate(x, y, z):
    return [1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1]


def rot_y(a):
    return [math.cos(a), 0, math.sin(a), 0, 0, 1, 0, 0, -math.sin(a), 0, math.cos(a), 0, 0, 0, 0, 1]


def rot_z(a):
    return [math.cos(a), -math.sin(a), 0, 0, math.sin(a), math.cos(a), 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


# world -> camera transforms.  The synthetic frames lie about 5 units in front of BASE; a pixel there is between 0.09
# (W = 65) and 5.8 (W = 1) units wide
BASE = translate(0.1, -0.2, 0.3)
PREV = {
    "static": BASE,
    "small": _matmul(translate(0.31, -0.17, 0.01), BASE),  # a few pixels at most
    "large": _matmul(translate(2.5, 0.6, -0.02), BASE),  # part of the frame leaves
    "rotated": _matmul(rot_z(0.1), rot_y(0.05), translate(-0.2, 0.1, 0.0), BASE),
    "away": _matmul(rot_y(math.pi), BASE),  # every point lies behind it: c[2] >= 0
}


def cameras(R, W, H, name):
    """(current, previous) cameras of a case"""
    return R.camera(W, H, FOV, BASE), R.camera(W, H, FOV, PREV[name])


def _planes(rng, W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    # a bumpy wall about 5 units in front of the camera (depth is measured along the pixel's ray), so that the planes of
    # two cameras that differ by a sideways move roughly agree and the plane term passes some taps and rejects others
    import rray_amd as R

    cam = R.camera(W, H, FOV, BASE)
    wx, wy = cam.half_width - (x + 0.5) * cam.pixel_size, cam.half_height - (y + 0.5) * cam.pixel_size
    depth = (5.0 + 0.05 * np.sin(0.3 * x + 0.2 * y) + 0.003 * rng.random((H, W))) * np.sqrt((wx * wx + wy * wy) + 1.0)
    normal = np.stack([0.1 * np.sin(0.4 * x) + 0.08 * rng.normal(size=(H, W)), 0.1 * np.cos(0.3 * y) +
                       0.08 * rng.normal(size=(H, W)), np.ones((H, W))], axis=2)
    normal /= np.sqrt((normal * normal).sum(axis=2, keepdims=True))
    obj = ((x >= W // 2).astype(np.int32) + 2 * (y >= (2 * H) // 3).astype(np.int32)).astype(np.int32)
    return depth, normal, obj


@functools.lru_cache(maxsize=None)
def frame(W, H):
    """A seeded pair of frames of W x H: dict of img1 / img3, depth, normal, object (the current frame) and prev_img1 /
    prev_img3, prev_m21 / prev_m23, prev_depth, prev_normal, prev_object, prev_n (the history).  The definition's edge
    cases wherever the frame has room: void pixels by depth, by object and by a NaN depth in both frames; NaN and inf
    in both images; a NaN normal component; history counts of 0, of more than RR_MAX_TEMPORAL_HISTORY and of INT32_MAX."""
    rng = np.random.default_rng(7000 * W + H)
    depth, normal, obj = _planes(rng, W, H)
    pdepth, pnormal, pobj = _planes(rng, W, H)
    img3 = 0.5 + 0.25 * rng.normal(size=(H, W, 3))
    img1 = np.clip(0.6 + 0.3 * rng.normal(size=(H, W)), 0.0, 1.0)
    pimg3 = 0.5 + 0.1 * rng.normal(size=(H, W, 3))
    pimg1 = np.clip(0.6 + 0.1 * rng.normal(size=(H, W)), 0.0, 1.0)
    pm23, pm21 = pimg3 * pimg3 + 0.01 * rng.random((H, W, 3)), pimg1 * pimg1 + 0.01 * rng.random((H, W))
    pn = rng.integers(0, 7, size=(H, W)).astype(np.int32)  # about one count in seven is 0
    if W * H >= 35:
        a, b = min(3, H - 1), min(4, H - 1)  # rows 3 and 4, or the last row of a lower frame
        depth[0, W - 1] = np.inf  # void by depth
        obj[1, 2] = -1  # void by object (where the object plane is passed)
        depth[2, 1] = np.nan  # a NaN depth is void
        pdepth[1, 3], pobj[2, 3], pdepth[a, 2] = np.inf, -1, np.nan
        img3[a, 4, 1], img1[a, 4] = np.nan, np.nan
        img3[b, 5], img1[b, 5] = np.inf, np.inf
        pimg3[2, 5, 0], pimg1[2, 5], pm23[2, 5, 2], pm21[2, 5] = np.nan, np.nan, np.inf, np.inf
        pimg3[0, 0], pimg1[0, 0] = -np.inf, -np.inf
        normal[b, 1, 0], pnormal[b, 4, 2] = np.nan, np.nan
        pn[0, 1], pn[1, 1], pn[a, 5], pn[b, 0] = 0, 2**20 + 5, 2**31 - 1, -3
    out = dict(img1=img1, img3=img3, depth=depth, normal=normal, object=obj, prev_img1=pimg1, prev_img3=pimg3,
               prev_m21=pm21, prev_m23=pm23, prev_depth=pdepth, prev_normal=pnormal, prev_object=pobj, prev_n=pn)
    for v in out.values():
        v.setflags(write=False)
    return out


def cases(W, H):
    """(C, combo, moments, alpha, max_history, camera) of the whole product for one frame size"""
    return list(itertools.product(CHANNELS, COMBOS, MOMENTS, ALPHAS, HISTORIES, CAMERAS))


def arguments(R, W, H, C, combo, moments, alpha, max_history, camera):
    """(args, kwargs) of Renderer.temporal / temporal_reference / temporal_filter for one case"""
    f = frame(W, H)
    kw, (cur_planes, prev_planes) = COMBOS[combo]
    tp = R.Temporal(max_history=max_history, alpha=alpha, **kw)
    cam, prev_cam = cameras(R, W, H, camera)
    prev = {"out": f[f"prev_img{C}"], "n": f["prev_n"], "m2": f[f"prev_m2{C}"] if moments else None,
            "depth": f["prev_depth"], "normal": f["prev_normal"] if "normal" in prev_planes else None,
            "object": f["prev_object"] if "object" in prev_planes else None}
    kwargs = dict(normal=f["normal"] if "normal" in cur_planes else None,
                  object=f["object"] if "object" in cur_planes else None, prev=prev, moments=moments)
    return (f[f"img{C}"], tp, cam, prev_cam, f["depth"]), kwargs


@functools.lru_cache(maxsize=None)
def expected(W, H, C, combo, moments, alpha, max_history, camera):
    """temporal_filter of the case (with its history), computed once per process and never written to"""
    import rray_amd as R

    args, kwargs = arguments(R, W, H, C, combo, moments, alpha, max_history, camera)
    out = R.temporal_filter(*args, return_history=True, **kwargs)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def same_bits(a, b):
    """bit-for-bit equality of two f64 arrays; a NaN equals a NaN (its sign and payload are the processor's choice)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def same_result(got, want):
    """out, n and m2 of two results, bit for bit"""
    if not (same_bits(got["out"], want["out"]) and np.array_equal(got["out"], want["out"], equal_nan=True)):
        return False
    if got["n"].dtype != np.int32 or not np.array_equal(got["n"], want["n"]):
        return False
    if (got["m2"] is None) != (want["m2"] is None):
        return False
    return got["m2"] is None or same_bits(got["m2"], want["m2"])


# ---- the oracle's first-hit planes (the geometry tests) ----
def oracle_scene(oracle):
    """tests/test_gpu_indirect.py's oracle scene: a floor, a cube and a sphere resting on it"""
    floor = (0.1, 0.9, 0.0, 50.0, 0.0, 0.0, 1.0)
    body = (0.1, 0.9, 0.3, 50.0, 0.0, 0.0, 1.0)
    cub = [0.8, 0, 0, -1.5, 0, 0.8, 0, 0.8, 0, 0, 0.8, 0.0, 0, 0, 0, 1]
    sph = [0.8, 0, 0, 1.5, 0, 0.8, 0, 0.8, 0, 0, 0.8, 0.0, 0, 0, 0, 1]
    o = oracle.Oracle()
    o.point_light((-2.0, 6.0, -5.0), (1, 1, 1))
    o.add("plane", material=floor, pattern=o.pattern("solid", color=(1, 1, 1)))
    o.add("cube", transform=cub, material=body, pattern=o.pattern("solid", color=(1, 0, 0)))
    o.add("sphere", transform=sph, material=body, pattern=o.pattern("solid", color=(1, 1, 1)))
    return o


def oracle_planes(oracle, o, cam):
    """dict(depth, normal, object, point, origin) of `cam`'s pixels: hit() + prepare_computations of every
    ray_for_pixel, in rr_render_aov's layouts (depth = t, +inf and id -1 for a miss); point is the world hit point"""
    W, H = cam.hsize, cam.vsize
    ocam = oracle.Oracle.camera(W, H, cam.field_of_view, list(cam.transform))
    depth = np.full((H, W), np.inf)
    normal, point, over = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    obj = np.full((H, W), -1, np.int32)
    origin = None
    for y in range(H):
        for x in range(W):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            origin = ro[:3]
            xs = o.intersect(ro[:3], rd[:3])
            hit = next((k for k, s in enumerate(xs) if s[0] >= 0.0), None)
            if hit is None:
                continue
            c = o.prepare_computations(ro[:3], rd[:3], xs, hit)
            depth[y, x], obj[y, x] = c["t"], xs[hit][1]
            normal[y, x], point[y, x], over[y, x] = c["normalv"][:3], c["point"][:3], c["over_point"][:3]
    return dict(depth=depth, normal=normal, object=obj, point=point, over_point=over, origin=np.array(origin, np.float64))
