"""Frames and parameter sets shared by the denoiser's host and GPU tests (test_denoise_host.py, test_gpu_denoise.py):
the same frame list, channel counts, level counts and term combinations on both sides, each built once per process."""
import functools

import numpy as np

# (W, H): one pixel; smaller than the kernel; one row and one column longer than a wave's run of 32; odd sizes; a frame
# of whole 32 x 8 tiles' width but half a tile's height; 70 x 37: more than one tile in both directions, partial last
# tiles in both
FRAMES = ((1, 1), (3, 2), (65, 1), (1, 65), (7, 5), (13, 5), (64, 4), (70, 37))
CHANNELS = (1, 3)
ITERATIONS = (1, 2, 6)  # 6: holes of 32 pixels, wider than most of the frames
# name -> (Denoise keywords, the planes that are passed).  Each term alone, all together with and without RR_DN_OBJECT,
# and none (the plain a-trous filter; depth and object only mark void pixels).
COMBOS = {
    "none": (dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0), ("depth", "object")),
    "object": (dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, object=True), ("object",)),
    "colour": (dict(sigma_color=0.5, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0), ()),
    "normal": (dict(sigma_color=0.0, sigma_normal=0.25, sigma_depth=0.0, sigma_albedo=0.0), ("normal", "depth")),
    "depth": (dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.05, sigma_albedo=0.0), ("depth",)),
    "albedo": (dict(sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.1), ("albedo", "object")),
    "all": (dict(sigma_color=0.5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1, object=True),
            ("depth", "normal", "object", "albedo")),
    "all_no_object": (dict(sigma_color=0.5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1),
                      ("depth", "normal", "object", "albedo")),
}


@functools.lru_cache(maxsize=None)
def frame(W, H):
    """A seeded frame of W x H: dict of img1 (H, W), img3 (H, W, 3), depth, normal, object, albedo.  Guides are smooth
    enough that every term passes some taps and cuts others, carry more bits than a float holds, and include the
    definition's edge cases wherever the frame has room: void rows and void islands (by depth alone, by object alone, by
    both), a depth of exactly 0.0, normals of (0, 0, 0), an object seam."""
    rng = np.random.default_rng(1000 * W + H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 5.0 + 0.11 * x + 0.23 * y + 0.01 * rng.random((H, W))
    normal = np.stack([0.3 * np.sin(0.4 * x) + 0.05 * rng.normal(size=(H, W)), 0.3 * np.cos(0.3 * y) +
                       0.05 * rng.normal(size=(H, W)), np.ones((H, W))], axis=2)
    normal /= np.sqrt((normal * normal).sum(axis=2, keepdims=True))
    obj = ((x >= W // 2).astype(np.int32) + 2 * (y >= (2 * H) // 3).astype(np.int32)).astype(np.int32)
    palette = np.array([[0.8, 0.2, 0.2], [0.78, 0.22, 0.25], [0.2, 0.7, 0.3], [0.21, 0.69, 0.33]])
    albedo = palette[obj] + 0.02 * rng.random((H, W, 3))
    img3 = 0.5 + 0.3 * np.sin(0.2 * x + 0.1 * y)[..., None] + 0.25 * rng.normal(size=(H, W, 3))
    img1 = np.clip(0.6 + 0.2 * np.cos(0.15 * x) + 0.3 * rng.normal(size=(H, W)), 0.0, 1.0)
    if W * H >= 6:
        depth[0, W - 1] = 0.0  # a depth of exactly 0
        normal[H - 1, 0] = 0.0  # a normal of (0, 0, 0)
    if W >= 7 and H >= 5:
        depth[1, 2:4] = np.inf  # an island, void by depth alone
        obj[3, 4:6] = -1  # void by object alone
        depth[2, 5], obj[2, 5] = np.inf, -1  # by both
        depth[H - 2, 1] = np.nan  # a NaN depth is void
    if H >= 30:
        depth[20:24, :] = np.inf  # four void rows
        obj[20:24, :] = -1
    if W >= 60 and H == 1:
        depth[0, 30:34], obj[0, 30:34] = np.inf, -1
    if H >= 60 and W == 1:
        depth[40:43, 0], obj[40:43, 0] = np.inf, -1
    out = dict(img1=img1, img3=img3, depth=depth, normal=normal, object=obj, albedo=albedo)
    for v in out.values():
        v.setflags(write=False)
    return out


def cases():
    """(W, H, C, iterations, combo name) of the whole product"""
    return [(W, H, C, I, name) for (W, H) in FRAMES for C in CHANNELS for I in ITERATIONS for name in COMBOS]


def arguments(R, W, H, C, iterations, name):
    """(image, Denoise, planes dict) of one case"""
    f = frame(W, H)
    kw, given = COMBOS[name]
    return f["img1" if C == 1 else "img3"], R.Denoise(iterations, **kw), {k: f[k] for k in given}


@functools.lru_cache(maxsize=None)
def expected(W, H, C, iterations, name):
    """denoise_filter of the case, computed once per process and never written to"""
    import rray_amd as R

    img, dn, planes = arguments(R, W, H, C, iterations, name)
    out = R.denoise_filter(img, dn, **planes)
    out.setflags(write=False)
    return out


def same_bits(a, b):
    """bit-for-bit equality of two f64 arrays; a NaN equals a NaN (its sign and payload are the processor's choice)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
