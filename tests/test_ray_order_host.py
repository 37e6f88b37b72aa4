"""CPU-side tests of the ordered ray batches (rr_ray_order_device, rr_color_at_device_ordered,
rr_hit_at_device_ordered; additive to ABI 11): declarations, exports, the header's RR_HAS_RAY_ORDER,
the Python mirror, the refusals that need no device, and the numpy mirror of the sort key (rray_amd.ray_order_keys)
against keys derived by hand from its definition: key = morton3(qx, qy, qz) << 14 | morton2(qu, qv), x and u bits
lowest, q = clamp(floor((c - lo) / (hi - lo) * 2^b), 0, 2^b - 1) with b = 6 for the origin and 7 for the octahedral
direction, 0 where hi == lo, 0xFFFFFFFF for a ray that is not valid.  The kernels are held to the mirror on the GPU
(tests/test_gpu_ray_order.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {"rr_ray_order_device": (5, r"rr_ctx\* ctx, int64_t n, const void\* d_rays, void\* d_perm, void\* hip_stream\)"),
         "rr_color_at_device_ordered": (9, r"rr_ctx\* ctx, int64_t n, const void\* d_rays, const void\* d_perm, int32_t remaining,"),
         "rr_hit_at_device_ordered": (6, r"rr_ctx\* ctx, int64_t n, const void\* d_rays, const void\* d_perm, void\* d_hits,")}
RR_E_ARG = -1
INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


def test_symbols_are_declared_exported_and_bound(R):
    L = R.lib()
    hdr = open(os.path.join(ROOT, "include", "rray", "rray.h")).read()
    assert re.search(r"^#define RR_HAS_RAY_ORDER 1\b", hdr, re.M)
    assert re.search(r"^#define RR_ABI_VERSION 11\b", hdr, re.M)
    assert L.rr_abi_version() == 11  # additive: the version does not move
    for n, (argc, params) in NAMES.items():
        assert hasattr(L, n), n
        assert n in R._lib.EXPORTS, n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == argc, n
        assert re.search(rf"^int {n}\({params}", hdr, re.M), n
    assert "NOT CHECKED" in hdr  # the header says that a caller's order is taken as it is
    for n in ("ray_order_device", "color_at_device_ordered", "hit_at_device_ordered"):
        assert callable(getattr(R.Renderer, n)), n
    assert callable(R.ray_order_keys) and "ray_order_keys" in R.__all__
    for f in ("render.py", "_lib.py"):  # the mirror does not import torch: pointers are integers
        assert not re.search(r"^\s*(import|from) torch\b", open(os.path.join(ROOT, "rray_amd", f)).read(), re.M), f


def test_a_null_context_is_refused_without_a_device(R):
    L = R.lib()
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    for n in (1, 0, -1):  # a null context is refused whatever n is
        assert L.rr_ray_order_device(None, n, p, p, None) == RR_E_ARG
        assert "null context" in L.rr_last_error().decode()
        assert L.rr_color_at_device_ordered(None, n, p, p, 5, 0, 0, p, None) == RR_E_ARG
        assert L.rr_color_at_device_ordered(None, n, p, None, 5, 0, 0, p, None) == RR_E_ARG
        assert L.rr_hit_at_device_ordered(None, n, p, p, p, None) == RR_E_ARG
        assert L.rr_hit_at_device_ordered(None, n, p, None, p, None) == RR_E_ARG
    assert L.rr_color_at_device_ordered(None, 1, p, p, -1, 0, 0, p, None) == RR_E_ARG  # before `remaining` is looked at


def test_documents_name_the_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in NAMES:
        assert re.search(rf"\bfn {n}\s*\(", integ), n
        assert n in readme, n
        assert n in design, n
    assert re.search(r"^### 3\.19 ", design, re.M)


# ---- the key, by hand ----
def rays_of(origins, directions):
    return np.concatenate([np.asarray(origins, np.float64), np.asarray(directions, np.float64)], axis=1)


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
# (u, v) of +-x, +-y, +-z: (1, 0), (-1, 0), (0, 1), (0, -1), (0, 0) and, folded over for dz < 0, (1, 1); the bounds are
# [-1, 1] on both axes, so q = clamp(floor((c + 1) / 2 * 128), 0, 127): -1 -> 0, 0 -> 64, 1 -> 127.
# morton2(qu, qv) interleaves with u lowest: 64 = bit 6 -> bit 12 (u) or 13 (v); 127 = seven ones -> 0x1555 (u) or 0x2AAA (v)
AXIS_KEYS = [0x1555 | 0x2000,  # +x: (127, 64)
             0x0000 | 0x2000,  # -x: (0, 64)
             0x1000 | 0x2AAA,  # +y: (64, 127)
             0x1000 | 0x0000,  # -y: (64, 0)
             0x1000 | 0x2000,  # +z: (64, 64)
             0x1555 | 0x2AAA]  # -z: (127, 127)


def test_directions_along_the_axes_with_one_origin(R):
    """identical origins: hi == lo on every origin axis, so the origin bits are 0 and the key is the direction's"""
    keys = R.ray_order_keys(rays_of([(0.5, -2.0, 7.0)] * 6, AXES))
    assert keys.dtype == np.uint32 and keys.shape == (6,)
    assert [int(k) for k in keys] == AXIS_KEYS
    # the direction need not be normalised: any positive multiple has the same (u, v) here (powers of two: exact)
    scaled = np.array(AXES, np.float64) * np.array([[4.0], [0.5], [8.0], [2.0], [0.25], [16.0]])
    assert [int(k) for k in R.ray_order_keys(rays_of([(0.5, -2.0, 7.0)] * 6, scaled))] == AXIS_KEYS


def test_origins_at_the_corners_of_their_box(R):
    """one direction: the direction bits are 0.  q = 0 at lo and 63 at hi; morton3 puts x at bits 0, 3, ..., y at 1, 4,
    ..., z at 2, 5, ...: 63 on one axis is 0x9249 shifted by the axis, on all three 0x3FFFF; the key is that << 14"""
    o = [(0, 0, 0), (1, 2, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3), (0.5, 1.0, 1.5)]
    keys = R.ray_order_keys(rays_of(o, [(0, 0, 1)] * 6))
    # the centre: floor(0.5 * 64) = 32 = bit 5 -> bits 15, 16, 17 of morton3
    want = [0, 0x3FFFF << 14, 0x9249 << 14, (0x9249 << 1) << 14, (0x9249 << 2) << 14, (0b111 << 15) << 14]
    assert [int(k) for k in keys] == want
    assert want[1] == 0xFFFFC000


def test_origin_bits_lie_above_direction_bits(R):
    o = [(0, 0, 0)] * 6 + [(1, 2, 3)] * 6
    keys = R.ray_order_keys(rays_of(o, AXES + AXES))
    assert [int(k) for k in keys] == AXIS_KEYS + [0xFFFFC000 | k for k in AXIS_KEYS]
    # the last one is a valid ray with every bit set: it shares the invalid rays' key, and a stable sort keeps it first
    assert int(keys[11]) == INVALID


def test_invalid_rays_get_the_last_key_and_change_no_other(R):
    o = [(0, 0, 0)] * 6 + [(1, 2, 3)] * 6
    base = rays_of(o, AXES + AXES)
    want = AXIS_KEYS + [0xFFFFC000 | k for k in AXIS_KEYS]
    bad = np.array([[np.nan, 0, 0, 0, 0, 1],      # a NaN component
                    [0, 0, 0, 0, np.nan, 1],
                    [0, np.inf, 0, 0, 0, 1],      # an infinite component (it must not stretch the bounds)
                    [0, 0, 0, -np.inf, 0, 1],
                    [1e300, -1e300, 0, 0, 0, 0],  # a zero direction (0 / 0), whatever its origin
                    [0, 0, 0, -0.0, 0.0, -0.0]])
    mixed = np.concatenate([bad[:3], base[:7], bad[3:], base[7:]])
    keys = [int(k) for k in R.ray_order_keys(mixed)]
    assert keys[:3] == [INVALID] * 3 and keys[10:13] == [INVALID] * 3
    assert keys[3:10] + keys[13:] == want
    assert [int(k) for k in R.ray_order_keys(bad)] == [INVALID] * 6  # a batch with no valid ray
    assert R.ray_order_keys(np.zeros((0, 6))).shape == (0,)


def test_the_order_of_a_shuffled_camera_is_coherent(R):
    """the issue's own measurement: a 64 x 64 pinhole camera under a random permutation, sorted by the key — the mean
    pixel bounding box of a 64-ray wave is far below the shuffled order's (3968 pixels there, 188 sorted)"""
    ys, xs = np.mgrid[0:64, 0:64]
    d = np.stack([(xs - 31.5) / 64.0, (31.5 - ys) / 64.0, np.ones((64, 64))], axis=2).reshape(-1, 3)
    rng = np.random.default_rng(7)
    shuffle = rng.permutation(4096)
    rays = rays_of(np.tile([0.0, 1.0, -5.0], (4096, 1)), d)[shuffle]

    def mean_box(order):
        px, py = xs.reshape(-1)[shuffle][order].reshape(64, 64), ys.reshape(-1)[shuffle][order].reshape(64, 64)
        return float(np.mean((np.ptp(px, axis=1) + 1) * (np.ptp(py, axis=1) + 1)))

    perm = np.argsort(R.ray_order_keys(rays), kind="stable")
    assert sorted(perm) == list(range(4096))
    assert mean_box(perm) < 400 and mean_box(np.arange(4096)) > 3000
