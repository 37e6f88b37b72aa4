"""The lens frames' definition on the host (rray.h RR_HAS_LENS): rr_camera_inverse, the counter hash,
rray_amd.lens_rays (the ray generator's mirror in numpy and the GPU tests' reference) and rray_amd.lens_resolve against
the oracle and against hand-made values.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


@pytest.fixture(scope="module")
def oracle():
    import oracle

    return oracle


def view(oracle):
    return oracle.Oracle.mat.view_transform((1.0, 2.5, -6.0), (0.3, 0.7, 0.2), (0.1, 1.0, 0.05))


SHEAR = [1.0, 0.3, 0.0, 0.5, 0.2, 1.0, -0.4, -1.0, 0.0, 0.1, 1.0, 2.0, 0.0, 0.0, 0.0, 1.0]


def test_abi_symbols_and_struct(R):
    L, E = R.lib(), R._lib
    for name in ("rr_camera_inverse", "rr_lens_rays_device", "rr_render_lens", "rr_render_lens_device"):
        assert hasattr(L, name) and name in E.EXPORTS
    assert C.sizeof(E.LensDesc) == 32 and E.LensDesc.aperture.offset == 8 and E.LensDesc.seed.offset == 24
    hdr = open(E.HEADER).read()
    assert "#define RR_HAS_LENS 1" in hdr and "#define RR_ABI_VERSION 11" in hdr
    assert f"#define RR_MAX_LENS_SAMPLES {E.RR_MAX_LENS_SAMPLES}" in hdr
    d = R.Lens(samples=8, pixel_jitter=True, aperture=0.25, focal_distance=5.5, seed=2**64 - 1).desc()
    assert (d.samples, d.pixel_jitter, d.aperture, d.focal_distance, d.seed) == (8, 1, 0.25, 5.5, 2**64 - 1)
    d = R.Lens().desc()
    assert (d.samples, d.pixel_jitter, d.aperture, d.focal_distance, d.seed) == (1, 0, 0.0, 1.0, 0)


@pytest.mark.parametrize("kind", ["affine", "sheared"])
def test_camera_inverse_equals_the_oracles(R, oracle, kind):
    t = view(oracle) if kind == "affine" else SHEAR
    cam = R.camera(13, 11, math.pi / 3, t)
    got = R.render.camera_inverse(cam)
    want = np.array(oracle.Oracle.mat.inverse(list(cam.transform)))
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert not np.array_equal(got, np.array(t))
    L, E = R.lib(), R._lib
    assert L.rr_camera_inverse(None, got.ctypes.data_as(E._D)) == E.RR_E_ARG
    assert L.rr_camera_inverse(C.byref(cam), None) == E.RR_E_ARG


def test_hash_equals_the_oracles_jitter(R, oracle):
    for seed in (0, 12345, 2**64 - 1):
        for i in (0, 1, 77, 2**31 + 5, 2**32 - 1):
            got = R.render.lens_hash(seed, np.array([i], np.uint64), np.arange(18, dtype=np.uint32))
            want = [oracle.Oracle.jitter(seed, i, 0, 0, k >> 1, k & 1) for k in range(18)]
            assert got.tolist() == want, (seed, i)
            assert all(0.0 <= v < 1.0 for v in want)


def test_pinhole_equals_ray_for_pixel(R, oracle):
    cam = R.camera(13, 11, math.pi / 3, view(oracle))
    ocam = oracle.Oracle.camera(13, 11, cam.field_of_view, list(cam.transform))
    want = np.array([list(o[:3]) + list(d[:3]) for y in range(11) for x in range(13)
                     for o, d in [oracle.Oracle.ray_for_pixel(ocam, x, y)]])
    got = R.lens_rays(cam, R.Lens())
    assert got.shape == (143, 6) and got.dtype == np.float64
    assert np.array_equal(got, want)
    # the lens seed is not read without jitter and aperture, and a focal distance is ignored by a pinhole
    assert np.array_equal(R.lens_rays(cam, R.Lens(seed=99, focal_distance=7.0)), want)


@pytest.mark.parametrize("lens_kw", [dict(samples=1), dict(samples=3, pixel_jitter=True),
                                     dict(samples=5, pixel_jitter=True, aperture=0.3, focal_distance=4.0, seed=7)],
                         ids=["pinhole", "jitter", "thin"])
def test_a_window_is_a_slice_of_the_frame(R, oracle, lens_kw):
    cam = R.camera(13, 11, math.pi / 3, view(oracle))
    lens = R.Lens(**lens_kw)
    S = lens.samples
    whole = R.lens_rays(cam, lens)
    assert whole.shape == (143 * S, 6)
    for first, n in ((0, 143), (5, 1), (17, 63), (142, 1), (30, 0), (143, 0)):
        got = R.lens_rays(cam, lens, first, n)
        assert np.array_equal(got, whole[first * S:(first + n) * S]), (first, n)
    assert np.array_equal(R.lens_rays(cam, lens, 100), whole[100 * S:])
    for first, n in ((-1, 1), (0, 144), (143, 1), (0, -1)):
        with pytest.raises(ValueError):
            R.lens_rays(cam, lens, first, n)


def test_jittered_image_points_stay_inside_their_pixels(R):
    # the identity camera: X is the identity, so the pinhole's f is (wx, wy, -1) itself
    cam = R.camera(13, 11, math.pi / 3)
    S = 16
    rays = R.lens_rays(cam, R.Lens(samples=S, pixel_jitter=True, seed=3))
    assert np.array_equal(rays[:, :3], np.zeros((143 * S, 3)))
    wx = rays[:, 3] / -rays[:, 5]  # the direction is (wx, wy, -1) / mag: back to the image plane at z = -1
    wy = rays[:, 4] / -rays[:, 5]
    p = np.repeat(np.arange(143), S)
    px, py = p % 13, p // 13
    tol = 4 * 2.0**-52 * max(cam.half_width, cam.half_height)  # the normalisation and the division back
    lo_x, hi_x = cam.half_width - (px + 1) * cam.pixel_size, cam.half_width - px * cam.pixel_size
    lo_y, hi_y = cam.half_height - (py + 1) * cam.pixel_size, cam.half_height - py * cam.pixel_size
    assert np.all(wx >= lo_x - tol) and np.all(wx <= hi_x + tol)
    assert np.all(wy >= lo_y - tol) and np.all(wy <= hi_y + tol)
    # and they do move: the S samples of a pixel are S different points, spread over most of the pixel
    spread = (wx.reshape(143, S).max(axis=1) - wx.reshape(143, S).min(axis=1)) / cam.pixel_size
    assert np.all(spread > 0.3) and len(np.unique(wx)) == 143 * S
    # the offsets are the hash's: u(0), u(1) of ray i
    i = np.arange(143 * S, dtype=np.uint64)
    jx = R.render.lens_hash(3, i, 0)
    assert np.allclose((cam.half_width - wx) / cam.pixel_size - px, jx, rtol=0, atol=1e-9)


def test_thin_lens_rays(R, oracle):
    cam = R.camera(13, 11, math.pi / 3, view(oracle))
    S, ap, fd = 8, 0.25, 5.5
    rays = R.lens_rays(cam, R.Lens(samples=S, aperture=ap, focal_distance=fd, seed=11))
    o, d = rays[:, :3], rays[:, 3:]
    # unit directions to 1 ulp
    assert np.all(np.abs(np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2) - 1.0) <= 2.0**-52)
    # origins on the lens: within `aperture` of the pinhole's origin.  The aperture is a camera-space radius, and
    # view_transform's `left` is not normalised (transformation.rs: cross(forward, normalize(up)) with an `up` that is
    # not perpendicular to the view), so this camera's inverse stretches x: the distance is taken in camera space,
    # where the pinhole's origin is (0, 0, 0) and the lens the disc of radius `aperture` in z = 0
    pin = R.lens_rays(cam, R.Lens())
    T = np.array(list(cam.transform)).reshape(4, 4)
    oc = np.concatenate([o, np.ones((len(o), 1))], axis=1) @ T.T
    assert np.abs(np.concatenate([pin[:1, :3], [[1.0]]], axis=1) @ T.T - [0, 0, 0, 1]).max() <= 1e-14
    assert np.all(np.hypot(oc[:, 0], oc[:, 1]) <= ap * (1 + 1e-12)) and np.abs(oc[:, 2]).max() <= 1e-14
    assert len(np.unique(o, axis=0)) > 143 * S // 2  # and they do spread over it
    # and with a camera whose axes are orthonormal (up perpendicular to the view) the same holds in world space
    rigid = R.camera(13, 11, math.pi / 3, oracle.Oracle.mat.view_transform((1.0, 2.5, -6.0), (1.0, 2.5, 0.0), (0.0, 1.0, 0.0)))
    rr = R.lens_rays(rigid, R.Lens(samples=S, aperture=ap, focal_distance=fd, seed=11))
    assert np.all(np.linalg.norm(rr[:, :3] - R.lens_rays(rigid, R.Lens())[0, :3], axis=1) <= ap * (1 + 1e-12))
    # the S rays of a pixel meet in its point of the plane in focus: f = origin + fd * (pinhole f - origin)
    M = R.render.camera_inverse(cam).reshape(4, 4)
    p = np.repeat(np.arange(143), S)
    wx = cam.half_width - ((p % 13) + 0.5) * cam.pixel_size
    wy = cam.half_height - ((p // 13) + 0.5) * cam.pixel_size
    f = np.stack([wx * fd, wy * fd, np.full(len(p), -fd), np.ones(len(p))], axis=1) @ M.T
    f = f[:, :3]
    t = np.einsum("ij,ij->i", f - o, d)  # the ray's parameter nearest to f
    miss = np.abs(o + t[:, None] * d - f)
    bound = 64 * 2.0**-52 * max(np.abs(f).max(), np.abs(o).max())
    print(f"thin lens: the rays miss their focus point by at most {miss.max() / (bound / 64):.2f} ulps of the largest "
          f"coordinate (bound 64)")
    assert miss.max() <= bound
    # with an identity camera the focus point is (wx fd, wy fd, -fd) itself and the lens lies in z = 0
    cam0 = R.camera(13, 11, math.pi / 3)
    r0 = R.lens_rays(cam0, R.Lens(samples=S, aperture=ap, focal_distance=fd, seed=11))
    assert np.array_equal(r0[:, 2], np.zeros(143 * S)) and np.all(r0[:, 0] ** 2 + r0[:, 1] ** 2 <= ap * ap)
    # the first accepted pair of the rejection loop, from the hash
    i = np.arange(143 * S, dtype=np.uint64)
    A, B = 2.0 * R.render.lens_hash(11, i, 2) - 1.0, 2.0 * R.render.lens_hash(11, i, 3) - 1.0
    first = A * A + B * B <= 1.0
    assert 0.7 < first.mean() < 0.86  # pi / 4
    assert np.array_equal(r0[first, 0], ap * A[first]) and np.array_equal(r0[first, 1], ap * B[first])


def test_pass_split(tmp_path):
    """rray_amd/csrc/frame_plan.hpp plan_lens_passes, compiled with g++ into tests/native/lens_pass_check.cpp.  The
    expectations are derived by hand from the definition: passes of whole pixels, a multiple of 64 each but the last;
    by default the largest such count with at most 2^22 rays and at least 64 pixels; an override rounded up to 64."""
    import os
    import shutil
    import subprocess

    here = os.path.dirname(os.path.abspath(__file__))
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "lens_pass_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment",
                    "-I" + os.path.join(os.path.dirname(here), "rray_amd", "csrc"),
                    os.path.join(here, "native", "lens_pass_check.cpp"), "-o", exe], check=True)
    rows = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *fields = line.split()
        assert kind == "lens" and name not in rows
        rows[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}

    def check(name, **want):
        assert {k: rows[name][k] for k in want} == want, (name, rows[name])

    check("none", pixels=0, passes=0, count=0)
    check("no_samples", pixels=0, passes=0, count=0)
    check("t200_s3_pass64", pixels=64, passes=4, count=4, sum=200, largest=64, smallest=8, misaligned=0)
    check("t200_s3_pass1", pixels=64, passes=4, count=4, sum=200, smallest=8, misaligned=0)
    check("t200_s3_pass65", pixels=128, passes=2, count=2, sum=200, largest=128, smallest=72, misaligned=0)
    check("t200_s3_default", pixels=(2**22 // 3) // 64 * 64, passes=1, count=1, sum=200, largest=200)
    hd = 1920 * 1080
    check("hd_s8", pixels=2**19, passes=4, count=4, sum=hd, largest=2**19, smallest=hd - 3 * 2**19, misaligned=0,
          pass_rays=2**22)
    check("hd_s1", pixels=2**22, passes=1, count=1, sum=hd, pass_rays=hd)
    check("hd_s5", pixels=838848, passes=3, count=3, sum=hd, misaligned=0, pass_rays=838848 * 5)  # 838 860 rounded down
    assert 838848 % 64 == 0 and 838848 * 5 <= 2**22 < (838848 + 64) * 5
    check("hd_s4096", pixels=1024, passes=2025, count=2025, sum=hd, misaligned=0, pass_rays=2**22)
    check("hd_s3000", pixels=1344, passes=1543, sum=hd, misaligned=0, pass_rays=1344 * 3000)  # 1398 pixels' worth -> 1344
    assert 1344 * 3000 <= 2**22 < (1344 + 64) * 3000 and 1542 * 1344 < hd <= 1543 * 1344
    check("s100000", pixels=64, passes=16, sum=1000, smallest=40)  # 41 pixels' worth of rays: at least 64 pixels
    check("exactly_one_pass_s8", pixels=2**19, passes=1, count=1, sum=2**19)
    check("one_more_pixel_s8", pixels=2**19, passes=2, count=2, sum=2**19 + 1, smallest=1, misaligned=0)
    check("huge_override", pixels=2**40, passes=1, count=1, sum=1000)


def test_resolve_sums_in_sample_order(R):
    c = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125], [4.0, 4.0, 4.0], [1.0, 1.0, 1.0]])
    assert np.array_equal(R.lens_resolve(c, 1), c)
    assert np.array_equal(R.lens_resolve(c, 2), np.array([[0.75, 1.125, 1.5625], [2.5, 2.5, 2.5]]))
    assert np.array_equal(R.lens_resolve(c, 4), np.array([[6.5 / 4, 7.25 / 4, 8.125 / 4]]))
    # the order matters: (1e16 + 1) - 1e16 is 0, (1e16 - 1e16) + 1 is 1
    a = np.array([[1e16, 1e16, 0.1], [1.0, -1e16, 0.2], [-1e16, 1.0, 0.3]])
    got = R.lens_resolve(a, 3)
    assert got.tolist() == [[0.0 / 3.0, 1.0 / 3.0, ((0.1 + 0.2) + 0.3) / 3.0]]
    assert ((0.1 + 0.2) + 0.3) != (0.1 + (0.2 + 0.3))
    # thirds are divisions, not multiplications by a reciprocal
    b = np.array([[5.0, 7.0, 11.0]] * 3)
    assert got.shape == (1, 3) and R.lens_resolve(b, 3).tolist() == [[15.0 / 3.0, 21.0 / 3.0, 33.0 / 3.0]]
    # NaN and inf pass through
    n = R.lens_resolve(np.array([[math.nan, math.inf, 1.0], [1.0, -math.inf, 1.0]]), 2)
    assert math.isnan(n[0, 0]) and math.isnan(n[0, 1]) and n[0, 2] == 1.0
