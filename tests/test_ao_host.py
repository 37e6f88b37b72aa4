"""The ambient-occlusion definition on the host (rray.h RR_HAS_AO): the symbols, the refusals that need
no device, rr_ao_directions (the very function ao_pairs_kernel calls, rray_amd/csrc/ao_dir.hpp) against its numpy mirror
rray_amd.ao_directions bit for bit, the directions' geometry and distribution, the hash against the oracle's, and the
frames' pass split.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KS = (1, 3, 64, 65, 1024)
FIRSTS = (0, 2**32 - 70)
EPS = 2.0**-52


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def normals():
    """the six axes, N.z = +0.0 and -0.0, N.z within 1e-9 of -1 (the basis's hard spot), 200 random unit vectors"""
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    zero = [[0.6, 0.8, 0.0], [0.6, 0.8, -0.0], [-1.0, 0.0, 0.0], [-1.0, 0.0, -0.0]]
    near = []
    for e in (1e-9, 1e-12, 1e-16, 3e-10):
        z = -1.0 + e
        r = math.sqrt(max(0.0, 1.0 - z * z))
        near += [[r * 0.6, r * 0.8, z], [-r, 0.0, z], [0.0, r, z]]
    rng = np.random.default_rng(20261021)
    rnd = unit(rng.normal(size=(200, 3)))
    out = np.concatenate([np.array(axes, np.float64), np.array(zero, np.float64), np.array(near, np.float64), rnd])
    assert np.signbit(out[7, 2]) and not np.signbit(out[6, 2])
    return out


def native_directions(R, ao, first, N):
    L, E = R.lib(), R._lib
    N = np.ascontiguousarray(N, np.float64)
    out = np.full((len(N), ao.samples, 3), -12345.5)
    d = ao.desc()
    assert L.rr_ao_directions(C.byref(d), first, len(N), N.ctypes.data_as(E._D), out.ctypes.data_as(E._D)) == 0
    return out


def test_abi_symbols_and_struct(R):
    L, E = R.lib(), R._lib
    for name in ("rr_ao_directions", "rr_ao_at_device", "rr_render_ao", "rr_render_ao_device"):
        assert hasattr(L, name) and name in E.EXPORTS, name
    hdr = open(E.HEADER).read()
    for name in ("rr_ao_directions", "rr_ao_at_device", "rr_render_ao", "rr_render_ao_device"):
        assert f"int {name}(" in hdr, name
    assert "#define RR_HAS_AO 1" in hdr and "#define RR_ABI_VERSION 11" in hdr
    assert f"#define RR_MAX_AO_SAMPLES {E.RR_MAX_AO_SAMPLES}" in hdr and E.RR_MAX_AO_SAMPLES == 1024
    assert C.sizeof(E.AoDesc) == 24 and E.AoDesc.radius.offset == 8 and E.AoDesc.seed.offset == 16
    d = R.Ao(16, 0.5, seed=2**64 - 1).desc()
    assert (d.samples, d.reserved, d.radius, d.seed) == (16, 0, 0.5, 2**64 - 1)
    assert R.Ao(3, 2).desc().seed == 0
    for name in ("ao_at_device", "render_ao", "render_ao_device"):
        assert callable(getattr(R.Renderer, name))
    for name in ("Ao", "ao_directions", "ao_targets", "ao_resolve"):
        assert name in R.__all__ and hasattr(R, name)


def test_sizeof_rr_ao_is_24_for_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not available")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rray/rray.h"\n'
                   '_Static_assert(sizeof(rr_ao) == 24, "rr_ao");\n'
                   '_Static_assert(offsetof(rr_ao, radius) == 8 && offsetof(rr_ao, seed) == 16, "rr_ao layout");\n'
                   '#if !defined(RR_HAS_AO) || RR_MAX_AO_SAMPLES != 1024 || RR_ABI_VERSION != 11\n#error\n#endif\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-comment", "-I" + os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_refusals_that_need_no_device(R):
    L, E = R.lib(), R._lib
    ARG = E.RR_E_ARG
    N = np.array([[0.0, 0.0, 1.0]])
    out = np.full((1, 4, 3), -12345.5)
    pn, po = N.ctypes.data_as(E._D), out.ctypes.data_as(E._D)
    cam = R.camera(8, 8, 1.0)
    o = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    host = np.full((8, 8), -12345.5)
    ph = host.ctypes.data_as(E._D)
    fake = C.c_void_p(4096)  # never dereferenced: the parameters are refused first

    def ao(**kw):
        f = dict(samples=4, reserved=0, radius=1.0, seed=0)
        f.update(kw)
        return C.byref(E.AoDesc(*f.values()))

    def err():
        return L.rr_last_error().decode()

    bad = (dict(samples=0), dict(samples=-1), dict(samples=1025), dict(reserved=1), dict(reserved=-1), dict(radius=0.0),
           dict(radius=-1.0), dict(radius=math.nan), dict(radius=math.inf), dict(radius=-math.inf))
    for kw in bad:
        assert L.rr_ao_directions(ao(**kw), 0, 1, pn, po) == ARG, kw
        assert L.rr_ao_at_device(None, 1, fake, fake, ao(**kw), fake, None) == ARG, kw
        assert L.rr_render_ao(None, C.byref(cam), C.byref(o), ao(**kw), ph, None) == ARG, kw
        assert L.rr_render_ao_device(None, C.byref(cam), C.byref(o), ao(**kw), fake, None) == ARG, kw
    assert L.rr_ao_directions(ao(samples=0), 0, 1, pn, po) == ARG and "samples" in err()
    assert L.rr_ao_directions(ao(reserved=2), 0, 1, pn, po) == ARG and "reserved" in err()
    assert L.rr_ao_directions(ao(radius=0.0), 0, 1, pn, po) == ARG and "radius" in err()
    # null pointers, negative counts
    assert L.rr_ao_directions(None, 0, 1, pn, po) == ARG
    assert L.rr_ao_directions(ao(), 0, 1, None, po) == ARG
    assert L.rr_ao_directions(ao(), 0, 1, pn, None) == ARG
    assert L.rr_ao_directions(ao(), -1, 1, pn, po) == ARG
    assert L.rr_ao_directions(ao(), 0, -1, pn, po) == ARG
    assert L.rr_ao_at_device(None, 1, fake, fake, ao(), fake, None) == ARG  # null context
    assert L.rr_ao_at_device(None, 1, fake, fake, None, fake, None) == ARG
    assert L.rr_render_ao(None, C.byref(cam), C.byref(o), ao(), ph, None) == ARG
    assert L.rr_render_ao(None, None, C.byref(o), ao(), ph, None) == ARG
    assert L.rr_render_ao(None, C.byref(cam), None, ao(), ph, None) == ARG
    assert L.rr_render_ao(None, C.byref(cam), C.byref(o), None, ph, None) == ARG
    assert L.rr_render_ao(None, C.byref(cam), C.byref(o), ao(), None, None) == ARG
    assert L.rr_render_ao_device(None, C.byref(cam), C.byref(o), ao(), fake, None) == ARG
    assert L.rr_render_ao_device(None, C.byref(cam), C.byref(o), ao(), None, None) == ARG
    assert (out == -12345.5).all() and (host == -12345.5).all()
    # n == 0 is RR_OK and touches nothing; the boundary values serve
    assert L.rr_ao_directions(ao(), 5, 0, None, None) == 0
    assert L.rr_ao_directions(ao(samples=4, radius=5e-324), 0, 1, pn, po) == 0
    assert np.isfinite(out).all()


@pytest.mark.parametrize("K", KS)
def test_directions_equal_the_numpy_mirror(R, K):
    N = normals()
    for first in FIRSTS:
        for seed in (0, 2**63 + 11):
            ao = R.Ao(K, 1.0, seed)
            got = native_directions(R, ao, first, N)
            want = R.ao_directions(N, ao, first)
            assert got.shape == want.shape == (len(N), K, 3) and want.dtype == np.float64
            assert np.array_equal(got, want), (K, first, seed)
    # the radius plays no part in a direction, the seed and the index do
    a = R.ao_directions(N, R.Ao(K, 1.0, 5), 0)
    assert np.array_equal(a, R.ao_directions(N, R.Ao(K, 7.5, 5), 0))
    assert not np.array_equal(a, R.ao_directions(N, R.Ao(K, 1.0, 6), 0))
    assert not np.array_equal(a, R.ao_directions(N, R.Ao(K, 1.0, 5), 1))
    # a window is a slice: point i's directions depend on first + i alone
    assert np.array_equal(R.ao_directions(N[3:9], R.Ao(K, 1.0, 5), 3), a[3:9])
    assert np.array_equal(native_directions(R, R.Ao(K, 1.0, 5), 3, N[3:9]), a[3:9])


def basis(N):
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    s = np.copysign(1.0, nz)
    q = -1.0 / (s + nz)
    b = (nx * ny) * q
    T = np.stack([1.0 + (s * (nx * nx)) * q, s * b, -(s * nx)], axis=1)
    B = np.stack([b, s + (ny * ny) * q, -ny], axis=1)
    return T, B


@pytest.mark.parametrize("K", KS)
def test_directions_are_unit_and_never_below_the_surface(R, K):
    N = normals()
    T, B = basis(N)
    assert np.isfinite(T).all() and np.isfinite(B).all()
    # unit inputs to 1 ulp, so the frame is orthonormal to 1e-15
    assert np.abs((N * N).sum(axis=1) - 1.0).max() <= 4 * EPS
    for a, b, want in ((T, T, 1.0), (B, B, 1.0), (T, B, 0.0), (T, N, 0.0), (B, N, 0.0)):
        assert np.abs((a * b).sum(axis=1) - want).max() <= 1e-15
    for first in FIRSTS:
        w = native_directions(R, R.Ao(K, 1.0, 3), first, N)
        assert np.isfinite(w).all()
        mag = np.sqrt((w[..., 0] ** 2 + w[..., 1] ** 2) + w[..., 2] ** 2)
        assert np.abs(mag - 1.0).max() <= 4 * EPS, (K, first, float(np.abs(mag - 1.0).max() / EPS))
        assert ((w * N[:, None, :]).sum(axis=2) >= 0.0).all(), (K, first)


def test_directions_are_cosine_weighted(R):
    """Malley's method: the density is cos(theta) / pi, so E[w . N] = 2/3 and Var[w . N] = 1/2 - 4/9 = 1/18; over n
    directions the mean lies within 4 standard errors of 2/3 (a fixed seed: the draw is always the same)."""
    N = unit(np.random.default_rng(7).normal(size=(200, 3)))
    w = native_directions(R, R.Ao(1000, 1.0, 99), 0, N)
    c = (w * N[:, None, :]).sum(axis=2).reshape(-1)
    n = len(c)
    assert n == 200000
    se = math.sqrt((1.0 / 18.0) / n)
    print(f"mean of w.N over {n} directions: {c.mean():.6f} (2/3 = {2 / 3:.6f}, standard error {se:.2e}, "
          f"{abs(c.mean() - 2 / 3) / se:.2f} of them off); smallest {c.min():.3g}")
    assert abs(c.mean() - 2.0 / 3.0) <= 4.0 * se
    # and uniform in azimuth: the tangent-plane components average to zero (variance 1/4 each)
    T, B = basis(N)
    for axis in (T, B):
        t = (w * axis[:, None, :]).sum(axis=2).reshape(-1)
        assert abs(t.mean()) <= 4.0 * math.sqrt(0.25 / n)


def test_hash_equals_the_oracles_jitter(R):
    import oracle

    for seed in (0, 12345, 2**64 - 1):
        for i in (0, 77, 2**32 - 70, 2**32 - 1):
            for k in (0, 1, 63, 1023):
                got = R.render.lens_hash(seed, np.array([i], np.uint64), (np.uint32(k) << np.uint32(21)) | np.arange(16, dtype=np.uint32))
                want = [oracle.Oracle.jitter(seed, i, 0, k, j >> 1, j & 1) for j in range(16)]
                assert got.tolist() == want, (seed, i, k)
    # the first accepted disc point of point 5, k = 2, from the hash itself
    ao = R.Ao(4, 1.0, 9)
    w = R.ao_directions(np.array([[0.0, 0.0, 1.0]]), ao, 5)[0, 2]
    for a in range(8):
        A = 2.0 * oracle.Oracle.jitter(9, 5, 0, 2, a, 0) - 1.0
        B = 2.0 * oracle.Oracle.jitter(9, 5, 0, 2, a, 1) - 1.0
        if A * A + B * B <= 1.0:
            break
    # N = +z: s = 1, q = -1/2, b = 0, T = (1, 0, -0) and Bv = (0, 1, -0): w = (A, B, c)
    assert w.tolist() == [A * 1.0 + B * 0.0 + math.sqrt(1.0 - (A * A + B * B)) * 0.0,
                          A * 0.0 + B * 1.0 + math.sqrt(1.0 - (A * A + B * B)) * 0.0,
                          (A * -0.0 + B * -0.0) + math.sqrt(1.0 - (A * A + B * B)) * 1.0]


def test_targets_and_resolve(R):
    ao = R.Ao(3, 0.25, 1)
    P = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.0]])
    N = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])
    w = R.ao_directions(N, ao, 10)
    t = R.ao_targets(P, N, ao, 10)
    assert t.shape == (2, 3, 3) and np.array_equal(t, P[:, None, :] + 0.25 * w)
    assert np.abs(np.linalg.norm(t - P[:, None, :], axis=2) - 0.25).max() <= 4 * EPS
    assert R.ao_resolve([0, 0, 0, 1, 1, 1, 1, 0, 0], 3).tolist() == [1.0, 0.0, 2.0 / 3.0]
    assert R.ao_resolve(np.array([[True, False], [False, False]]), 2).tolist() == [0.5, 1.0]
    assert R.ao_resolve(np.zeros(7, np.int32), 7).tolist() == [1.0]
    # thirds are divisions, not multiplications by a reciprocal
    assert R.ao_resolve([1, 0, 0], 3)[0] == 2.0 / 3.0 and R.ao_resolve([1] * 5 + [0] * 44, 49)[0] == 44.0 / 49.0


def test_pass_split(tmp_path):
    """rray_amd/csrc/frame_plan.hpp plan_ao_passes, compiled with g++ into tests/native/ao_pass_check.cpp.  The
    expectations are derived by hand from the definition: passes of whole points, a multiple of 64 each but the last; by
    default the largest such count with at most 2^22 pairs and at least 64 points; an override rounded up to 64; either
    capped by the batch rounded down to 64 (at least 64) and kept below 2^32 pairs."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "ao_pass_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-comment",
                    "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "rray_amd", "csrc"),
                    os.path.join(HERE, "native", "ao_pass_check.cpp"), "-o", exe], check=True)
    rows, dirs = {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *fields = line.split()
        into = {"ao": rows, "dir": dirs}[kind]
        assert name not in into
        into[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}

    def check(name, **want):
        assert {k: rows[name][k] for k in want} == want, (name, rows[name])

    for name in ("none", "no_samples", "no_batch"):
        check(name, points=0, passes=0, count=0)
    check("t65_k3_pass64", points=64, passes=2, count=2, sum=65, largest=64, smallest=1, misaligned=0)
    check("t65_k3_pass1", points=64, passes=2, count=2, sum=65, smallest=1, misaligned=0)
    check("t384_k16_pass65", points=128, passes=3, count=3, sum=384, largest=128, smallest=128, misaligned=0)
    check("t384_k16_default", points=2**18, passes=1, count=1, sum=384, largest=384)
    hd = 1920 * 1080
    check("hd_k16", points=2**18, passes=8, count=8, sum=hd, largest=2**18, smallest=hd - 7 * 2**18, misaligned=0,
          pass_pairs=2**22)
    check("hd_k1", points=2**22, passes=1, count=1, sum=hd, pass_pairs=hd)
    check("hd_k5", points=838848, passes=3, count=3, sum=hd, misaligned=0, pass_pairs=838848 * 5)  # 838 860 rounded down
    assert 838848 % 64 == 0 and 838848 * 5 <= 2**22 < (838848 + 64) * 5
    check("hd_k1024", points=4096, passes=507, count=507, sum=hd, misaligned=0, pass_pairs=2**22)
    assert 506 * 4096 < hd <= 507 * 4096
    check("k100000", points=64, passes=16, sum=1000, smallest=40)  # 41 points' worth of pairs: at least 64 points
    check("hd_k16_batch1024", points=1024, passes=2025, count=2025, sum=hd, largest=1024, smallest=1024, misaligned=0)
    assert 2025 * 1024 == hd
    check("t3000_k1_batch1100", points=1088, passes=3, count=3, sum=3000, largest=1088, smallest=3000 - 2 * 1088, misaligned=0)
    check("t3000_k1_batch1100_pass4096", points=1088, passes=3, count=3, sum=3000)
    check("t100_k1_batch10", points=64, passes=2, count=2, sum=100, smallest=36)
    check("huge_override_k1024", points=4194240, passes=3, count=3, sum=10**7, misaligned=0, pass_pairs=4194240 * 1024)
    assert 4194240 % 64 == 0 and 4194240 * 1024 < 2**32 <= (4194240 + 64) * 1024
    check("huge_override_k1", points=2**32 - 64, passes=1, count=1, sum=1000)
    # ao_dir.hpp on the host compiler: finite, above the surface and unit at the basis's edge normals
    assert set(dirs) == {"x", "-x", "y", "-y", "z", "-z", "z+0", "z-0", "near-z"}
    for name, d in dirs.items():
        assert d == dict(finite=1, above=1, unit=1), (name, d)
