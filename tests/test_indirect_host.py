"""One-bounce indirect light on the host (rray.h RR_HAS_INDIRECT): the symbols, the refusals that need
no device, the numpy definitions (indirect_rays against ao_directions composed by hand, indirect_resolve,
indirect_compose, object_diffuse) and the pass split.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("rr_indirect_at_device", "rr_render_indirect", "rr_render_indirect_device")
SENT = -12345.5


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def test_abi_symbols_and_struct(R):
    L, E = R.lib(), R._lib
    hdr = open(E.HEADER).read()
    for name in NAMES:
        assert hasattr(L, name) and name in E.EXPORTS, name
        assert f"int {name}(" in hdr, name
    assert "#define RR_HAS_INDIRECT 1" in hdr and "#define RR_ABI_VERSION 11" in hdr
    assert f"#define RR_MAX_INDIRECT_SAMPLES {E.RR_MAX_INDIRECT_SAMPLES}" in hdr and E.RR_MAX_INDIRECT_SAMPLES == 1024
    assert C.sizeof(E.IndirectDesc) == 16 and E.IndirectDesc.remaining.offset == 4 and E.IndirectDesc.seed.offset == 8
    d = R.Indirect(16, 3, seed=2**64 - 1).desc()
    assert (d.samples, d.remaining, d.seed) == (16, 3, 2**64 - 1)
    d = R.Indirect(4).desc()
    assert (d.samples, d.remaining, d.seed) == (4, 1, 0)
    for name in ("indirect_at_device", "render_indirect", "render_indirect_device"):
        assert callable(getattr(R.Renderer, name))
    for name in ("Indirect", "indirect_rays", "indirect_resolve", "indirect_compose", "object_diffuse"):
        assert name in R.__all__ and hasattr(R, name)
    # the caveat of the plain ray entries is stated for this feature too
    block = hdr[hdr.index("test RR_HAS_INDIRECT"):hdr.index("#define RR_HAS_INDIRECT 1")]
    assert "shininess" in block and "ulp" in block


def test_sizeof_rr_indirect_is_16_for_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not available")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rray/rray.h"\n'
                   '_Static_assert(sizeof(rr_indirect) == 16, "rr_indirect");\n'
                   '_Static_assert(offsetof(rr_indirect, remaining) == 4 && offsetof(rr_indirect, seed) == 8, "layout");\n'
                   '#if !defined(RR_HAS_INDIRECT) || RR_MAX_INDIRECT_SAMPLES != 1024 || RR_ABI_VERSION != 11\n#error\n#endif\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-comment", "-I" + os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_refusals_that_need_no_device(R):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    cam = R.camera(8, 8, 1.0)
    o = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    host = np.full((8, 8, 3), SENT)
    ph = host.ctypes.data_as(E._D)
    fake = C.c_void_p(4096)  # never dereferenced: the parameters are refused first
    pc, po = C.byref(cam), C.byref(o)

    def ind(**kw):
        f = dict(samples=4, remaining=1, seed=0)
        f.update(kw)
        return C.byref(E.IndirectDesc(*f.values()))

    def err():
        return L.rr_last_error().decode()

    def all_entries(d):
        return (L.rr_indirect_at_device(None, 1, fake, fake, d, 0, 0, fake, None),
                L.rr_render_indirect(None, pc, po, d, ph, None),
                L.rr_render_indirect_device(None, pc, po, d, fake, None))

    for kw in (dict(samples=0), dict(samples=-1), dict(samples=1025)):
        assert all_entries(ind(**kw)) == (ARG, ARG, ARG), kw
        assert "samples" in err()
    for kw in (dict(remaining=-1), dict(remaining=9), dict(remaining=2**31 - 1)):  # RR_MAX_DEPTH is 8
        assert all_entries(ind(**kw)) == (LIM, LIM, LIM), kw
        assert "remaining" in err()
    # null pointers: the descriptor, the context, the camera, the options, the outputs
    assert all_entries(None) == (ARG, ARG, ARG)
    assert all_entries(ind()) == (ARG, ARG, ARG) and "null context" in err()
    assert all_entries(ind(samples=1024, remaining=8)) == (ARG, ARG, ARG) and "null context" in err()  # the boundary values pass
    assert L.rr_render_indirect(None, None, po, ind(), ph, None) == ARG
    assert L.rr_render_indirect(None, pc, None, ind(), ph, None) == ARG
    assert L.rr_render_indirect(None, pc, po, ind(), None, None) == ARG
    assert L.rr_render_indirect_device(None, None, po, ind(), fake, None) == ARG
    assert L.rr_render_indirect_device(None, pc, None, ind(), fake, None) == ARG
    assert L.rr_render_indirect_device(None, pc, po, ind(), None, None) == ARG
    assert (host == SENT).all()


def test_rays_are_the_occlusion_directions_from_the_points(R):
    rng = np.random.default_rng(20261021)
    N = np.concatenate([np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0.6, 0.8, -0.0]], np.float64),
                        unit(rng.normal(size=(61, 3)))])
    P = rng.uniform(-5, 5, size=(65, 3))
    for K in (1, 3, 64, 65):
        for first in (0, 130, 2**32 - 70):
            ind = R.Indirect(K, 2, seed=7 + K)
            rays = R.indirect_rays(P, N, ind, first)
            assert rays.shape == (65 * K, 6) and rays.dtype == np.float64 and rays.flags.c_contiguous
            # composed by hand: ray i * K + k is (P[i], ao_directions[i][k]); the seed is the descriptor's, the hash index
            # first + i; `remaining` plays no part
            w = R.ao_directions(N, R.Ao(K, 123.0, seed=7 + K), first)
            for i in (0, 1, 33, 64):
                for k in sorted({0, K // 2, K - 1}):
                    assert rays[i * K + k].tolist() == P[i].tolist() + w[i, k].tolist(), (K, first, i, k)
            assert np.array_equal(rays[:, 0:3].reshape(65, K, 3), np.broadcast_to(P[:, None, :], (65, K, 3)))
            assert np.array_equal(rays[:, 3:6].reshape(65, K, 3), w)
            assert np.array_equal(rays, R.indirect_rays(P, N, R.Indirect(K, 0, seed=7 + K), first))
            # a window is a slice: point i's rays depend on first + i alone
            assert np.array_equal(R.indirect_rays(P[5:9], N[5:9], ind, first + 5), rays[5 * K:9 * K])
        # directions are unit to a few ulp and never below the surface (ao_direction's properties), and taken as they are
        d = R.indirect_rays(P, N, R.Indirect(K), 0)[:, 3:6].reshape(65, K, 3)
        assert np.abs(np.sqrt((d * d).sum(axis=2)) - 1.0).max() <= 4 * 2.0**-52
        assert ((d * N[:, None, :]).sum(axis=2) >= 0.0).all()
    with pytest.raises(ValueError):
        R.indirect_rays(P[:3], N[:4], R.Indirect(2))


def test_resolve_is_the_in_order_mean(R):
    c = np.array([[1.0, 2.0, 3.0], [0.5, 0.25, 0.125], [1e-17, 1e17, -1.0],
                  [4.0, 4.0, 4.0], [1.0, 1.0, 1.0], [1.0, -1e17, 1.0]])
    got = R.indirect_resolve(c, 3)
    want = [[((1.0 + 0.5) + 1e-17) / 3.0, ((2.0 + 0.25) + 1e17) / 3.0, ((3.0 + 0.125) + -1.0) / 3.0],
            [((4.0 + 1.0) + 1.0) / 3.0, ((4.0 + 1.0) + -1e17) / 3.0, ((4.0 + 1.0) + 1.0) / 3.0]]
    assert got.tolist() == want
    assert R.indirect_resolve(c, 1).tolist() == c.tolist()
    assert R.indirect_resolve(c, 6).shape == (1, 3)
    # the order matters in f64 and is increasing k; the division is one, not a multiplication by a reciprocal
    x = np.array([[1e16, 0, 0], [1.0, 0, 0], [1.0, 0, 0]])
    assert R.indirect_resolve(x, 3)[0, 0] == ((1e16 + 1.0) + 1.0) / 3.0 != (1e16 + (1.0 + 1.0)) / 3.0
    assert R.indirect_resolve(np.ones((49, 3)), 49)[0, 0] == 49.0 / 49.0
    assert R.indirect_resolve(np.full((7, 3), 0.1), 7)[0, 1] == ((((((0.1 + 0.1) + 0.1) + 0.1) + 0.1) + 0.1) + 0.1) / 7.0


def test_compose_adds_the_bounce_where_a_sample_hit(R):
    base = np.array([[[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]], [[1.0, 0.0, 0.25], [0.0, 0.0, 0.0]]])
    ind = np.array([[[0.3, 0.1, 0.7], [9.0, 9.0, 9.0]], [[0.5, 0.5, 0.5], [0.2, 0.4, 0.6]]])
    alb = np.array([[[1.0, 0.5, 0.25], [7.0, 7.0, 7.0]], [[0.1, 0.2, 0.3], [1.0, 1.0, 1.0]]])
    obj = np.array([[0, -1], [2, 1]], np.int32)
    kd = np.array([0.9, 0.7, 0.3])
    got = R.indirect_compose(base, ind, alb, obj, kd)
    assert got.shape == (2, 2, 3) and got.dtype == np.float64
    assert got[0, 0].tolist() == [0.1 + (1.0 * 0.9) * 0.3, 0.2 + (0.5 * 0.9) * 0.1, 0.3 + (0.25 * 0.9) * 0.7]
    assert got[0, 1].tolist() == [0.5, 0.5, 0.5]  # a miss keeps the colour frame's value, whatever the other planes hold
    assert got[1, 0].tolist() == [1.0 + (0.1 * 0.3) * 0.5, 0.0 + (0.2 * 0.3) * 0.5, 0.25 + (0.3 * 0.3) * 0.5]
    assert got[1, 1].tolist() == [(1.0 * 0.7) * 0.2, (1.0 * 0.7) * 0.4, (1.0 * 0.7) * 0.6]
    # a NaN in a miss's planes does not leak; flat inputs are taken in the frame's shape
    ind2 = ind.copy()
    ind2[0, 1] = np.nan
    assert np.array_equal(R.indirect_compose(base, ind2.reshape(4, 3), alb.reshape(-1), obj.reshape(-1), kd), got)
    assert np.array_equal(R.indirect_compose(base, np.zeros_like(ind), alb, obj, kd), base)


YAML = """camera:
  fov: 60
  from: [0, 2.5, -5.0]
  to: [0, 1, 0]
  up: [0, 1, 0]
lights:
  - type: point
    color: [1, 1, 1]
    position: [-10, 10, -10]
scene:
  - type: plane
    transforms: []
    material:
      pattern:
        type: solid
        color: [1, 1, 1]
        transforms: []
      ambient: 0.1
      diffuse: 0.625
      specular: 0
      shininess: 200
  - type: sphere
    transforms:
      - type: translate
        amount: [0, 1, 2]
    material:
      pattern:
        type: solid
        color: [1, 0, 0]
        transforms: []
      ambient: 0.1
      diffuse: 0.25
      specular: 0.9
      shininess: 200
      reflective: 0.5
"""


def test_object_diffuse(R):
    b = R.SceneBuilder()
    b.point_light((-5, 6, -4), (1, 1, 1))
    b.plane(material=(0.1, 0.8, 0.0, 50.0, 0.0, 0.0, 1.0))
    g = b.group()
    b.sphere(material=(0.1, 0.35, 0.3, 50.0, 0.2, 0.0, 1.0), parent=g)
    b.cube()  # the default material: diffuse 0.9
    kd = R.object_diffuse(b)
    assert kd.dtype == np.float64 and kd.shape == (4,)
    assert kd[0] == 0.8 and kd[2] == 0.35 and kd[3] == 0.9
    d = b.desc()
    assert d.material[1] < 0 and kd[1] == 0.0  # a group has no material and is never a first hit
    assert [kd[i] for i in (0, 2, 3)] == [d.mat[7 * d.material[i] + 1] for i in (0, 2, 3)]
    s = R.YamlScene(YAML, 8, 8)
    assert R.object_diffuse(s).tolist() == [0.625, 0.25]


def test_pass_split(tmp_path):
    """rray_amd/csrc/frame_plan.hpp plan_indirect_passes, compiled with g++ into tests/native/indirect_pass_check.cpp.
    The expectations are derived by hand from the definition: passes of whole points, a multiple of 64 each but the last
    (so every pass starts at a ray index that is a multiple of 64 too); by default the largest such count with at most
    2^22 rays and at least 64 points; an override rounded up to 64; either capped by the batch rounded down to 64 (at
    least 64) and kept below 2^32 rays."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "indirect_pass_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "rray_amd", "csrc"),
                    os.path.join(HERE, "native", "indirect_pass_check.cpp"), "-o", exe], check=True)
    rows = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        kind, name, *fields = line.split()
        assert kind == "ind" and name not in rows
        rows[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}

    def check(name, **want):
        assert {k: rows[name][k] for k in want} == want, (name, rows[name])

    for name in ("none", "no_samples", "no_batch"):
        check(name, points=0, passes=0, count=0)
    check("n1_k1_pass64", points=64, passes=1, count=1, sum=1, largest=1, smallest=1, pass_rays=1)
    check("n63_k3_pass64", points=64, passes=1, count=1, sum=63, largest=63, pass_rays=189)
    check("n64_k1024_pass64", points=64, passes=1, count=1, sum=64, largest=64, pass_rays=65536)
    check("n65_k3_pass64", points=64, passes=2, count=2, sum=65, largest=64, smallest=1, misaligned=0, pass_rays=192)
    check("n65_k1024_pass64", points=64, passes=2, count=2, sum=65, largest=64, smallest=1, misaligned=0)
    check("n65_k3_pass1", points=64, passes=2, count=2, sum=65, smallest=1, misaligned=0)
    check("n384_k16_pass65", points=128, passes=3, count=3, sum=384, largest=128, smallest=128, misaligned=0)
    check("n1_k1", points=2**22, passes=1, count=1, sum=1)
    check("n65_k1024", points=4096, passes=1, count=1, sum=65, pass_rays=65 * 1024)
    hd = 1920 * 1080
    check("hd_k1", points=2**22, passes=1, count=1, sum=hd, pass_rays=hd)
    check("hd_k3", points=1398080, passes=2, count=2, sum=hd, misaligned=0, pass_rays=1398080 * 3)  # 1 398 101 rounded down
    assert 1398080 % 64 == 0 and 1398080 * 3 <= 2**22 < (1398080 + 64) * 3
    check("hd_k4", points=2**20, passes=2, count=2, sum=hd, largest=2**20, smallest=hd - 2**20, misaligned=0,
          pass_rays=2**22)
    check("hd_k1024", points=4096, passes=507, count=507, sum=hd, misaligned=0, pass_rays=2**22)
    assert 506 * 4096 < hd <= 507 * 4096
    check("k100000", points=64, passes=16, sum=1000, smallest=40)  # 41 points' worth of rays: at least 64 points
    check("hd_k4_batch1024", points=1024, passes=2025, count=2025, sum=hd, largest=1024, smallest=1024, misaligned=0)
    assert 2025 * 1024 == hd
    check("n3000_k1_batch1100", points=1088, passes=3, count=3, sum=3000, largest=1088, smallest=3000 - 2 * 1088,
          misaligned=0)
    check("n3000_k1_batch1100_pass4096", points=1088, passes=3, count=3, sum=3000)
    check("n100_k1_batch10", points=64, passes=2, count=2, sum=100, smallest=36)
    check("huge_override_k1024", points=4194240, passes=3, count=3, sum=10**7, misaligned=0, pass_rays=4194240 * 1024)
    assert 4194240 % 64 == 0 and 4194240 * 1024 < 2**32 <= (4194240 + 64) * 1024
    check("huge_override_k1", points=2**32 - 64, passes=1, count=1, sum=1000)
