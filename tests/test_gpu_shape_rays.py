"""The edge-ray batteries of tests/shape_rays.py on the GPU: hit_at, color_at and is_shadowed against the oracle, ray
by ray and bit for bit (np.array_equal; NaNs equal NaNs).  The general kernels (the G = 2 variant, EntriesT<4>,
csg_eval, quartic.inc, pattern_tree, texture_at) restate the reference's f64 operations in the reference's order, so
no tolerance applies and no record is left out.  tests/test_shape_rays_host.py holds the conditions that keep these
tests from passing vacuously (hit fractions, entry counts, both shadow answers, both sub-colours)."""
import time

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library, as in tests/test_gpu_hit.py

import scene_fuzz as F  # noqa: E402,F401
import shape_rays as S  # noqa: E402
from test_gpu_hit import assert_records_equal, oracle_hits, same  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _first_difference(got, want, o, d, what):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(len(got), -1).all(axis=1)).reshape(-1)
    for k in bad[:8]:
        print(f"{what}: ray {k} o={o[k].tolist()} d={d[k].tolist()}: gpu {got[k].tolist()} oracle {want[k].tolist()}")
    return len(bad)


@pytest.mark.parametrize("name", S.leaf_names() + list(S.CSG_NAMES))
def test_edge_rays_equal_the_oracle(R, renderer, name):
    """The identity cone batteries found 524 of 27 200 rays that missed on the GPU where the oracle hits:
    a cone ray with |a| < EPSILON takes t = -c / (2 b) (cone.rs:96-103), half the distance to the infinite cone, a
    point that need not lie inside the cone's box; the reference tests every leaf and reports it, so a cone, and every
    container above it, has no cull: what bounds it is the exact box test of its groups."""
    t0 = time.perf_counter()
    B = S.build(name)
    P = B.P
    renderer.upload(P.b)
    rays = list(zip(B.o.tolist(), B.d.tolist()))
    try:
        want = oracle_hits(R, P.o, rays, {v: k for k, v in P.ids.items()})
        got = renderer.hit_at(B.o, B.d)
        st = renderer.last_stats()
        assert_records_equal(got, want, f"{name} hit_at")
        hits = int((want["object"] >= 0).sum())
        assert (st["rays"], st["samples"], st["n1n2_scans"]) == (len(rays), len(rays), hits), st
        assert st["nan_rays"] == 0 and P.o.stats()["nan_sorts"] == 0
        # colours: correctly rounded powers on both sides, recursion depth 3
        P.o.set_pow_mode(1)
        want_c = np.array([P.o.color_at(o, d, 3) for o, d in rays])
        got_c = renderer.color_at(B.o, B.d, remaining=3)
        assert _first_difference(got_c, want_c, B.o, B.d, f"{name} color_at") == 0
        assert renderer.last_stats()["nan_rays"] == 0
        want_s = np.array([P.o.is_shadowed(tuple(p), tuple(l)) for p, l in zip(B.shadow_p, B.shadow_l)])
        got_s = renderer.is_shadowed(B.shadow_p, B.shadow_l)
        bad = np.argwhere(got_s != want_s).reshape(-1)
        for k in bad[:8]:
            print(f"{name} is_shadowed: pair {k} p={B.shadow_p[k].tolist()} light={B.shadow_l[k].tolist()}: gpu {got_s[k]} "
                  f"oracle {want_s[k]}")
        assert len(bad) == 0
    except AssertionError:
        print("\n".join(P.log))
        raise
    print(f"{name}: {len(rays)} rays, {hits} hits, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("alone", [True, False], ids=["alone", "beside"])
@pytest.mark.parametrize("name", S.PATTERN_NAMES)
def test_pattern_points_equal_the_oracle(R, renderer, name, alone):
    """Rays straight down onto a plane carrying each pattern kind, at integers +- 0..2 ulps, negative odd integers,
    -0.0, 1e9, beyond 2^31, integer radii: color_at, and the albedo plane of a camera looking down at the origin."""
    import oracle

    P, o, d, plane, pat = S.build_pattern(name, alone)
    renderer.upload(P.b)
    want = np.array([P.o.color_at(tuple(a), tuple(b), 3) for a, b in zip(o, d)])
    got = renderer.color_at(o, d, remaining=3)
    assert _first_difference(got, want, o, d, f"pattern {name} color_at") == 0
    # the albedo plane: pattern_at_object(object, over_point) per sample (material.rs:77-80)
    Hs, V = 24, 16
    t = P.M.view_transform((0.3, 9.0, 0.2), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    cam, ocam = R.camera(Hs, V, 1.2, t), oracle.Oracle.camera(Hs, V, 1.2, t)
    albedo = np.zeros((V * Hs, 3))
    ids = {v: k for k, v in P.ids.items()}
    for y in range(V):
        for x in range(Hs):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            xs = P.o.intersect(ro[:3], rd[:3])
            hit = next((k for k, e in enumerate(xs) if e[0] >= 0.0), None)
            if hit is not None and ids[xs[hit][1]] == plane:
                c = P.o.prepare_computations(ro[:3], rd[:3], xs, hit)
                albedo[y * Hs + x] = P.o.pattern_at(pat[1], P.o.world_to_object(xs[hit][1], c["over_point"][:3])[:3])
    aov = renderer.render_aov(cam, planes=("object", "albedo"))
    on_plane = (aov["object"] == plane).reshape(-1)
    assert on_plane.mean() > 0.5
    assert same(aov["albedo"].reshape(-1, 3)[on_plane], albedo[on_plane]), f"pattern {name}: albedo plane"


@pytest.mark.parametrize("kind", S.TEXTURED_KINDS)
def test_textured_shapes_equal_the_oracle(R, renderer, kind):
    """Textures of 1 x 1, 2 x 3 and 5 x 1 texels on every shape kind, hit at the poles and the seam of the sphere, at
    cube edges where two faces tie, at the cap / side boundary of a cylinder and a cone (u and v exactly 0 and 1)."""
    for tex in range(3):
        P, o, d = S.build_textured(kind, tex)
        renderer.upload(P.b)
        want = np.array([P.o.color_at(tuple(a), tuple(b), 3) for a, b in zip(o, d)])
        got = renderer.color_at(o, d, remaining=3)
        assert _first_difference(got, want, o, d, f"texture {tex} on {kind}") == 0
