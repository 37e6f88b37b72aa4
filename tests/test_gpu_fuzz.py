"""Exact-cull fuzz on the GPU: seeded adversarial scenes (tests/scene_fuzz.py) rendered through the C ABI
must equal the oracle bit for bit, with the same ray / shadow-ray / shading-event counts.

The kernels test only the nodes their conservative f32 culls cannot reject; the
reference tests every primitive (scene.rs:97-106).  A margin that is too tight shows up as a missed hit —
a wrong pixel and a changed counter — in exactly the scenes the configs never render: extreme scales,
far cameras, near-parallel bundles, sheared group hierarchies, grazing planes, lights at surfaces.  A
failing seed prints its scene (tests/scene_fuzz.py builds it again from the seed alone).

The one arithmetic difference the kernels keep on purpose is the specular power: they compute the
correctly rounded x^n for integer shininess, while the reference's f64::powf is libm's
pow (<= 0.52 ulp, not always correctly rounded).  So the GPU canvas must equal, bit for bit, the oracle
with correctly rounded powers (oracle pow_mode 1, a diagnostic switch), and may differ from the
libm-pow oracle only in samples where the two oracles themselves differ (a last-ulp pow difference,
never a walk or cull error)."""
import contextlib
import os

import numpy as np
import pytest

import scene_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = range(96)


@pytest.fixture(scope="module")
def renderer():
    import rray_amd

    if rray_amd.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")
    r = rray_amd.Renderer(0)
    yield r
    r.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_scene_bit_exact(renderer, seed):
    P, spec, depth, cat = F.build(seed)
    aa = 2 if seed % 3 == 0 else 1
    W, H = (24, 16) if aa == 2 else (32, 24)
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    got = renderer.render(cam, aa=aa, max_depth=depth, canvas=True)
    # libm pow (the reference's own arithmetic) and correctly rounded x^n
    canvas_cr, st_cr, (canvas, st) = F.oracle_frame(P, ocam, depth, libm=True)
    F.check_frame(got, P, f"seed {seed} ({cat}) {W}x{H} aa{aa}", canvas_cr, st_cr, libm=(canvas, st))
    assert float(np.max(np.abs(got["avg"] - P.o.aa_average(canvas, aa)))) <= 1e-12


@pytest.mark.parametrize("seed", F.GENERAL_SEEDS)
def test_general_fuzz_bit_exact(renderer, seed):
    """The general kernels (tests/scene_fuzz.py build_general: cones, tori at scales 1e-3 to 1e3 seen from far, nested
    and glass CSG, pattern trees, textures, everything mixed in sheared groups at depth 5): the canvas must equal the
    oracle's (correctly rounded powers) bit for bit, with the same ray / shadow-ray / shading-event counts, and may
    differ from the libm-pow oracle only where the two oracles differ.

    Seeds 1 and 19 (tori seen from 1e5 tube sizes away) found 355 and 291 of 768 samples that differed:
    there the quartic's coefficients cancel to noise and the reference's find_roots_quartic returns roots up to 4e4
    units off the surface; the reference tests every leaf and shades that speckle, so a torus, and every container
    above it, has no cull."""
    P, spec, depth, cat = F.build_general(seed)
    aa = 2 if seed % 5 == 0 else 1
    W, H = (24, 16) if aa == 2 else (32, 24)
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    got = renderer.render(cam, aa=aa, max_depth=depth, canvas=True)
    # libm pow (the reference's own arithmetic) and correctly rounded x^n
    canvas_cr, st_cr, (canvas, st) = F.oracle_frame(P, ocam, depth, libm=True)
    F.check_frame(got, P, f"seed {seed} ({cat}) {W}x{H} aa{aa}", canvas_cr, st_cr, libm=(canvas, st))
    assert float(np.max(np.abs(got["avg"] - P.o.aa_average(canvas, aa)))) <= 1e-12


@pytest.mark.parametrize("seed", range(32))
def test_area_light_fuzz_bit_exact(renderer, seed):
    """Area lights (light.rs:47-96) with occluders at the edge of the light-hull pre-test's capsule
    (render_levels.inc area_may_shadow: events whose hull no node reaches skip their level^2 walks): the
    canvas must equal the oracle's (correctly rounded powers) bit for bit, with the same ray counts."""
    P, spec, depth, cat = F.build_area(seed)
    aa = 2 if seed % 2 else 1
    W, H = (24, 16) if aa == 2 else (40, 24)
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    got = renderer.render(cam, aa=aa, max_depth=depth, seed=seed, canvas=True)
    canvas_cr, st = F.oracle_frame(P, ocam, depth, seed)
    F.check_frame(got, P, f"seed {seed} ({cat}) {W}x{H} aa{aa}", canvas_cr, st)


@pytest.mark.parametrize("seed", range(48))
def test_own_skip_fuzz_bit_exact(renderer, seed):
    """The own-object skip (shadow and reflected rays skip the object they leave) at its edges
    (tests/scene_fuzz.py build_own): lights on the tangent planes of visible points, lights inside spheres, the camera
    inside a sphere, sheared spheres and scaled planes, 1e-3..1e3 spheres seen from far with narrow fields of view,
    grazing mirrors, an area light straddling tangent planes.  The canvas must equal the oracle's (correctly rounded
    powers) bit for bit, with the same ray counts."""
    P, spec, depth, cat = F.build_own(seed)
    aa = 2 if seed % 4 == 3 else 1
    W, H = (24, 16) if aa == 2 else (40, 24)
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    got = renderer.render(cam, aa=aa, max_depth=depth, seed=seed, canvas=True)
    canvas_cr, st = F.oracle_frame(P, ocam, depth, seed)
    F.check_frame(got, P, f"seed {seed} ({cat}) {W}x{H} aa{aa}", canvas_cr, st)


# --- area lights across every kernel variant, light mix and level (scene_fuzz.build_area_mix) ----------------------

MIX_IDENTITY_SEEDS = (8, 33, 42, 19, 44, 37, 30, 55)  # one scene per family, of different seed // 8
MIX_SWITCHES = ("RRAY_GLOBAL_CULLS", "RRAY_NO_CHAIN", "RRAY_NO_TREE", "RRAY_UNFUSED", "RRAY_DEEP")


def mix_frame_size(seed, cat):
    """24 x 16 aa 2 or 40 x 24 aa 1 in turn; the `levels` family at its own size -> (W, H, aa)"""
    if cat == "levels":
        return F.MIX_LEVELS_SIZE + (1,)
    return (24, 16, 2) if (seed // 8) % 2 else (40, 24, 1)


@pytest.mark.parametrize("seed", F.AREA_MIX_SEEDS)
def test_area_mix_fuzz_bit_exact(renderer, seed):
    """Area lights outside build_area's envelope (tests/scene_fuzz.py build_area_mix: 8 to 600 nodes, two to five lights
    in every order, levels up to 181, general shapes and CSG, pattern trees, glass, degenerate light geometry, umbrae;
    coloured and black lights, black surfaces): the canvas must equal the oracle's (correctly rounded powers) bit for
    bit, with the same ray / shadow-ray / shading-event counts.  tests/test_area_mix_host.py holds the kernel variant
    of every frame and shows that the scenes shadow partly, wholly and not at all."""
    P, spec, depth, cat = F.build_area_mix(seed)
    W, H, aa = mix_frame_size(seed, cat)
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    got = renderer.render(cam, aa=aa, max_depth=depth, seed=seed, canvas=True)
    canvas_cr, st = F.oracle_frame(P, ocam, depth, seed)
    F.check_frame(got, P, f"seed {seed} ({cat}) {W}x{H} aa{aa}", canvas_cr, st)


@pytest.mark.parametrize("seed", F.MIX_DEPTH0_SEEDS)
def test_area_mix_depth0_bit_exact(renderer, seed):
    """One scene without glass per (G, PRE, CP) at max_depth 0: the fused level-0 kernels' area path, which the frames
    above reach only through the chain and tree kernels."""
    P, spec, depth, cat = F.build_area_mix(seed)
    W, H, aa = mix_frame_size(seed + 8, cat)  # the other size than the scene's frame above
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    renderer.upload(P.b)
    renderer.kernel_profile(True)
    try:
        got = renderer.render(cam, aa=aa, max_depth=0, seed=seed, canvas=True)
        kt = {k: v[1] for k, v in renderer.kernel_times().items() if v[1]}
    finally:
        renderer.kernel_profile(False)
    canvas_cr, st = F.oracle_frame(P, ocam, 0, seed)
    F.check_frame(got, P, f"seed {seed} ({cat}) depth 0 {W}x{H} aa{aa}", canvas_cr, st)
    assert set(kt) <= {"trace_shade", "aa"} and kt["trace_shade"] >= 1, kt


def level_limit_scene(level):
    """A floor and three spheres under one wide area light, seen from above so that every sample of a 16 x 16 frame hits:
    one block of 256 shading events, most of them inside some sphere's penumbra -> (Pair, camera spec)"""
    P = F.Pair()
    M = P.M
    P.obj("plane", M.identity(), (0.1, 0.8, 0.4, F.SHININESS, 0.3, 0.0, 1.0), (0.9, 0.8, 0.7))
    for x, y, z, r in ((-1.2, 1.6, 0.4, 0.8), (1.1, 2.2, -0.3, 0.7), (0.1, 1.2, 1.4, 0.6)):
        P.obj("sphere", F._mul(M, M.scale(r, r, r), M.translate(x, y, z)), (0.1, 0.7, 0.5, F.SHININESS, 0.2, 0.0, 1.0),
              (0.3, 0.6, 0.9))
    P.area_light((-3.0, 6.0, -3.0), (6.0, 0.0, 0.5), (0.0, 0.5, 6.0), level, (1.0, 0.9, 0.8))
    return P, {"from_": (0.5, 9.0, -4.0), "to": (0.0, 0.0, 0.5), "up": (0.0, 1.0, 0.0), "fov": 0.7}


@pytest.mark.parametrize("level", (256, 1024))
def test_area_level_limit(renderer, level):
    """area_shadow_block deals nh * level^2 (event, sample) pairs over the block and indexes them with small_div: at
    level 256 a full block holds 2^24 pairs (the bound small_div's comment used to state), at RR_MAX_AREA_LEVEL = 1024
    2^28.  A 16 x 16 aa 1 frame in which every sample hits, so one block holds 256 events, against the oracle bit for
    bit with equal counters (256 * level^2 shadow rays at level 0 alone).  Depth 1: the reflected rays' events share
    blocks too.  Measured: the level-1024 case takes 3.1 s on 16 CPU threads (the oracle's 2.8e8 shadow rays, about 3 s, plus
    the render; the oracle alone 6.1 s on 8 threads), the level-256 case 0.2 s; under the 10 s at which the frame would be halved."""
    P, spec = level_limit_scene(level)
    cam, ocam = F.cameras(P, spec, 16, 16)
    assert (F.first_hits(P, ocam) >= 0).all()
    renderer.upload(P.b)
    got = renderer.render(cam, aa=1, max_depth=1, seed=5, canvas=True)
    canvas_cr, st = F.oracle_frame(P, ocam, 1, 5)
    assert st["shadow_rays"] >= 256 * level * level
    F.check_frame(got, P, f"level {level} 16x16", canvas_cr, st)


@contextlib.contextmanager
def mix_switches(**kw):
    saved = {k: os.environ.get(k) for k in MIX_SWITCHES}
    try:
        for k in MIX_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("seed", MIX_IDENTITY_SEEDS)
def test_area_mix_same_binary_identities(renderer, seed):
    """GPU against GPU: the default frame of one scene per family (40 x 24 aa 1 at the scene's depth, so the deep queue
    may take it) equals, bit for bit and in its counters, the frame under each switch that sends it through another
    kernel family — culls in global memory (uploaded again; rr_kernel_times cannot tell that instantiation from the
    LDS one, so there only the equality is checked and the launches must stay as they were), the fused per-level kernels (RRAY_NO_CHAIN), the unfused
    ones (RRAY_UNFUSED; glass: RRAY_NO_TREE) and the deep-chain launch (RRAY_DEEP).  The family that ran is read from
    rr_kernel_times; a switch that does not apply to the scene (RRAY_NO_TREE without glass, the others with it) must
    leave the launches as they were."""
    P, spec, depth, cat = F.build_area_mix(seed)
    glass = F.traits(P)["transparent"]
    assert depth >= 2
    cam, _ = F.cameras(P, spec, 40, 24)

    def frame(at_upload, at_launch):
        with mix_switches(**at_upload):
            renderer.upload(P.b)
        renderer.kernel_profile(True)
        try:
            with mix_switches(**at_launch):
                got = renderer.render(cam, aa=1, max_depth=depth, seed=seed, canvas=True)
            kt = {k: v[1] for k, v in renderer.kernel_times().items()}
        finally:
            renderer.kernel_profile(False)
        return got, kt

    base, kt0 = frame({}, {})
    what = f"seed {seed} ({cat})"
    assert kt0["chain"] >= 1 and not any(kt0[k] for k in ("trace", "n1n2", "shade", "trace_shade", "deep")), (what, kt0)
    for name in MIX_SWITCHES:
        got, kt = frame({name: "1"}, {}) if name == "RRAY_GLOBAL_CULLS" else frame({}, {name: "1"})
        print(f"{what} {name}: {({k: v for k, v in kt.items() if v})}")
        assert np.array_equal(got["canvas"], base["canvas"]) and np.array_equal(got["avg"], base["avg"]), (what, name)
        for key in ("rays", "shadow_rays", "shade_events"):
            assert got["stats"][key] == base["stats"][key], (what, name, key)
        applies = {"RRAY_GLOBAL_CULLS": False, "RRAY_NO_TREE": glass}.get(name, not glass)
        if not applies:
            assert kt == kt0, (what, name, kt, kt0)
        elif name == "RRAY_DEEP":
            assert kt["chain"] >= 1 and kt["deep"] >= 1, (what, name, kt)
        elif name == "RRAY_NO_CHAIN":
            # the fused levels: one trace_shade launch per level
            assert kt["chain"] == 0 and kt["trace_shade"] == depth + 1 and kt["trace"] == 0 and kt["shade"] == 0, (what, name, kt)
        else:  # the unfused levels: a trace and a shade launch per level, n1 / n2 scans under glass
            assert kt["chain"] == 0 and kt["trace_shade"] == 0 and kt["trace"] >= 2 and kt["shade"] >= 2, (what, name, kt)
            assert not glass or kt["n1n2"] >= 1, (what, name, kt)
    renderer.upload(P.b)
