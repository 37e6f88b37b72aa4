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
