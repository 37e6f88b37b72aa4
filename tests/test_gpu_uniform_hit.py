"""Hit-uniform tiles in the flat fused kernels (shade_body.inc UH): planes' normals from the per-node
table, and tiles whose 64 lanes hit one node shaded from scalar records.

Every case renders with the path on and with RRAY_NO_UNIFORM_HIT=1 (the per-lane code), through the per-tile launch
(RRAY_NO_PERSIST=1) and through the loop (RRAY_PERSIST_BLOCKS=2), and asserts the same image and canvas bit for bit
(np.array_equal) and the same counters.  Cases marked with an oracle size are also compared with the CPU oracle by the
comparison of tests/test_gpu_parity.py (restated here).  The switches are read at launch, so one process renders every
variant; which launch a frame took is asked of the context and asserted.  The path lives in the kernels with global
culls, which scenes of a few nodes leave for the LDS-cull kernels: every scene is uploaded under RRAY_GLOBAL_CULLS=1
(read at upload), so that the small scenes here run the kernels the benchmark scene runs."""
import contextlib
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
COUNTERS = ("rays", "shadow_rays", "shade_events", "prim_tests", "exact_flops", "wave_visits")
SWITCHES = ("RRAY_NO_PERSIST", "RRAY_PERSIST_BLOCKS", "RRAY_PERSIST_HEADS", "RRAY_NO_UNIFORM_HIT", "RRAY_GLOBAL_CULLS")
TOL = 1e-5  # tests/test_gpu_parity.py


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


@contextlib.contextmanager
def switches(**kw):
    """the launch switches set for the block (None: unset), every one restored after it"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _compare(got, ref, label):  # tests/test_gpu_parity.py _compare
    err = float(np.max(np.abs(got - ref))) if got.size else 0.0
    exact = float(np.mean(got == ref)) if got.size else 1.0
    print(f"{label}: max|d|={err:.3g} bit-exact={exact:.6f}")
    assert np.all(np.isfinite(got)), label
    assert err <= TOL, f"{label}: max |delta| {err} > {TOL}"


CHECKER = """
      pattern:
        type: checker
        color_a: [0.25, 0.25, 0.75]
        color_b: [0.75, 0.75, 0.75]
        transforms: []
"""
DOWN = """
camera:
  fov: 60
  from: [0.3, 6, 0.2]
  to: [0.3, 0, 0.25]
  up: [0, 0, 1]
"""
# a sphere above the camera (never seen) between the light and the floor: its shadow covers part of the view
SHADOW_CASTER = """
  - type: sphere
    transforms:
      - {type: scale, amount: [0.5, 0.5, 0.5]}
      - {type: translate, amount: [1, 10, 1]}
"""


def floor_scene(material, lights="[{type: point, color: [1, 1, 1], position: [0, 20, 0]}]"):
    return DOWN + f"lights: {lights}\nscene:\n  - type: plane\n    transforms: []\n{material}" + SHADOW_CASTER


FLOOR = floor_scene("    material:\n      specular: 0\n" + CHECKER)
FLOOR_DEFAULT = floor_scene("")  # Material::default: no pattern, white
FLOOR_SOLID = floor_scene("    material:\n      pattern: {type: solid, color: [0.2, 0.7, 0.4]}\n")
FLOOR_NESTED = floor_scene("""    material:
      pattern:
        type: stripe
        pattern_a:
          type: checker
          color_a: [1, 0, 0]
          color_b: [0, 1, 0]
          transforms: [{type: scale, amount: [0.5, 0.5, 0.5]}]
        pattern_b:
          type: checker
          color_a: [0, 0, 1]
          color_b: [1, 1, 0]
          transforms: [{type: rotate, axis: y, angle: 30}]
        transforms: [{type: scale, amount: [1.5, 1, 1]}]
""")
# a negative intensity component: (I * 0) and the sums around it carry negative zeros
FLOOR_NEGATIVE = floor_scene("    material:\n      specular: 0\n" + CHECKER,
                             "[{type: point, color: [1, -0.5, 0.25], position: [0, 20, 0]}]")

# a mirrored floor: the diagonal inverse has negative entries, so the kernels' normal has negative zeros where the
# reference's has positive ones; the table entry is then not marked usable and the tile keeps the per-lane code
FLOOR_MIRRORED = (DOWN + "lights: [{type: point, color: [1, 1, 1], position: [0, 20, 0]}]\nscene:\n  - type: plane\n"
                  "    transforms:\n      - {type: scale, amount: [-2, 1, -3]}\n      - {type: translate, amount: [0.5, 0, 1]}\n"
                  "    material:\n      specular: 0\n" + CHECKER + SHADOW_CASTER)

GENERAL_PLANE = """
camera:
  fov: 60
  from: [0, -3, -4]
  to: [0, 2, 2]
  up: [0, 1, 0]
lights: [{type: point, color: [1, 0.9, 0.8], position: [2, -5, -3]}]
scene:
  - type: plane
    transforms:
      - {type: scale, amount: [1.5, 1, 0.7]}
      - {type: shear, xy: 0.3, xz: 0, yx: 0.1, yz: 0, zx: 0, zy: 0.2}
      - {type: rotate, axis: x, angle: 25}
      - {type: rotate, axis: z, angle: -15}
      - {type: translate, amount: [0, 2, 0]}
    material:
      specular: 0.4
      shininess: 50
      pattern:
        type: ring
        color_a: [0.9, 0.3, 0.2]
        color_b: [0.1, 0.4, 0.8]
        transforms:
          - {type: scale, amount: [0.5, 0.5, 0.5]}
          - {type: rotate, axis: y, angle: 30}
          - {type: translate, amount: [0.3, 0, -0.2]}
"""


def sphere_scene(transforms, cam_from, cam_to, light, fov=30):
    return f"""
camera:
  fov: {fov}
  from: {cam_from}
  to: {cam_to}
  up: [0, 1, 0]
lights: [{{type: point, color: [1, 1, 1], position: {light}}}]
scene:
  - type: sphere
    transforms:
{transforms}
    material:
      specular: 0.9
      shininess: 200
      pattern: {{type: solid, color: [0.8, 0.3, 0.3]}}
"""


SPHERE_DIAG = sphere_scene("      - {type: scale, amount: [3, 2.6, 3]}\n      - {type: translate, amount: [0, 0, 5]}",
                           [0, 0, 0], [0, 0, 5], [-1.5, 1.5, -2])
SPHERE_FULL = sphere_scene("      - {type: scale, amount: [3, 2.6, 3]}\n"
                           "      - {type: shear, xy: 0.2, xz: 0, yx: 0, yz: 0.1, zx: 0, zy: 0}\n"
                           "      - {type: rotate, axis: y, angle: 30}\n      - {type: rotate, axis: z, angle: 10}\n"
                           "      - {type: translate, amount: [0, 0, 5]}", [0, 0, 0], [0, 0, 5], [-1.5, 1.5, -2])
SPHERE_INSIDE = sphere_scene("      - {type: scale, amount: [4, 3, 4]}\n      - {type: rotate, axis: x, angle: 20}",
                             [0, 0, -1], [0, 0.2, 1], [1, 1, 0], fov=70)


def two_planes(lights):
    return f"""
camera:
  fov: 60
  from: [0, 2, -5]
  to: [0, 1, 4]
  up: [0, 1, 0]
lights: {lights}
scene:
  - type: plane
    transforms: []
    material:
      specular: 0
{CHECKER}
  - type: plane
    transforms:
      - {{type: rotate, axis: x, angle: 90}}
      - {{type: rotate, axis: y, angle: 20}}
      - {{type: translate, amount: [0, 0, 4]}}
    material:
      pattern:
        type: stripe
        color_a: [0.9, 0.9, 0.2]
        color_b: [0.2, 0.2, 0.2]
        transforms: []
"""


ONE_LIGHT = "[{type: point, color: [1, 1, 1], position: [-4, 6, -6]}]"
TWO_LIGHTS = ("[{type: point, color: [0.6, 0.6, 0.6], position: [-4, 6, -6]}, "
              "{type: point, color: [0.5, 0.4, 0.3], position: [5, 3, -2]}]")


def yaml_file(name):
    return open(os.path.join(SCENES, name)).read()


# (id, scene text, W, H, max_depth, compared with the oracle)
CASES = [
    ("c2_64x64", yaml_file("c2_s1024.yaml"), 64, 64, 5, True),
    ("c2_160x90_partial_tiles", yaml_file("c2_s1024.yaml"), 160, 90, 5, True),
    ("floor_only", FLOOR, 64, 48, 5, True),
    ("mirrored_floor", FLOOR_MIRRORED, 64, 48, 5, True),
    ("general_plane_from_below", GENERAL_PLANE, 64, 48, 5, True),
    ("sphere_diag", SPHERE_DIAG, 64, 64, 5, True),
    ("sphere_full_inverse", SPHERE_FULL, 64, 64, 5, True),
    ("sphere_from_inside", SPHERE_INSIDE, 64, 48, 5, True),
    ("two_planes", two_planes(ONE_LIGHT), 64, 48, 5, False),
    ("two_planes_two_lights", two_planes(TWO_LIGHTS), 64, 48, 5, False),
    ("default_material", FLOOR_DEFAULT, 48, 40, 5, False),
    ("solid_root", FLOOR_SOLID, 48, 40, 5, False),
    ("stripe_of_checkers", FLOOR_NESTED, 48, 40, 5, False),
    # reflective materials with no depth left: one fused level, which takes the gated kernels (asserted below)
    ("c3_reflective_depth_0", yaml_file("c3_s1024_reflect.yaml"), 64, 64, 0, False),
    ("negative_intensity", FLOOR_NEGATIVE, 64, 48, 5, False),
]


@pytest.mark.parametrize("name,text,W,H,depth,oracle", CASES, ids=[c[0] for c in CASES])
def test_uniform_path_changes_no_result(R, renderer, name, text, W, H, depth, oracle):
    scene = R.YamlScene(text, W, H, 1, obj_root=SCENES)
    with switches(RRAY_GLOBAL_CULLS="1"):
        renderer.upload(scene)
    full_tiles = W % 8 == 0 and H % 8 == 0  # the loop takes frames of whole tiles only
    frames = {}
    for launch, env in (("per_tile", {"RRAY_NO_PERSIST": "1"}), ("loop", {"RRAY_PERSIST_BLOCKS": "2"})):
        for path, off in (("on", None), ("off", "1")):
            with switches(RRAY_NO_UNIFORM_HIT=off, **env):
                frames[(launch, path)] = renderer.render(scene.camera, aa=1, max_depth=depth, canvas=True)
            want = (2, 8) if launch == "loop" and full_tiles else (0, 0)
            assert renderer.resident_launch() == want, (name, launch, path)
    ref = frames[("per_tile", "off")]  # the code as it was
    assert ref["stats"]["rays"] == W * H, "one fused level: the kernels this path lives in"
    for key, got in frames.items():
        assert np.array_equal(got["avg"], ref["avg"]), (name, key, "avg")
        assert np.array_equal(got["canvas"], ref["canvas"]), (name, key, "canvas")
        assert {k: got["stats"][k] for k in COUNTERS} == {k: ref["stats"][k] for k in COUNTERS}, (name, key)
    if oracle:
        from oracle.scene_yaml import build_from_yaml

        o, cam = build_from_yaml(text, W, H, 1, obj_root=SCENES)
        canvas, st = o.render(cam, max_depth=depth, threads=0)
        on = frames[("loop" if full_tiles else "per_tile", "on")]
        _compare(on["canvas"], canvas, f"{name} canvas")
        _compare(on["avg"], o.aa_average(canvas, 1), f"{name} avg")
        assert on["stats"]["shade_events"] == st["shade_events"]
        assert on["stats"]["shadow_rays"] == st["shadow_rays"]
