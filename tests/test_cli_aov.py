"""`rray --aov PREFIX`: the one CLI option beyond the reference's (src/main.rs:49-77).  After the colour PNG it writes
PREFIX_normal.png (normalv * 0.5 + 0.5) and PREFIX_albedo.png, the camera rays' first-hit planes at the supersampled
size, through the colour image's quantisation (canvas.rs:97-100) and PNG writer.  The argument handling never
reaches the GPU; the rendering test runs the binary end to end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rray_amd", "bin", "rray")
SCENE = os.path.join(ROOT, "scenes", "c1_readme.yaml")


def _run(args, cwd=None, timeout=120):
    if not os.path.exists(CLI):
        pytest.fail("rray_amd/bin/rray is not built (run __graft_entry__.build())")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_aov_option_is_parsed(tmp_path):
    r = _run(["--help"])
    assert r.returncode == 0 and "--aov <PREFIX>" in r.stderr
    # accepted: the run gets as far as the missing scene file (exit 1), not a usage error (exit 2)
    r = _run(["-s", str(tmp_path / "nope.yaml"), "--aov", str(tmp_path / "x"), "-o", str(tmp_path / "o.png")])
    assert r.returncode == 1 and "File does not exist" in r.stderr, (r.returncode, r.stderr)
    assert "unexpected argument" not in r.stderr
    assert not list(tmp_path.iterdir())  # nothing written
    r = _run(["-s", "x.yaml", "--aov"])
    assert r.returncode == 2 and "missing value" in r.stderr
    r = _run(["-s", "x.yaml", "--aov", ""])
    assert r.returncode == 2 and "prefix" in r.stderr


@pytest.mark.gpu
def test_aov_pngs_equal_the_library_planes(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    import rray_amd as R

    W, H, aa = 40, 30, 2
    out, prefix = tmp_path / "c1.png", tmp_path / "c1"
    r = _run(["-W", str(W), "-H", str(H), "-a", str(aa), "-s", SCENE, "-o", str(out), "--aov", str(prefix)])
    assert r.returncode == 0, r.stderr
    colour = np.asarray(PIL.open(out).convert("RGBA"))
    normal = np.asarray(PIL.open(str(prefix) + "_normal.png").convert("RGBA"))
    albedo = np.asarray(PIL.open(str(prefix) + "_albedo.png").convert("RGBA"))
    assert colour.shape == (H, W, 4)
    assert normal.shape == albedo.shape == (H * aa, W * aa, 4)  # per sample, never averaged
    scene = R.YamlScene(open(SCENE).read(), W, H, aa)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        ref = rend.render_aov(scene.camera, aa=aa, planes=("normal", "albedo"))
        avg = rend.render(scene.camera, aa=aa)["avg"]
    finally:
        rend.close()
    assert np.array_equal(normal, R.quantize(ref["normal"] * 0.5 + 0.5))
    assert np.array_equal(albedo, R.quantize(ref["albedo"]))
    assert np.array_equal(colour, R.quantize(avg))  # the colour image is the one the CLI writes without the option
    assert len(np.unique(normal.reshape(-1, 4), axis=0)) > 50  # a real image, not a constant
    # without the option nothing but the colour PNG appears
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run(["-W", str(W), "-H", str(H), "-a", str(aa), "-s", SCENE, "-o", "only.png"], cwd=str(plain))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in plain.iterdir()) == ["only.png"]
    assert np.array_equal(np.asarray(PIL.open(plain / "only.png").convert("RGBA")), colour)
