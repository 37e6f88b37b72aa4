"""`rray --samples S --aperture A --focus F --pixel-jitter`: lens frames from the command line (rr_render_lens, DESIGN.md
§3.20).  Each flag selects the lens path; none may be combined with -a other than 1, --adaptive or --aov.  The argument
handling never reaches the GPU; the rendering test runs the binary end to end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rray_amd", "bin", "rray")
SCENE = os.path.join(ROOT, "scenes", "c1_readme.yaml")
COMBINE = "cannot be combined"


def _run(args, cwd=None, timeout=120):
    if not os.path.exists(CLI):
        pytest.fail("rray_amd/bin/rray is not built (run __graft_entry__.build())")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_lens_options_are_parsed(tmp_path):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in ("--samples <S>", "--aperture <A>", "--focus <F>", "--pixel-jitter"):
        assert flag in r.stderr, flag
    missing = str(tmp_path / "nope.yaml")
    # accepted, alone or together: the run gets as far as the missing scene file (exit 1), not a usage error (exit 2)
    for flags in (["--samples", "4"], ["--aperture", "0.25"], ["--focus", "5.5"], ["--pixel-jitter"],
                  ["--samples", "8", "--aperture", "0.1", "--focus", "4", "--pixel-jitter", "-a", "1"]):
        r = _run(["-s", missing, "-o", str(tmp_path / "o.png")] + flags)
        assert r.returncode == 1 and "File does not exist" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())  # nothing written
    # values
    for flags, text in ((["--samples"], "missing value"), (["--samples", "0"], "1 to 4096"),
                        (["--samples", "4097"], "1 to 4096"), (["--samples", "x"], "1 to 4096"),
                        (["--aperture", "-0.1"], ">= 0"), (["--aperture", "nan"], ">= 0"), (["--aperture"], "missing value"),
                        (["--focus", "0"], "> 0"), (["--focus", "inf"], "> 0"), (["--focus"], "missing value")):
        r = _run(["-s", "x.yaml"] + flags)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)


@pytest.mark.parametrize("lens", [["--samples", "4"], ["--aperture", "0.2"], ["--focus", "3"], ["--pixel-jitter"]],
                         ids=["samples", "aperture", "focus", "jitter"])
@pytest.mark.parametrize("other", [["-a", "2"], ["--adaptive", "0.1"], ["--aov", "p"]], ids=["aa", "adaptive", "aov"])
def test_forbidden_combinations_are_usage_errors(tmp_path, lens, other):
    for args in (lens + other, other + lens):
        r = _run(["-s", SCENE, "-o", str(tmp_path / "o.png")] + args)
        assert r.returncode == 2 and COMBINE in r.stderr and "Usage:" in r.stderr, (args, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_lens_png_equals_the_quantised_library_frame(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    import rray_amd as R

    W, H = 40, 30
    scene = R.YamlScene(open(SCENE).read(), W, H, 1)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        for k, (flags, lens) in enumerate((
                (["--samples", "4", "--aperture", "0.25", "--focus", "5.5", "--pixel-jitter"],
                 R.Lens(4, True, 0.25, 5.5)),
                (["--samples", "3"], R.Lens(3)),
                (["--pixel-jitter"], R.Lens(1, True)))):
            out = tmp_path / f"lens{k}.png"
            r = _run(["-W", str(W), "-H", str(H), "-s", SCENE, "-o", str(out)] + flags)
            assert r.returncode == 0, r.stderr
            got = np.asarray(PIL.open(out).convert("RGBA"))
            want = R.quantize(rend.render_lens(scene.camera, lens)["avg"])
            assert got.shape == (H, W, 4) and np.array_equal(got, want), flags
        plain = R.quantize(rend.render(scene.camera)["avg"])
    finally:
        rend.close()
    assert not np.array_equal(got, plain)  # the jittered frame is not the plain one
    assert len(np.unique(got.reshape(-1, 4), axis=0)) > 50  # a real image, not a constant
