"""`rray --denoise I [--denoise-color SIGMA]`: the edge-avoiding denoiser from the command line (rr_denoise, DESIGN.md
§3.22).  With --samples the lens frame's colour image is filtered with the aa 1 first-hit planes of the same camera, with
--ao-samples the PREFIX_ao.png plane with the planes --aov renders; the other sigmas are rray_amd.Denoise's defaults.
Refused (usage error, exit 2) with -a other than 1, with --adaptive, or with neither kind of frame.  The argument handling
never reaches the GPU; the rendering tests run the binary end to end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rray_amd", "bin", "rray")
SCENE = os.path.join(ROOT, "scenes", "c1_readme.yaml")
AREA = os.path.join(ROOT, "scenes", "c5_area_light.yaml")
PLANES = ("depth", "normal", "object", "albedo")


def _run(args, cwd=None, timeout=120):
    if not os.path.exists(CLI):
        pytest.fail("rray_amd/bin/rray is not built (run __graft_entry__.build())")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_denoise_options_are_parsed(tmp_path):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in ("--denoise <I>", "--denoise-color <SIGMA>"):
        assert flag in r.stderr, flag
    missing = str(tmp_path / "nope.yaml")
    # accepted with a lens frame or an occlusion plane, in any order: the run gets as far as the missing scene file
    # (exit 1), not a usage error
    for flags in (["--samples", "4", "--denoise", "3"], ["--denoise", "8", "--pixel-jitter", "--denoise-color", "0.5"],
                  ["--denoise-color", "0", "--denoise", "1", "--aperture", "0.1"],
                  ["--aov", str(tmp_path / "p"), "--ao-samples", "16", "--ao-radius", "0.5", "--denoise", "5"],
                  ["--denoise", "2", "--denoise-color", "1e-3", "--ao-radius", "2", "--ao-samples", "4", "--aov",
                   str(tmp_path / "p"), "-a", "1"]):
        r = _run(["-s", missing, "-o", str(tmp_path / "o.png")] + flags)
        assert r.returncode == 1 and "File does not exist" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())  # nothing written
    # values
    for flags, text in ((["--denoise"], "missing value"), (["--denoise", "0"], "1 to 8"), (["--denoise", "9"], "1 to 8"),
                        (["--denoise", "x"], "1 to 8"), (["--denoise", "-1"], "1 to 8"),
                        (["--denoise", "2", "--denoise-color"], "missing value"),
                        (["--denoise", "2", "--denoise-color", "-0.5"], ">= 0"),
                        (["--denoise", "2", "--denoise-color", "nan"], ">= 0"),
                        (["--denoise", "2", "--denoise-color", "inf"], ">= 0")):
        r = _run(["-s", "x.yaml", "--samples", "2"] + flags)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)


@pytest.mark.parametrize("flags,text", [
    (["--denoise", "3"], "give one of them"),
    (["--denoise", "3", "--aov", "p"], "give one of them"),
    (["--denoise-color", "0.5", "--samples", "2"], "only with --denoise"),
    (["--denoise", "3", "--samples", "2", "-a", "2"], "-a other than 1"),
    (["--denoise", "3", "--aov", "p", "--ao-samples", "4", "--ao-radius", "1", "-a", "2"], "-a other than 1"),
    (["--denoise", "3", "--samples", "2", "--adaptive", "0.1"], "--adaptive"),
    (["--denoise", "3", "--aov", "p", "--ao-samples", "4", "--ao-radius", "1", "--adaptive", "0.1"], "--adaptive"),
    (["--denoise", "3", "--ao-samples", "4", "--ao-radius", "1"], "only together and only with --aov"),
], ids=["no_frame", "aov_alone", "color_alone", "lens_aa2", "ao_aa2", "lens_adaptive", "ao_adaptive", "ao_no_aov"])
def test_refusals_are_usage_errors(tmp_path, flags, text):
    r = _run(["-s", SCENE, "-o", str(tmp_path / "o.png")] + flags, cwd=str(tmp_path))
    assert r.returncode == 2 and text in r.stderr and "Usage:" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_lens_png_equals_the_quantised_denoise_of_the_unfiltered_frame(tmp_path):
    from PIL import Image
    import rray_amd as R

    W, H, S, I, sc = 40, 30, 2, 3, 0.5
    out, raw = tmp_path / "dn.png", tmp_path / "raw.png"
    common = ["-W", str(W), "-H", str(H), "-s", AREA, "--samples", str(S), "--pixel-jitter"]
    r = _run(common + ["-o", str(out), "--denoise", str(I), "--denoise-color", str(sc)])
    assert r.returncode == 0, r.stderr
    assert _run(common + ["-o", str(raw)]).returncode == 0
    got = np.asarray(Image.open(out).convert("RGBA"))
    scene = R.YamlScene(open(AREA).read(), W, H, 1)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        frame = rend.render_lens(scene.camera, R.Lens(S, pixel_jitter=True), max_depth=5)["avg"]
        g = rend.render_aov(scene.camera)
        want = rend.denoise(frame, R.Denoise(I, sigma_color=sc), **{k: g[k] for k in PLANES})
    finally:
        rend.close()
    assert np.array_equal(np.asarray(Image.open(raw).convert("RGBA")), R.quantize(frame))
    assert got.shape == (H, W, 4) and np.array_equal(got, R.quantize(want))
    assert not np.array_equal(got, R.quantize(frame))  # the filter changed the picture


@pytest.mark.gpu
def test_ao_png_equals_the_quantised_denoise_of_the_unfiltered_plane(tmp_path):
    from PIL import Image
    import rray_amd as R

    W, H, K, radius, I = 40, 30, 4, 0.75, 3
    out, prefix = tmp_path / "c1.png", tmp_path / "c1"
    r = _run(["-W", str(W), "-H", str(H), "-s", SCENE, "-o", str(out), "--aov", str(prefix), "--ao-samples", str(K),
              "--ao-radius", str(radius), "--denoise", str(I)])
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c1.png", "c1_albedo.png", "c1_ao.png", "c1_normal.png"]
    got = np.asarray(Image.open(str(prefix) + "_ao.png").convert("RGBA"))
    scene = R.YamlScene(open(SCENE).read(), W, H, 1)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        plane = rend.render_ao(scene.camera, R.Ao(K, radius, 0))["ao"]
        g = rend.render_aov(scene.camera)
        want = rend.denoise(plane, R.Denoise(I), **{k: g[k] for k in PLANES})
        colour = rend.render(scene.camera, max_depth=5)["avg"]
    finally:
        rend.close()
    assert got.shape == (H, W, 4) and np.array_equal(got, R.quantize(np.repeat(want[:, :, None], 3, axis=2)))
    assert not np.array_equal(got, R.quantize(np.repeat(plane[:, :, None], 3, axis=2)))
    # the other files are the ones the run writes without --denoise
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_normal.png").convert("RGBA")), R.quantize(g["normal"] * 0.5 + 0.5))
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_albedo.png").convert("RGBA")), R.quantize(g["albedo"]))
    assert np.array_equal(np.asarray(Image.open(out).convert("RGBA")), R.quantize(colour))
