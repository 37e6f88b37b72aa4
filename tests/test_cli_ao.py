"""`rray --aov PREFIX --ao-samples K --ao-radius R`: the ambient-occlusion plane from the command line (rr_render_ao,
DESIGN.md §3.21).  The two flags are valid only together and only with --aov; anything else is a usage error, exit 2.
They add PREFIX_ao.png, grey, per canvas sample like the other planes, through the colour image's quantisation.  The
argument handling never reaches the GPU; the rendering test runs the binary end to end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rray_amd", "bin", "rray")
SCENE = os.path.join(ROOT, "scenes", "c1_readme.yaml")
ONLY = "only together and only with --aov"


def _run(args, cwd=None, timeout=120):
    if not os.path.exists(CLI):
        pytest.fail("rray_amd/bin/rray is not built (run __graft_entry__.build())")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_ao_options_are_parsed(tmp_path):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in ("--ao-samples <K>", "--ao-radius <R>"):
        assert flag in r.stderr, flag
    missing = str(tmp_path / "nope.yaml")
    # accepted with --aov, in any order: the run gets as far as the missing scene file (exit 1), not a usage error
    for flags in (["--aov", str(tmp_path / "p"), "--ao-samples", "16", "--ao-radius", "0.5"],
                  ["--ao-radius", "2", "--ao-samples", "1024", "--aov", str(tmp_path / "p"), "-a", "2"]):
        r = _run(["-s", missing, "-o", str(tmp_path / "o.png")] + flags)
        assert r.returncode == 1 and "File does not exist" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())  # nothing written
    # values
    for flags, text in ((["--ao-samples"], "missing value"), (["--ao-samples", "0"], "1 to 1024"),
                        (["--ao-samples", "1025"], "1 to 1024"), (["--ao-samples", "x"], "1 to 1024"),
                        (["--ao-radius"], "missing value"), (["--ao-radius", "0"], "> 0"), (["--ao-radius", "-1"], "> 0"),
                        (["--ao-radius", "nan"], "> 0"), (["--ao-radius", "inf"], "> 0")):
        r = _run(["-s", "x.yaml", "--aov", "p"] + flags)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)


@pytest.mark.parametrize("flags", [["--ao-samples", "16", "--ao-radius", "0.5"], ["--ao-samples", "16"],
                                   ["--ao-radius", "0.5"], ["--aov", "p", "--ao-samples", "16"],
                                   ["--ao-radius", "0.5", "--aov", "p"],
                                   ["--ao-samples", "16", "--ao-radius", "0.5", "--adaptive", "0.1"]],
                         ids=["no_aov", "samples_alone", "radius_alone", "aov_samples", "aov_radius", "adaptive_no_aov"])
def test_anything_but_both_with_aov_is_a_usage_error(tmp_path, flags):
    r = _run(["-s", SCENE, "-o", str(tmp_path / "o.png")] + flags, cwd=str(tmp_path))
    assert r.returncode == 2 and ONLY in r.stderr and "Usage:" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_ao_png_equals_the_quantised_library_plane(tmp_path):
    from PIL import Image
    import rray_amd as R

    W, H, aa, K, radius = 40, 30, 2, 16, 0.75
    out, prefix = tmp_path / "c1.png", tmp_path / "c1"
    r = _run(["-W", str(W), "-H", str(H), "-a", str(aa), "-s", SCENE, "-o", str(out), "--aov", str(prefix),
              "--ao-samples", str(K), "--ao-radius", str(radius)])
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c1.png", "c1_albedo.png", "c1_ao.png", "c1_normal.png"]
    got = np.asarray(Image.open(str(prefix) + "_ao.png").convert("RGBA"))
    assert got.shape == (H * aa, W * aa, 4)  # per canvas sample, never averaged
    scene = R.YamlScene(open(SCENE).read(), W, H, aa)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        plane = rend.render_ao(scene.camera, R.Ao(K, radius, 0), aa=aa)["ao"]
        ref = rend.render_aov(scene.camera, aa=aa, planes=("normal", "albedo"))
    finally:
        rend.close()
    assert np.array_equal(got, R.quantize(np.repeat(plane[:, :, None], 3, axis=2)))
    assert (got[..., 0] == got[..., 1]).all() and (got[..., 1] == got[..., 2]).all()  # grey
    assert len(np.unique(got[..., 0])) > 4 and got[..., 0].max() == 255  # a real plane: open parts and darker creases
    # the other planes are the ones --aov writes without the flags
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_normal.png").convert("RGBA")), R.quantize(ref["normal"] * 0.5 + 0.5))
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_albedo.png").convert("RGBA")), R.quantize(ref["albedo"]))
    # without the flags no occlusion plane appears
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run(["-W", str(W), "-H", str(H), "-a", str(aa), "-s", SCENE, "-o", "only.png", "--aov", "q"], cwd=str(plain))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in plain.iterdir()) == ["only.png", "q_albedo.png", "q_normal.png"]
