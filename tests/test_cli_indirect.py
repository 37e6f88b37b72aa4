"""`rray --indirect K [--indirect-depth D] [--indirect-seed N]`: one bounce of indirect light from the command line
(rr_render_indirect).  The written image is the colour frame composed with the bounce on the host
(rray_amd.indirect_compose); --aov PREFIX adds PREFIX_indirect.png; --denoise I filters the indirect plane with the aa 1
first-hit planes before composing.  Refused (usage error, exit 2) with -a other than 1, --adaptive and --samples.  The
argument handling never reaches the GPU; the rendering tests run the binary end to end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "rray_amd", "bin", "rray")
SCENE = os.path.join(ROOT, "scenes", "c1_readme.yaml")
PLANES = ("depth", "normal", "object", "albedo")


def _run(args, cwd=None, timeout=120):
    if not os.path.exists(CLI):
        pytest.fail("rray_amd/bin/rray is not built (run __graft_entry__.build())")
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def test_indirect_options_are_parsed(tmp_path):
    r = _run(["--help"])
    assert r.returncode == 0
    for flag in ("--indirect <K>", "--indirect-depth <D>", "--indirect-seed <N>"):
        assert flag in r.stderr, flag
    missing = str(tmp_path / "nope.yaml")
    # accepted, in any order: the run gets as far as the missing scene file (exit 1), not a usage error
    for flags in (["--indirect", "4"], ["--indirect-depth", "0", "--indirect", "1024", "--indirect-seed", "7"],
                  ["--indirect", "1", "--indirect-depth", "8", "-a", "1"],
                  ["--aov", str(tmp_path / "p"), "--indirect", "16", "--denoise", "3", "--denoise-color", "0.5"]):
        r = _run(["-s", missing, "-o", str(tmp_path / "o.png")] + flags)
        assert r.returncode == 1 and "File does not exist" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())  # nothing written
    # values
    for flags, text in ((["--indirect"], "missing value"), (["--indirect", "0"], "1 to 1024"),
                        (["--indirect", "1025"], "1 to 1024"), (["--indirect", "x"], "1 to 1024"),
                        (["--indirect", "-4"], "1 to 1024"), (["--indirect", "4", "--indirect-depth"], "missing value"),
                        (["--indirect", "4", "--indirect-depth", "9"], "0 to 8"),
                        (["--indirect", "4", "--indirect-depth", "-1"], "0 to 8"),
                        (["--indirect", "4", "--indirect-seed", "x"], "needs a number"),
                        (["--indirect", "4", "--indirect-seed", "-1"], "needs a number")):
        r = _run(["-s", "x.yaml"] + flags)
        assert r.returncode == 2 and text in r.stderr, (flags, r.stderr)


@pytest.mark.parametrize("flags,text", [
    (["--indirect", "4", "-a", "2"], "-a other than 1"),
    (["--indirect", "4", "--adaptive", "0.1"], "--adaptive"),
    (["--indirect", "4", "--samples", "2"], "--samples"),
    (["--indirect", "4", "--pixel-jitter"], "--samples"),
    (["--indirect-depth", "2"], "only with --indirect"),
    (["--indirect-seed", "2"], "only with --indirect"),
    (["--indirect", "4", "--denoise", "3", "-a", "3"], "-a other than 1"),
], ids=["aa2", "adaptive", "samples", "lens", "depth_alone", "seed_alone", "denoise_aa3"])
def test_refusals_are_usage_errors(tmp_path, flags, text):
    r = _run(["-s", SCENE, "-o", str(tmp_path / "o.png")] + flags, cwd=str(tmp_path))
    assert r.returncode == 2 and text in r.stderr and "Usage:" in r.stderr, (flags, r.returncode, r.stderr)
    assert not list(tmp_path.iterdir())


def _library_planes(W, H, K, depth, seed):
    import rray_amd as R

    scene = R.YamlScene(open(SCENE).read(), W, H, 1)
    rend = R.Renderer(0)
    try:
        rend.upload(scene)
        colour = rend.render(scene.camera, max_depth=5)["avg"]
        plane = rend.render_indirect(scene.camera, R.Indirect(K, depth, seed))["indirect"]
        g = rend.render_aov(scene.camera)
        return R, rend, scene, colour, plane, g
    except Exception:
        rend.close()
        raise


@pytest.mark.gpu
def test_pngs_equal_the_quantised_composition_of_the_librarys_planes(tmp_path):
    from PIL import Image

    W, H, K = 40, 30, 8
    out, prefix = tmp_path / "c1.png", tmp_path / "c1"
    r = _run(["-W", str(W), "-H", str(H), "-s", SCENE, "-o", str(out), "--indirect", str(K), "--indirect-depth", "2",
              "--indirect-seed", "11", "--aov", str(prefix)])
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c1.png", "c1_albedo.png", "c1_indirect.png", "c1_normal.png"]
    R, rend, scene, colour, plane, g = _library_planes(W, H, K, 2, 11)
    rend.close()
    want = R.indirect_compose(colour, plane, g["albedo"], g["object"], R.object_diffuse(scene))
    got = np.asarray(Image.open(out).convert("RGBA"))
    assert got.shape == (H, W, 4) and np.array_equal(got, R.quantize(want))
    assert not np.array_equal(got, R.quantize(colour))  # the bounce changed the picture
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_indirect.png").convert("RGBA")), R.quantize(plane))
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_albedo.png").convert("RGBA")), R.quantize(g["albedo"]))
    # the defaults: depth 1, seed 0; without --aov only the image
    plain = tmp_path / "plain"
    plain.mkdir()
    r = _run(["-W", str(W), "-H", str(H), "-s", SCENE, "-o", "d.png", "--indirect", str(K)], cwd=str(plain))
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in plain.iterdir()) == ["d.png"]
    R, rend, scene, colour, plane, g = _library_planes(W, H, K, 1, 0)
    rend.close()
    want = R.indirect_compose(colour, plane, g["albedo"], g["object"], R.object_diffuse(scene))
    assert np.array_equal(np.asarray(Image.open(plain / "d.png").convert("RGBA")), R.quantize(want))


@pytest.mark.gpu
def test_denoise_filters_the_indirect_plane_before_composing(tmp_path):
    from PIL import Image

    W, H, K, I, sc = 40, 30, 4, 3, 0.5
    out, prefix = tmp_path / "c1.png", tmp_path / "c1"
    r = _run(["-W", str(W), "-H", str(H), "-s", SCENE, "-o", str(out), "--indirect", str(K), "--aov", str(prefix),
              "--denoise", str(I), "--denoise-color", str(sc)])
    assert r.returncode == 0, r.stderr
    R, rend, scene, colour, plane, g = _library_planes(W, H, K, 1, 0)
    try:
        clean = rend.denoise(plane, R.Denoise(I, sigma_color=sc), **{k: g[k] for k in PLANES})
    finally:
        rend.close()
    kd = R.object_diffuse(scene)
    want = R.indirect_compose(colour, clean, g["albedo"], g["object"], kd)
    got = np.asarray(Image.open(out).convert("RGBA"))
    assert np.array_equal(got, R.quantize(want))
    assert np.array_equal(np.asarray(Image.open(str(prefix) + "_indirect.png").convert("RGBA")), R.quantize(clean))
    assert not np.array_equal(R.quantize(clean), R.quantize(plane))  # the filter changed the plane
