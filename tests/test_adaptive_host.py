"""CPU-side tests of adaptive anti-aliasing (rr_render_adaptive, additive to ABI 11): exports, the header's
RR_HAS_ADAPTIVE, argument refusals that need no device, the numpy criterion rray_amd.adaptive_mask on the committed
oracle frames, the documents and the CLI usage text.  The frames themselves are checked on the GPU
(tests/test_gpu_adaptive.py)."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("rr_render_adaptive", "rr_render_adaptive_device")


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


@pytest.fixture(scope="module")
def frames():
    files = sorted(glob.glob(os.path.join(GOLDEN, "oracle_*.npy")))
    assert len(files) >= 5
    out = {os.path.basename(f): np.load(f) for f in files}
    assert all(a.ndim == 3 and a.shape[2] == 3 for a in out.values())
    return out


def test_symbols_are_exported_and_listed(R):
    L = R.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in R._lib.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "rray", "rray.h")).read()
    assert re.search(r"^#define RR_HAS_ADAPTIVE 1\b", hdr, re.M)
    assert L.rr_abi_version() == 11  # additive: the version does not move
    for n in ("render_adaptive", "render_adaptive_device"):
        assert callable(getattr(R.Renderer, n))
    assert callable(R.adaptive_mask) and "adaptive_mask" in R.__all__


def test_bad_arguments_are_refused_without_a_device(R):
    L, E = R.lib(), R._lib.RR_E_ARG
    cam = R.camera(16, 16, 1.0)
    ok = R._lib.RenderOpts(2, 5, 0, 0, 0, 1, 8, 0, 0, 0)
    avg = np.zeros((8, 8, 3))
    p = avg.ctypes.data_as(R._lib._D)

    def host(c, o, thr, out):
        return L.rr_render_adaptive(None, c, o, thr, out, None, None, None)

    def dev(c, o, thr, out):
        return L.rr_render_adaptive_device(None, c, o, thr, out, None, None, None)

    for f, out in ((host, p), (dev, C.c_void_p(avg.ctypes.data))):
        assert f(C.byref(cam), C.byref(ok), 0.25, out) == E  # a null context
        assert "null context" in L.rr_last_error().decode()
        assert f(None, C.byref(ok), 0.25, out) == E
        assert f(C.byref(cam), None, 0.25, out) == E
        assert f(C.byref(cam), C.byref(ok), 0.25, None) == E
        assert "null" in L.rr_last_error().decode()
        assert f(C.byref(cam), C.byref(ok), math.nan, out) == E
        assert "NaN" in L.rr_last_error().decode()
        for bad in (R._lib.RenderOpts(2, 5, 0, 0, 1, 2, 8, 0, 0, 0), R._lib.RenderOpts(2, 5, 0, 0, 0, 2, 8, 0, 0, 0),
                    R._lib.RenderOpts(2, 5, 0, 0, 0, 1, 8, 0, 0, 4), R._lib.RenderOpts(2, 5, 0, 0, 0, 1, 8, 0, 2, 4)):
            assert f(C.byref(cam), C.byref(bad), 0.25, out) == E
            assert "part 0 of 1, no band" in L.rr_last_error().decode()
        for flag in (R._lib.RR_OUT_CANVAS, R._lib.RR_OUT_AVG, R._lib.RR_OUT_AVG_F32, R._lib.RR_PART_INTERLEAVE):
            assert f(C.byref(cam), C.byref(R._lib.RenderOpts(2, 5, 0, 0, 0, 1, 8, flag, 0, 0)), 0.25, out) == E
            assert "flag" in L.rr_last_error().decode()


def brute_mask(f, thr):
    """rule 2, pixel by pixel"""
    H, W = f.shape[:2]
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            for qy in range(max(0, y - 1), min(H, y + 2)):
                for qx in range(max(0, x - 1), min(W, x + 2)):
                    d = np.abs(f[y, x] - f[qy, qx])
                    m = math.nan if np.isnan(d).any() else d.max()
                    if not m <= thr:
                        out[y, x] = True
    return out


def test_mask_extremes_on_the_golden_frames(R, frames):
    for name, f in frames.items():
        assert R.adaptive_mask(f, -1.0).all(), name
        assert not R.adaptive_mask(f, math.inf).any(), name
        m = R.adaptive_mask(f, 0.25)
        assert m.dtype == bool and m.shape == f.shape[:2]
        assert np.array_equal(m, brute_mask(f, 0.25)), name
        assert 0 < m.sum() < m.size, name  # these scenes have both flat regions and edges
        # monotone in the threshold
        assert not (R.adaptive_mask(f, 0.5) & ~m).any(), name


def test_a_nan_pixel_flags_its_3x3_block(R, frames):
    f = frames["oracle_c2_s1024_48x27_aa1.npy"].copy()
    H, W = f.shape[:2]
    for y, x in ((10, 20), (0, 0), (H - 1, W - 1), (0, 7)):
        g = f.copy()
        g[y, x, 1] = math.nan
        want = np.zeros((H, W), bool)
        want[max(0, y - 1):y + 2, max(0, x - 1):x + 2] = True
        assert np.array_equal(R.adaptive_mask(g, math.inf), want), (y, x)
        assert np.array_equal(R.adaptive_mask(g, 0.25), brute_mask(g, 0.25)), (y, x)
    g = f.copy()
    g[5, 5] = [math.inf, 0.0, 0.0]  # inf - inf is NaN: the pixel itself refines, and so do its neighbours (inf > thr)
    assert R.adaptive_mask(g, 1e300)[4:7, 4:7].all()
    with pytest.raises(ValueError):
        R.adaptive_mask(f, math.nan)
    with pytest.raises(ValueError):
        R.adaptive_mask(f[..., :2], 0.25)


def test_the_mask_is_symmetric_across_an_edge(R):
    f = np.zeros((6, 8, 3))
    f[:, 4:] = [0.0, 0.5, 0.0]  # a vertical edge between columns 3 and 4
    m = R.adaptive_mask(f, 0.25)
    want = np.zeros((6, 8), bool)
    want[:, 3:5] = True
    assert np.array_equal(m, want)
    assert np.array_equal(R.adaptive_mask(f[:, ::-1], 0.25), m[:, ::-1])
    assert np.array_equal(R.adaptive_mask(f.transpose(1, 0, 2), 0.25), m.T)
    assert not R.adaptive_mask(f, 0.5).any()  # the difference equals the threshold: not refined (<=)
    assert R.adaptive_mask(f, np.nextafter(0.5, 0.0))[:, 3:5].all()


def test_degenerate_frames(R):
    one = np.full((1, 1, 3), 0.3)
    assert R.adaptive_mask(one, 0.0).tolist() == [[False]] and R.adaptive_mask(one, -1.0).tolist() == [[True]]
    row = np.zeros((1, 7, 3))
    row[0, 3] = 1.0
    assert R.adaptive_mask(row, 0.25)[0].tolist() == [False, False, True, True, True, False, False]
    col = row.transpose(1, 0, 2)
    assert R.adaptive_mask(col, 0.25)[:, 0].tolist() == [False, False, True, True, True, False, False]
    for f in (one, row, col):
        assert np.array_equal(R.adaptive_mask(f, 0.25), brute_mask(f, 0.25))


def test_documents_name_the_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert re.search(rf"\bfn {n}\s*\(", integ), n
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in NAMES:
        assert n in readme, n
        assert n in design, n
    assert "render_adaptive" in readme and "--adaptive" in readme
    assert re.search(r"^### 3\.15 ", design, re.M)


def test_cli_usage_lists_adaptive(R):
    cli = os.path.join(ROOT, "rray_amd", "bin", "rray")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--adaptive <THRESHOLD>" in r.stderr
    r = subprocess.run([cli, "-s", "x.yaml", "--adaptive", "abc"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--adaptive needs a number" in r.stderr
    r = subprocess.run([cli, "-s", "x.yaml", "--adaptive"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
