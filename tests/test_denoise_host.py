"""The denoiser's definition on the host (rray.h RR_HAS_DENOISE): the symbols and the struct, the
refusals that need no device, rr_denoise_reference (the very function denoise_level_kernel calls,
rray_amd/csrc/denoise_tap.hpp) against its numpy mirror rray_amd.denoise_filter bit for bit over the frames of
tests/denoise_cases.py, the filter's properties, a usefulness check on a synthetic frame, and the hand-derived native
check.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_cases as D  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLANES = ("depth", "normal", "object", "albedo")
NAMES = ("rr_denoise_reference", "rr_denoise", "rr_denoise_device")
# Per level the two sums of at most 25 non-negative products and the one division err by at most 51 * 2^-53 relative,
# over at most RR_MAX_DENOISE_ITERATIONS = 8 levels: 408 * 2^-53 < 1e-13.
BOUND = 1e-13
assert 8 * 51 * 2.0**-53 < BOUND


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


def test_abi_symbols_and_struct(R):
    L, E = R.lib(), R._lib
    hdr = open(E.HEADER).read()
    for name in NAMES:
        assert hasattr(L, name) and name in E.EXPORTS and f"int {name}(" in hdr, name
    assert "#define RR_HAS_DENOISE 1" in hdr and "#define RR_ABI_VERSION 11" in hdr and L.rr_abi_version() == 11
    assert f"#define RR_MAX_DENOISE_ITERATIONS {E.RR_MAX_DENOISE_ITERATIONS}" in hdr and E.RR_MAX_DENOISE_ITERATIONS == 8
    assert f"#define RR_DN_OBJECT {E.RR_DN_OBJECT}" in hdr and E.RR_DN_OBJECT == 1
    T = E.DenoiseDesc
    assert C.sizeof(T) == 40 and (T.iterations.offset, T.flags.offset, T.sigma_color.offset, T.sigma_normal.offset,
                                  T.sigma_depth.offset, T.sigma_albedo.offset) == (0, 4, 8, 16, 24, 32)
    d = R.Denoise(3).desc()
    assert (d.iterations, d.flags, d.sigma_color, d.sigma_normal, d.sigma_depth, d.sigma_albedo) == (3, 0, 0.0, 0.25, 0.05, 0.1)
    assert R.Denoise(1, sigma_color=0.5, object=True).desc().flags == 1
    for name in ("denoise", "denoise_device"):
        assert callable(getattr(R.Renderer, name))
    for name in ("Denoise", "denoise_reference", "denoise_filter"):
        assert name in R.__all__ and hasattr(R, name)


def test_sizeof_rr_denoise_desc_is_40_for_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not available")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rray/rray.h"\n'
                   '_Static_assert(sizeof(rr_denoise_desc) == 40, "rr_denoise_desc");\n'
                   '_Static_assert(offsetof(rr_denoise_desc, flags) == 4 && offsetof(rr_denoise_desc, sigma_color) == 8 &&\n'
                   '               offsetof(rr_denoise_desc, sigma_albedo) == 32, "rr_denoise_desc layout");\n'
                   '#if !defined(RR_HAS_DENOISE) || RR_MAX_DENOISE_ITERATIONS != 8 || RR_DN_OBJECT != 1 || RR_ABI_VERSION != 11\n'
                   '#error\n#endif\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-comment", "-I" + os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_refusals_that_need_no_device(R):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    f = D.frame(W, H)
    out = np.full((H, W, 3), -12345.5)
    hp = {k: f[k].ctypes.data_as(E._I if k == "object" else E._D) for k in PLANES + ("img3",)}
    po = out.ctypes.data_as(E._D)
    fake = C.c_void_p(4096)  # never dereferenced: the arguments are refused first

    def err():
        return L.rr_last_error().decode()

    def desc(**kw):
        fields = dict(iterations=2, flags=1, sigma_color=0.5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
        fields.update(kw)
        return C.byref(E.DenoiseDesc(*fields.values()))

    def ref(d=None, w=W, h=H, c=3, skip=(), src=hp["img3"], dst=po, nodesc=False):
        d = None if nodesc else (d or desc())
        return L.rr_denoise_reference(d, w, h, c, src, *[None if k in skip else hp[k] for k in PLANES], dst)

    assert ref(nodesc=True) == ARG and ref(src=None) == ARG and ref(dst=None) == ARG
    for c in (0, 2, 4, -3):
        assert ref(c=c) == ARG and "channels" in err()
    for w, h in ((0, 5), (7, 0), (-1, 5), (7, -1)):
        assert ref(w=w, h=h) == ARG
    bad = (dict(iterations=0), dict(iterations=-1), dict(iterations=9), dict(flags=2), dict(flags=3), dict(flags=-1),
           dict(sigma_color=-1.0), dict(sigma_color=math.nan), dict(sigma_color=math.inf), dict(sigma_normal=-1e-300),
           dict(sigma_normal=math.nan), dict(sigma_depth=math.inf), dict(sigma_depth=-math.inf), dict(sigma_albedo=-0.5),
           dict(sigma_albedo=math.nan))
    for kw in bad:
        assert ref(desc(**kw)) == ARG, kw
        # the device entries refuse the same before they touch the context or a buffer
        assert L.rr_denoise(None, desc(**kw), W, H, 3, hp["img3"], *[hp[k] for k in PLANES], po) == ARG, kw
        assert L.rr_denoise_device(None, desc(**kw), W, H, 3, fake, fake, fake, fake, fake, fake, None) == ARG, kw
    assert ref(desc(iterations=9)) == ARG and "iterations" in err()
    assert ref(desc(flags=2)) == ARG and "flag" in err()
    assert ref(desc(sigma_depth=math.nan)) == ARG and "sigma" in err()
    # a null context
    assert L.rr_denoise(None, desc(), W, H, 3, hp["img3"], *[hp[k] for k in PLANES], po) == ARG
    assert L.rr_denoise_device(None, desc(), W, H, 3, fake, fake, fake, fake, fake, C.c_void_p(1 << 20), None) == ARG
    # a term that is on needs its plane; with the term off the plane may go
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert ref(skip=(k,)) == ARG and "plane" in err(), k
    assert (out == -12345.5).all()
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert ref(desc(**off), skip=(k,)) == 0, k
    out[:] = -12345.5
    # out overlapping an input: the image itself, its last double, the middle of a plane
    assert ref(dst=hp["img3"]) == ARG and "overlap" in err()
    last = C.cast(C.c_void_p(f["img3"].ctypes.data + f["img3"].nbytes - 8), E._D)
    assert ref(dst=last) == ARG and "overlap" in err()
    for k in PLANES:
        mid = C.cast(C.c_void_p(f[k].ctypes.data + 8), E._D)
        assert ref(dst=mid) == ARG and "overlap" in err(), k
    # W * H >= 2^31
    assert ref(w=2**16, h=2**15) == LIM and "2^31" in err()
    assert ref(w=2**31, h=1) == LIM and ref(w=1, h=2**31) == LIM and ref(w=2**40, h=2**40) == LIM
    assert (out == -12345.5).all()
    # the boundary values serve
    assert ref(desc(iterations=8, sigma_color=5e-324, sigma_normal=1e300)) == 0 and np.isfinite(out).all()


@pytest.mark.parametrize("W,H", D.FRAMES, ids=[f"{w}x{h}" for w, h in D.FRAMES])
def test_reference_equals_the_numpy_mirror(R, W, H):
    n = 0
    for (w, h, Cn, I, name) in D.cases():
        if (w, h) != (W, H):
            continue
        img, dn, planes = D.arguments(R, W, H, Cn, I, name)
        got = R.denoise_reference(img, dn, **planes)
        want = D.expected(W, H, Cn, I, name)
        assert got.shape == img.shape and D.same_bits(got, want), (W, H, Cn, I, name)
        n += 1
    assert n == len(D.CHANNELS) * len(D.ITERATIONS) * len(D.COMBOS) == 48


def test_the_cases_are_not_vacuous(R):
    """On the largest frame every term cuts or weakens taps (its result differs from the plain filter's), the levels
    differ from one another, and the frame holds each edge case the definition names."""
    W, H = 70, 37
    f = D.frame(W, H)
    assert (f["depth"] == 0.0).sum() == 1 and (np.abs(f["normal"]).sum(axis=2) == 0.0).sum() == 1
    assert np.isinf(f["depth"]).sum() >= 4 * W and np.isnan(f["depth"]).sum() == 1
    assert ((f["object"] < 0) & np.isfinite(f["depth"])).any() and ((f["object"] >= 0) & np.isinf(f["depth"])).any()
    assert len(np.unique(f["object"][f["object"] >= 0])) == 4
    assert (f["depth"].astype(np.float32).astype(np.float64) != f["depth"])[np.isfinite(f["depth"])].mean() > 0.9
    for Cn in D.CHANNELS:
        plain = D.expected(W, H, Cn, 2, "none")
        for name in D.COMBOS:
            if name not in ("none", "colour"):  # colour passes no planes, so its void pixels differ as well
                assert not D.same_bits(D.expected(W, H, Cn, 2, name), plain), name
        assert not D.same_bits(D.expected(W, H, Cn, 1, "all"), D.expected(W, H, Cn, 2, "all"))
        assert not D.same_bits(D.expected(W, H, Cn, 2, "all"), D.expected(W, H, Cn, 6, "all"))
        assert not D.same_bits(D.expected(W, H, Cn, 2, "all"), D.expected(W, H, Cn, 2, "all_no_object"))


def test_a_nan_colour_stays_under_the_colour_term_and_spreads_without_it(R):
    f = D.frame(13, 5)
    for key in ("img1", "img3"):
        img = f[key].copy()
        img[2, 6] = math.nan  # one NaN colour (every channel of the pixel at C = 3)
        at = np.isnan(img)
        stays = R.Denoise(2, sigma_color=0.5, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
        spreads = R.Denoise(2, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
        a, b = R.denoise_reference(img, stays), R.denoise_reference(img, spreads)
        assert D.same_bits(a, R.denoise_filter(img, stays)) and D.same_bits(b, R.denoise_filter(img, spreads))
        assert np.array_equal(np.isnan(a), at)  # where it was, and nowhere else
        # without the term every pixel with a tap on it takes it in: level 0 reaches 2 pixels, level 1 another 4
        yy, xx = np.mgrid[0:5, 0:13]
        reach = (np.abs(yy - 2) <= 6) & (np.abs(xx - 6) <= 6)
        assert np.array_equal(np.isnan(b).reshape(5, 13, -1).all(axis=2), reach)
    # one NaN channel at C = 3 makes dc NaN all the same: the pixel keeps its NaN channel and nobody else gets one
    img = f["img3"].copy()
    img[1, 3, 1] = math.nan
    a = R.denoise_reference(img, stays)
    assert D.same_bits(a, R.denoise_filter(img, stays)) and np.array_equal(np.isnan(a), np.isnan(img))


def test_properties(R):
    W, H = 70, 37
    f = D.frame(W, H)
    void = ~(f["depth"].astype(np.float32) < np.inf) | (f["object"] < 0)
    planes = {k: f[k] for k in PLANES}
    for Cn in D.CHANNELS:
        img = f["img1" if Cn == 1 else "img3"]
        for I in (1, 2, 6, 8):
            dn = R.Denoise(I, sigma_color=0.5, object=True)
            # a constant image comes back
            const = np.full(img.shape, 0.7310585786300049)
            out = R.denoise_reference(const, dn, **planes)
            assert np.abs(out - const).max() <= BOUND * 0.7310585786300049, (Cn, I)
            # every output lies between the minimum and maximum of its inputs
            out = R.denoise_reference(img, dn, **planes)
            lo, hi, scale = img.min(), img.max(), np.abs(img).max()
            assert out.min() >= lo - BOUND * scale and out.max() <= hi + BOUND * scale, (Cn, I)
            # void pixels come back bit for bit, and the others do change
            assert D.same_bits(out[void], img[void]) and void.sum() > 4 * W
            assert (out[~void] != img[~void]).mean() > 0.9
    # two halves that differ in object id do not mix across the seam with RR_DN_OBJECT, and do without it
    obj = np.zeros((H, W), np.int32)
    obj[:, W // 2:] = 5
    img = np.where(obj == 0, 1.0, 3.0) + 0.0 * f["img1"]
    for I in (1, 3, 6):
        out = R.denoise_reference(img, R.Denoise(I, 0.0, 0.0, 0.0, 0.0, object=True), object=obj)
        assert np.abs(out - img).max() <= BOUND * 3.0, I
        mixed = R.denoise_reference(img, R.Denoise(I, 0.0, 0.0, 0.0, 0.0), object=obj)
        assert mixed[:, W // 2 - 1].min() > 1.1 and mixed[:, W // 2].max() < 2.9, I
    # a noisy image on the two halves: each half's outputs stay inside its own half's range
    noisy = np.where(obj == 0, 1.0, 3.0) + 0.5 * (f["img1"] - 0.5)
    out = R.denoise_reference(noisy, R.Denoise(6, 0.0, 0.0, 0.0, 0.0, object=True), object=obj)
    for half in (obj == 0, obj == 5):
        assert out[half].min() >= noisy[half].min() - BOUND * 4 and out[half].max() <= noisy[half].max() + BOUND * 4


def synthetic(W=56, H=40, K=4, seed=20261021):
    """A floor whose depth falls with the row, a disc with sphere normals in front of it, four void rows on top, and a
    smooth true value; binomial K = 4 noise on it (an occlusion plane's noise)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 40.0 / (1.0 + y)  # the floor: far at the top, near at the bottom
    normal = np.zeros((H, W, 3))
    normal[..., 1] = 1.0
    obj = np.zeros((H, W), np.int32)
    cx, cy, rad = 0.55 * W, 0.55 * H, 0.28 * H
    dx, dy = (x - cx) / rad, (y - cy) / rad
    disc = dx * dx + dy * dy < 1.0
    nz = np.sqrt(np.where(disc, 1.0 - (dx * dx + dy * dy), 0.0))
    normal[disc] = np.stack([dx, -dy, nz], axis=2)[disc]
    depth[disc] = (8.0 - 2.0 * nz)[disc]
    obj[disc] = 1
    truth = np.where(disc, 0.35 + 0.5 * nz, 0.9 - 0.4 * np.exp(-((x - cx) ** 2 + (y - cy - rad) ** 2) / (0.5 * rad) ** 2))
    truth = np.clip(truth, 0.0, 1.0)
    depth[:4], obj[:4], truth[:4] = np.inf, -1, 1.0
    noisy = rng.binomial(K, truth) / float(K)
    noisy[:4] = 1.0
    albedo = np.where(disc[..., None], [0.8, 0.3, 0.3], [0.6, 0.6, 0.6])
    return dict(truth=truth, noisy=noisy, depth=depth, normal=normal, object=obj, albedo=albedo, live=obj >= 0)


def test_the_filter_brings_a_noisy_plane_closer_to_the_truth(R):
    """The mean squared error against the true value over non-void pixels is lower after filtering than before.  The
    ratios this test measures are recorded in DESIGN.md §3.22."""
    s = synthetic()
    live = s["live"]
    before = ((s["noisy"] - s["truth"])[live] ** 2).mean()
    assert before > 0.01
    for sc in (0.0, 0.5):
        for I in (1, 3, 5):
            dn = R.Denoise(I, sigma_color=sc, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.0)
            out = R.denoise_reference(s["noisy"], dn, depth=s["depth"], normal=s["normal"], object=s["object"])
            assert D.same_bits(out, R.denoise_filter(s["noisy"], dn, depth=s["depth"], normal=s["normal"], object=s["object"]))
            ratio = ((out - s["truth"])[live] ** 2).mean() / before
            print(f"synthetic 56x40 K=4, sigma_color {sc}, iterations {I}: mse ratio {ratio:.4f}")
            assert ratio < 1.0, (sc, I, ratio)
            assert D.same_bits(out[~live], s["noisy"][~live])


def test_native_check(tmp_path):
    """tests/native/denoise_check.cpp: denoise_tap.hpp under g++ on frames whose results are derived by hand."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "denoise_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-comment",
                    "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "rray_amd", "csrc"),
                    os.path.join(HERE, "native", "denoise_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "0 failures", r.stdout
    ok = {ln.split()[1] for ln in lines if ln.startswith("ok ")}
    assert len(ok) == len(lines) - 1 >= 22 and {"row5_level1", "void_depth", "depth_zero", "normal_zero", "nan_stays",
                                                 "nan_spreads", "guide_rounding", "object_seam"} <= ok
