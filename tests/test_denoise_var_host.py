"""Variance-guided denoising's definition on the host (rray.h RR_HAS_DENOISE_VAR): the symbols and
the two structs, the refusals that need no device, rr_variance_reference and rr_denoise_var_reference (the very functions
the kernels call, rray_amd/csrc/denoise_var_tap.hpp) against their numpy mirrors rray_amd.variance_estimate and
rray_amd.denoise_var_filter bit for bit over the cases of tests/denoise_var_cases.py, the exact properties, the
usefulness check against the plain filter's sigma sweep, and the hand-derived native check.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import denoise_var_cases as V  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLANES = ("depth", "normal", "object", "albedo")
NAMES = ("rr_variance_reference", "rr_variance", "rr_variance_device", "rr_denoise_var_reference", "rr_denoise_var",
         "rr_denoise_var_device")
# DESIGN.md §3.22's bound for the same sums: per level two sums of at most 25 non-negative products and one division err
# by at most 51 * 2^-53 relative, over at most RR_MAX_DENOISE_ITERATIONS = 8 levels: 408 * 2^-53 < 1e-13.
BOUND = 1e-13
assert 8 * 51 * 2.0**-53 < BOUND


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


def test_abi_symbols_and_structs(R):
    L, E = R.lib(), R._lib
    hdr = open(E.HEADER).read()
    for name in NAMES:
        assert hasattr(L, name) and name in E.EXPORTS and f"int {name}(" in hdr, name
    assert "#define RR_HAS_DENOISE_VAR 1" in hdr and "#define RR_ABI_VERSION 11" in hdr and L.rr_abi_version() == 11
    T = E.VarianceDesc
    assert C.sizeof(T) == 32 and (T.flags.offset, T.min_history.offset, T.sigma_normal.offset, T.sigma_depth.offset,
                                  T.sigma_albedo.offset) == (0, 4, 8, 16, 24)
    T = E.DenoiseVarDesc
    assert C.sizeof(T) == 48 and (T.iterations.offset, T.flags.offset, T.sigma_color.offset, T.sigma_normal.offset,
                                  T.sigma_depth.offset, T.sigma_albedo.offset, T.epsilon.offset) == (0, 4, 8, 16, 24, 32, 40)
    d = R.Variance().desc()
    assert (d.flags, d.min_history, d.sigma_normal, d.sigma_depth, d.sigma_albedo) == (0, 4, 0.25, 0.05, 0.0)
    assert R.Variance(object=True).desc().flags == 1
    d = R.DenoiseVar(3).desc()
    assert (d.iterations, d.flags, d.sigma_color, d.sigma_normal, d.sigma_depth, d.sigma_albedo, d.epsilon) == \
        (3, 0, 4.0, 0.25, 0.05, 0.1, 1e-12)
    assert R.DenoiseVar(1, object=True).desc().flags == 1
    for name in ("variance", "variance_device", "denoise_var", "denoise_var_device"):
        assert callable(getattr(R.Renderer, name))
    for name in ("Variance", "variance_reference", "variance_estimate", "DenoiseVar", "denoise_var_reference",
                 "denoise_var_filter"):
        assert name in R.__all__ and hasattr(R, name)


def test_sizeof_the_descriptors_for_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not available")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rray/rray.h"\n'
                   '_Static_assert(sizeof(rr_variance_desc) == 32, "rr_variance_desc");\n'
                   '_Static_assert(offsetof(rr_variance_desc, min_history) == 4 && offsetof(rr_variance_desc, sigma_normal) == 8 &&\n'
                   '               offsetof(rr_variance_desc, sigma_albedo) == 24, "rr_variance_desc layout");\n'
                   '_Static_assert(sizeof(rr_denoise_var_desc) == 48, "rr_denoise_var_desc");\n'
                   '_Static_assert(offsetof(rr_denoise_var_desc, flags) == offsetof(rr_denoise_desc, flags) &&\n'
                   '               offsetof(rr_denoise_var_desc, sigma_color) == offsetof(rr_denoise_desc, sigma_color) &&\n'
                   '               offsetof(rr_denoise_var_desc, sigma_albedo) == offsetof(rr_denoise_desc, sigma_albedo) &&\n'
                   '               offsetof(rr_denoise_var_desc, epsilon) == 40, "rr_denoise_var_desc layout");\n'
                   '#if !defined(RR_HAS_DENOISE_VAR) || RR_ABI_VERSION != 11\n'
                   '#error\n#endif\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-comment", "-I" + os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_refusals_that_need_no_device(R):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    f = V.frame(W, H)
    keys = PLANES + ("img3", "m2_3", "count", "var")
    hp = {k: f[k].ctypes.data_as(E._I if k in ("object", "count") else E._D) for k in keys}
    var_out = np.full((H, W), -12345.5)
    out = np.full((H, W, 3), -12345.5)
    vout = np.full((H, W), -12345.5)
    pv, po, pvo = (a.ctypes.data_as(E._D) for a in (var_out, out, vout))
    fake = C.c_void_p(4096)  # never dereferenced: the arguments are refused first

    def err():
        return L.rr_last_error().decode()

    def mid(k):
        return C.cast(C.c_void_p(f[k].ctypes.data + 8), E._D)

    # ---- rr_variance ----
    def vdesc(**kw):
        fields = dict(flags=1, min_history=4, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
        fields.update(kw)
        return C.byref(E.VarianceDesc(*fields.values()))

    def vref(d=None, w=W, h=H, c=3, skip=(), src=hp["img3"], dst=pv, nodesc=False):
        d = None if nodesc else (d or vdesc())
        return L.rr_variance_reference(d, w, h, c, src, *[None if k in skip else hp[k] for k in ("m2_3", "count") + PLANES], dst)

    assert vref(nodesc=True) == ARG and vref(src=None) == ARG and vref(dst=None) == ARG
    for c in (0, 2, 4, -3):
        assert vref(c=c) == ARG and "channels" in err()
    for w, h in ((0, 5), (7, 0), (-1, 5), (7, -1)):
        assert vref(w=w, h=h) == ARG
    bad = (dict(flags=2), dict(flags=-1), dict(min_history=-1), dict(min_history=E.RR_MAX_TEMPORAL_HISTORY + 1),
           dict(sigma_normal=-1e-300), dict(sigma_normal=math.nan), dict(sigma_depth=math.inf), dict(sigma_albedo=-0.5))
    for kw in bad:
        assert vref(vdesc(**kw)) == ARG, kw
        # the device entries refuse the same before they touch the context or a buffer
        assert L.rr_variance(None, vdesc(**kw), W, H, 3, hp["img3"], hp["m2_3"], hp["count"], *[hp[k] for k in PLANES], pv) == ARG
        assert L.rr_variance_device(None, vdesc(**kw), W, H, 3, *[fake] * 8, None) == ARG
    assert vref(vdesc(min_history=-1)) == ARG and "min_history" in err()
    assert vref(vdesc(flags=2)) == ARG and "flag" in err()
    assert vref(vdesc(sigma_depth=math.nan)) == ARG and "sigma" in err()
    assert vref(skip=("m2_3",)) == ARG and "go together" in err() and vref(skip=("count",)) == ARG and "go together" in err()
    assert L.rr_variance(None, vdesc(), W, H, 3, hp["img3"], None, None, *[hp[k] for k in PLANES], pv) == ARG  # a null context
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert vref(skip=(k,)) == ARG and "plane" in err(), k
        assert (var_out == -12345.5).all()
        assert vref(vdesc(**off), skip=(k,)) == 0, k
        var_out[:] = -12345.5
    assert vref(dst=hp["img3"]) == ARG and "overlap" in err()
    for k in ("m2_3", "count") + PLANES:
        assert vref(dst=mid(k)) == ARG and "overlap" in err(), k
    assert vref(w=2**16, h=2**15) == LIM and "2^31" in err()
    assert vref(w=2**31, h=1) == LIM and vref(w=1, h=2**31) == LIM and vref(w=2**40, h=2**40) == LIM
    assert (var_out == -12345.5).all()
    assert vref(vdesc(min_history=0)) == 0 and vref(vdesc(min_history=E.RR_MAX_TEMPORAL_HISTORY)) == 0
    assert vref(skip=("m2_3", "count")) == 0 and np.isfinite(var_out).all()

    # ---- rr_denoise_var ----
    def desc(**kw):
        fields = dict(iterations=2, flags=1, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1,
                      epsilon=1e-12)
        fields.update(kw)
        return C.byref(E.DenoiseVarDesc(*fields.values()))

    def ref(d=None, w=W, h=H, c=3, skip=(), src=hp["img3"], var=hp["var"], dst=po, vdst=pvo, nodesc=False):
        d = None if nodesc else (d or desc())
        return L.rr_denoise_var_reference(d, w, h, c, src, var, *[None if k in skip else hp[k] for k in PLANES], dst, vdst)

    assert ref(nodesc=True) == ARG and ref(src=None) == ARG and ref(dst=None) == ARG
    assert ref(var=None) == ARG and "var" in err()
    for c in (0, 2, 4, -3):
        assert ref(c=c) == ARG and "channels" in err()
    for w, h in ((0, 5), (7, 0), (-1, 5), (7, -1)):
        assert ref(w=w, h=h) == ARG
    bad = (dict(iterations=0), dict(iterations=-1), dict(iterations=9), dict(flags=2), dict(flags=-1),
           dict(sigma_color=-1.0), dict(sigma_color=math.nan), dict(sigma_normal=math.inf), dict(sigma_depth=-math.inf),
           dict(sigma_albedo=math.nan), dict(epsilon=0.0), dict(epsilon=-1e-12), dict(epsilon=math.nan), dict(epsilon=math.inf))
    for kw in bad:
        assert ref(desc(**kw)) == ARG, kw
        assert L.rr_denoise_var(None, desc(**kw), W, H, 3, hp["img3"], hp["var"], *[hp[k] for k in PLANES], po, pvo) == ARG, kw
        assert L.rr_denoise_var_device(None, desc(**kw), W, H, 3, *[fake] * 8, None) == ARG, kw
    assert ref(desc(iterations=9)) == ARG and "iterations" in err() and "rr_denoise_var" in err()
    assert ref(desc(epsilon=0.0)) == ARG and "epsilon" in err()
    assert L.rr_denoise_var(None, desc(), W, H, 3, hp["img3"], hp["var"], *[hp[k] for k in PLANES], po, pvo) == ARG
    for k, off in (("depth", dict(sigma_depth=0.0)), ("normal", dict(sigma_normal=0.0)), ("object", dict(flags=0)),
                   ("albedo", dict(sigma_albedo=0.0))):
        assert ref(skip=(k,)) == ARG and "plane" in err(), k
        assert (out == -12345.5).all() and (vout == -12345.5).all()
        assert ref(desc(**off), skip=(k,)) == 0, k
        out[:], vout[:] = -12345.5, -12345.5
    # an output overlapping an input or the other output
    assert ref(dst=hp["img3"]) == ARG and "overlap" in err() and ref(dst=hp["var"]) == ARG and "overlap" in err()
    assert ref(vdst=hp["var"]) == ARG and "overlap" in err() and ref(vdst=mid("img3")) == ARG and "overlap" in err()
    for k in PLANES:
        assert ref(dst=mid(k)) == ARG and "overlap" in err() and ref(vdst=mid(k)) == ARG and "overlap" in err(), k
    assert ref(vdst=C.cast(C.c_void_p(out.ctypes.data + 16), E._D)) == ARG and "overlap" in err()
    assert ref(w=2**16, h=2**15) == LIM and "2^31" in err()
    assert ref(w=2**31, h=1) == LIM and ref(w=1, h=2**31) == LIM and ref(w=2**40, h=2**40) == LIM
    assert (out == -12345.5).all() and (vout == -12345.5).all()
    # var_out is optional, and the boundary values serve
    assert ref(vdst=None) == 0 and (vout == -12345.5).all()
    assert ref(desc(iterations=8, sigma_color=5e-324, epsilon=5e-324, sigma_normal=1e300)) == 0


@pytest.mark.parametrize("W,H", V.FRAMES, ids=[f"{w}x{h}" for w, h in V.FRAMES])
def test_references_equal_the_numpy_mirrors(R, W, H):
    n = 0
    for case in V.variance_cases():
        if case[:2] != (W, H):
            continue
        img, vr, args = V.variance_arguments(R, *case)
        got = R.variance_reference(img, vr, **args)
        assert got.shape == (H, W) and V.same_bits(got, V.variance_expected(*case)), case
        n += 1
    assert n == len(V.CHANNELS) * len(V.GUIDES) * len(V.HISTORIES) == 42
    n = 0
    for case in V.filter_cases():
        if case[:2] != (W, H):
            continue
        img, var, dv, planes = V.filter_arguments(R, *case)
        want, want_v = V.filter_expected(*case)
        got, got_v = R.denoise_var_reference(img, var, dv, return_var=True, **planes)
        assert got.shape == img.shape and V.same_bits(got, want) and V.same_bits(got_v, want_v), case
        assert V.same_bits(R.denoise_var_reference(img, var, dv, **planes), want), case  # var_out NULL
        n += 1
    assert n == len(V.CHANNELS) * len(V.ITERATIONS) * len(V.GUIDES) * len(V.COLOURS) == 84


def test_the_cases_are_not_vacuous(R):
    """On the largest frame both variance branches are taken within single waves, the guide terms change the spatial
    estimate, the colour term skips some taps and keeps others, and the planes hold the edge cases the definition names."""
    W, H = 70, 37
    f = V.frame(W, H)
    void = ~(f["depth"].astype(np.float32) < np.inf) | (f["object"] < 0)
    assert (f["depth"] == 0.0).sum() == 1 and np.isnan(f["img1"]).sum() == 1 and np.isnan(f["img3"]).sum() == 3
    assert (f["var"] == 0.0).sum() > 100 and np.isnan(f["var"]).sum() == 1 and np.isinf(f["var"]).sum() == 1
    assert ((f["var"] > 0.0) & (f["var"] < 2.3e-308)).sum() == 2
    for n in (0, V.MIN_HISTORY - 1, V.MIN_HISTORY, 1 << 20):
        assert (f["count"] == n).sum() > 100
    # every wave (two rows of 32 pixels of a tile) of the mixed history holds both branches
    temporal = f["count"] >= V.MIN_HISTORY
    for y0 in range(0, 36, 2):
        for x0 in (0, 32):
            wave = temporal[y0:y0 + 2, x0:x0 + 32]
            assert wave.any() and not wave.all(), (x0, y0)
    for Cn in V.CHANNELS:
        absent, mixed, zero = (V.variance_expected(W, H, Cn, "all", h) for h in V.HISTORIES)
        assert V.same_bits(mixed[~temporal], absent[~temporal]) and not (mixed[temporal & ~void] == absent[temporal & ~void]).all()
        assert V.same_bits(zero[temporal], mixed[temporal]) and not V.same_bits(zero, mixed)
        m2, img = f[f"m2_{Cn}"], f[f"img{Cn}"]
        exact = temporal & ~void & (m2 == img * img).reshape(H, W, -1).all(axis=2)
        assert exact.sum() > 50 and (mixed[exact] == 0.0).all()  # m2 == in * in gives V == 0.0 exactly
        assert (mixed[void] == 0.0).all() and void.sum() > 4 * W
        assert ((m2 < img * img) & (m2 != 0.0)).sum() > 20  # the clamp is taken
        plain = V.variance_expected(W, H, Cn, "none", "absent")
        for g in V.GUIDES:
            if g != "none":
                assert not V.same_bits(V.variance_expected(W, H, Cn, g, "absent"), plain), g
        # the colour term skips taps: every tap on the NaN colour (t is NaN), so it stays where it is, and spreads
        # without the term; inside the block of zero variance den is epsilon, every off-centre weight falls below
        # 1e-18 of the centre's and the pixel keeps its value to the two roundings of (9/64 F) / (9/64)
        # (but for pixels clipped to exactly 0.0 or equal to a neighbour, which the term rightly lets through).  It
        # keeps taps elsewhere: the pixels change, and differ from the plain filter's
        img, var, dv, planes = V.filter_arguments(R, W, H, Cn, 1, "none", "colour")
        on, off = V.filter_expected(W, H, Cn, 1, "none", "colour")[0], V.filter_expected(W, H, Cn, 1, "none", "plain")[0]
        img3, on3, off3 = (a.reshape(H, W, -1) for a in (img, on, off))
        assert np.array_equal(np.isnan(on3), np.isnan(img3)) and np.isnan(off3).all(axis=2).sum() == 20  # 5 x 5 less a void row
        kept = ~void & ~np.isnan(off3).any(axis=2)
        same = (np.abs(on3 - img3) <= 2.0**-52 * np.abs(img3)).all(axis=2)
        block = np.zeros((H, W), bool)
        block[9:15, 41:59] = True
        assert (var[8:16, 40:60] == 0.0).all() and same[block].mean() > 0.8 and (~same & kept).sum() > 1000
        assert ((on3 != off3).any(axis=2) & kept).sum() > 1000
        for I in (1, 2):
            a, b = V.filter_expected(W, H, Cn, I, "all", "colour"), V.filter_expected(W, H, Cn, I + (1 if I == 1 else 4), "all", "colour")
            assert not V.same_bits(a[0], b[0]) and not V.same_bits(a[1], b[1])
        assert not V.same_bits(V.filter_expected(W, H, Cn, 2, "all", "colour")[0], V.filter_expected(W, H, Cn, 2, "all_no_object", "colour")[0])


def test_exact_properties(R):
    W, H = 70, 37
    f = V.frame(W, H)
    void = ~(f["depth"].astype(np.float32) < np.inf) | (f["object"] < 0)
    planes = {k: f[k] for k in PLANES}
    rng = np.random.default_rng(5)
    for Cn in V.CHANNELS:
        img = f[f"img{Cn}"]
        for I in (1, 2, 6, 8):
            dv = R.DenoiseVar(I, object=True)
            # void pixels keep F and V bit for bit
            out, vout = R.denoise_var_reference(img, f["var"], dv, return_var=True, **planes)
            assert V.same_bits(out[void], img[void]) and V.same_bits(vout[void], f["var"][void]) and void.sum() > 4 * W
            # a constant image stays constant
            const = np.full(img.shape, 0.7310585786300049)
            out = R.denoise_var_reference(const, f["var"], dv, **planes)
            assert np.abs(out - const).max() <= BOUND * 0.7310585786300049, (Cn, I)
    # var == 0 everywhere and every two pixels further apart than sqrt(epsilon) * 1e8: every off-centre tap's weight is
    # below 1e-32 of the centre's, so acc = fl(9/64 F) and ws = 9/64.  The values are integers below 2^40, for which
    # 9/64 F is exact, so out == in bit for bit; for a general F the two roundings of (9/64 F) / (9/64) allow 2^-52
    # relative per level
    eps = 1e-12
    step = math.sqrt(eps) * 1e8
    assert step == 100.0
    for (w, h) in ((70, 37), (7, 5)):
        for Cn in V.CHANNELS:
            shape = (h, w) if Cn == 1 else (h, w, 3)
            ints = (1000.0 + 128.0 * rng.permutation(w * h)).reshape(h, w)
            img = ints if Cn == 1 else np.stack([ints, ints + 7.0, ints[::-1, ::-1] + 3.0], axis=2)
            assert np.abs(ints.reshape(-1)[:, None] - ints.reshape(-1)[None, :])[~np.eye(w * h, dtype=bool)].min() > step
            general = img * 1.0000000123
            zero = np.zeros((h, w))
            for I in (1, 3, 6):
                dv = R.DenoiseVar(I, sigma_color=4.0, epsilon=eps, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
                out, vout = R.denoise_var_reference(img, zero, dv, return_var=True)
                assert out.shape == shape and V.same_bits(out, img) and (vout == 0.0).all(), (w, h, Cn, I)
                out = R.denoise_var_reference(general, zero, dv)
                assert np.abs(out - general).max() <= I * 2.0**-52 * np.abs(general).max(), (w, h, Cn, I)
    # sigma_color = 0, I = 1, equal guides, a constant variance plane: var_out of an interior pixel is V sum (h_i h_j)^2 =
    # V (35/128)^2: 25 products and 24 additions of non-negative terms, then one division by ws * ws = 1: 51 roundings
    vplane = np.full((H, W), 0.37)
    dv = R.DenoiseVar(1, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0)
    _, vout = R.denoise_var_reference(f["img1"], vplane, dv, return_var=True)
    want = 0.37 * (35.0 / 128.0) ** 2
    assert np.abs(vout[2:-2, 2:-2] - want).max() <= 51 * 2.0**-53 * want and abs(vout[0, 0] - want) > 0.1 * want
    # the temporal branch: a pixel whose m2 == in * in has V == 0.0 exactly, whatever its count
    img = rng.random((H, W, 3))
    count = rng.integers(4, 100, size=(H, W)).astype(np.int32)
    var = R.variance_reference(img, R.Variance(sigma_normal=0.0, sigma_depth=0.0), m2=img * img, count=count)
    assert (var == 0.0).all() and not np.signbit(var).any()
    var = R.variance_reference(img, R.Variance(sigma_normal=0.0, sigma_depth=0.0), m2=img * img + 0.5, count=count)
    assert np.abs(var * count - 1.5).max() < 1e-12


# ---- the usefulness check on the definition alone ----
USEFUL_LEVELS = 3
SWEEP = (0.05, 0.1, 0.2, 0.5, 1.0)


def accumulated(R, W=56, H=40, K=4, N=8, seed=20261021, cell=3):
    """A floor whose depth falls with the row; the left half a noise-free checker of 3-pixel cells that no guide shows,
    the right half a smooth value under binomial K = 4 noise; N frames accumulated by temporal_filter as a running mean
    under a fixed camera, with moments."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 40.0 / (1.0 + y)
    normal = np.zeros((H, W, 3))
    normal[..., 1] = 1.0
    left = x < W // 2
    truth = np.where(left, np.where(((x // cell) + (y // cell)) % 2 == 0, 0.8, 0.2), 0.5 + 0.3 * np.sin(0.11 * x + 0.07 * y))
    cam = R.camera(W, H, math.pi / 3, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1])
    tp = R.Temporal(max_history=64, alpha=0.0, sigma_plane=0.0, sigma_normal=0.0, object=False)
    hist = None
    for _ in range(N):
        noisy = np.where(left, truth, rng.binomial(K, truth) / float(K))
        hist = R.temporal_filter(noisy, tp, cam, cam, depth, normal=normal, prev=hist, moments=True)
    assert (hist["n"] == N).all()
    return dict(truth=truth, left=left, guides=dict(depth=depth, normal=normal), hist=hist)


def _mse(a, b, mask):
    d = (a - b)[mask]
    return float((d * d).mean())


def test_no_fixed_sigma_is_as_good_on_both_regions(R):
    """The variance-guided filter at its default sigma_color lowers the noisy region's squared error, and no sigma_color of
    the sweep given to the plain denoise_filter (same guides, same levels) is at least as good on both the noise-free
    checker and the noisy region: the sweep straddles the trade-off (its small sigmas keep the checker and the noise,
    its large ones remove both).  Measured, seed 20261021, 3 levels: variance-guided 6.9e-06 on the
    checker and 0.277 of the noisy half's error; plain 0.05: 3.2e-07 / 0.916, 0.1: 2.0e-06 / 0.707, 0.2: 2.8e-05 /
    0.397, 0.5: 3.3e-03 / 0.203, 1.0: 5.3e-02 / 0.271."""
    s = accumulated(R)
    h, left, g, truth = s["hist"], s["left"], s["guides"], s["truth"]
    raw = _mse(h["out"], truth, ~left)
    assert raw > 0.004 and _mse(h["out"], truth, left) == 0.0
    var = R.variance_estimate(h["out"], R.Variance(), m2=h["m2"], count=h["n"], **g)
    assert V.same_bits(var, R.variance_reference(h["out"], R.Variance(), m2=h["m2"], count=h["n"], **g))
    dv = R.DenoiseVar(USEFUL_LEVELS, sigma_albedo=0.0)
    assert dv.sigma_color == 4.0
    out = R.denoise_var_filter(h["out"], var, dv, **g)
    assert V.same_bits(out, R.denoise_var_reference(h["out"], var, dv, **g))
    mine = (_mse(out, truth, left), _mse(out, truth, ~left))
    print(f"variance-guided, {USEFUL_LEVELS} levels: checker mse {mine[0]:.3g}, noisy ratio {mine[1] / raw:.3f}")
    assert mine[1] < raw
    pairs = []
    for sc in SWEEP:
        o = R.denoise_filter(h["out"], R.Denoise(USEFUL_LEVELS, sigma_color=sc, sigma_albedo=0.0), **g)
        pairs.append((_mse(o, truth, left), _mse(o, truth, ~left)))
        print(f"plain sigma_color {sc}: checker mse {pairs[-1][0]:.3g}, noisy ratio {pairs[-1][1] / raw:.3f}")
    assert len(pairs) >= 4
    for sc, (e_left, e_right) in zip(SWEEP, pairs):
        assert not (e_left <= mine[0] and e_right <= mine[1]), (sc, e_left, e_right, mine)
    # the sweep straddles the trade-off: one end beats the new filter on the checker, the other on the noisy half
    assert pairs[0][0] < mine[0] and pairs[0][1] > mine[1]
    assert min(p[1] for p in pairs) < mine[1] and max(p[0] for p in pairs) > mine[0]


def test_native_check(tmp_path):
    """tests/native/denoise_var_check.cpp: denoise_var_tap.hpp under g++ on frames whose V and F' are derived by hand."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "denoise_var_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-comment",
                    "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "rray_amd", "csrc"),
                    os.path.join(HERE, "native", "denoise_var_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "0 failures", r.stdout
    ok = {ln.split()[1] for ln in lines if ln.startswith("ok ")}
    assert len(ok) == len(lines) - 1 >= 30 and {"var_pair", "var_temporal", "var_temporal_zero_count", "var_depth_term",
                                                 "dv_row5_plain", "dv_interior_variance", "dv_colour_term", "dv_prefilter",
                                                 "dv_zero_variance_overflow", "dv_void", "dv_nan_variance",
                                                 "dv_level1_prefilter_step"} <= ok
