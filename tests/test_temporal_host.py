"""Temporal accumulation's definition on the host (rray.h RR_HAS_TEMPORAL): the symbols and the
structs, the refusals that need no device, rr_temporal_reference (the very function temporal_kernel calls,
rray_amd/csrc/temporal_tap.hpp) against its numpy mirror rray_amd.temporal_filter bit for bit over the case product of
tests/temporal_cases.py, the hand-derived native check, and the geometry of the reprojection on first-hit planes the CPU
oracle produces: where the history comes from, how much of it is reused, and what is rejected.  No GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import temporal_cases as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("rr_temporal_reference", "rr_temporal", "rr_temporal_device")


@pytest.fixture(scope="module")
def R():
    import rray_amd

    return rray_amd


def test_abi_symbols_and_structs(R):
    L, E = R.lib(), R._lib
    hdr = open(E.HEADER).read()
    for name in NAMES:
        assert hasattr(L, name) and name in E.EXPORTS and f"int {name}(" in hdr, name
    assert "#define RR_HAS_TEMPORAL 1" in hdr and "#define RR_ABI_VERSION 11" in hdr and L.rr_abi_version() == 11
    assert f"#define RR_MAX_TEMPORAL_HISTORY {E.RR_MAX_TEMPORAL_HISTORY}" in hdr and E.RR_MAX_TEMPORAL_HISTORY == 2**20
    assert f"#define RR_TP_OBJECT {E.RR_TP_OBJECT}" in hdr and E.RR_TP_OBJECT == 1
    D, F = E.TemporalDesc, E.TemporalFrame
    assert C.sizeof(D) == 32 and (D.flags.offset, D.max_history.offset, D.alpha.offset, D.sigma_plane.offset,
                                  D.sigma_normal.offset) == (0, 4, 8, 16, 24)
    assert C.sizeof(F) == 48 and [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 16, 24, 32, 40]
    d = R.Temporal().desc()
    assert (d.flags, d.max_history, d.alpha, d.sigma_plane, d.sigma_normal) == (1, 32, 0.0, 0.01, 0.1)
    assert R.Temporal(object=False).desc().flags == 0
    for name in ("temporal", "temporal_device"):
        assert callable(getattr(R.Renderer, name))
    for name in ("Temporal", "temporal_reference", "temporal_filter", "temporal_variance"):
        assert name in R.__all__ and hasattr(R, name)


def test_sizeof_the_structs_for_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.fail("gcc not available")
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "rray/rray.h"\n'
                   '_Static_assert(sizeof(rr_temporal_desc) == 32, "rr_temporal_desc");\n'
                   '_Static_assert(sizeof(rr_temporal_frame) == 48, "rr_temporal_frame");\n'
                   '_Static_assert(offsetof(rr_temporal_desc, max_history) == 4 && offsetof(rr_temporal_desc, alpha) == 8 &&\n'
                   '               offsetof(rr_temporal_desc, sigma_normal) == 24, "rr_temporal_desc layout");\n'
                   '_Static_assert(offsetof(rr_temporal_frame, count) == 32 && offsetof(rr_temporal_frame, m2) == 40, "frame");\n'
                   '#if !defined(RR_HAS_TEMPORAL) || RR_MAX_TEMPORAL_HISTORY != 1048576 || RR_TP_OBJECT != 1 || RR_ABI_VERSION != 11\n'
                   '#error\n#endif\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-comment", "-I" + os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "size.o")], check=True)


def test_refusals_that_need_no_device(R):
    L, E = R.lib(), R._lib
    ARG, LIM = E.RR_E_ARG, E.RR_E_LIMIT
    W, H = 7, 5
    f = T.frame(W, H)
    cam, pcam = T.cameras(R, W, H, "small")
    out, n, m2 = np.full((H, W, 3), -12345.5), np.full((H, W), -77, np.int32), np.full((H, W, 3), -12345.5)
    fake = C.c_void_p(4096)  # never dereferenced: the arguments are refused first

    def err():
        return L.rr_last_error().decode()

    def ptr(a, skip=False):
        return None if skip or a is None else C.c_void_p(a.ctypes.data)

    def desc(**kw):
        fields = dict(flags=1, max_history=8, alpha=0.1, sigma_plane=0.01, sigma_normal=0.1)
        fields.update(kw)
        return E.TemporalDesc(*fields.values())

    def frames(skip=(), m2_in=True):
        cur = E.TemporalFrame(ptr(f["img3"], "image" in skip), ptr(f["depth"], "depth" in skip),
                              ptr(f["normal"], "normal" in skip), ptr(f["object"], "object" in skip), None, None)
        prev = E.TemporalFrame(ptr(f["prev_img3"], "prev_image" in skip), ptr(f["prev_depth"], "prev_depth" in skip),
                               ptr(f["prev_normal"], "prev_normal" in skip), ptr(f["prev_object"], "prev_object" in skip),
                               ptr(f["prev_n"], "prev_count" in skip), ptr(f["prev_m23"], not m2_in))
        return cur, prev

    def ref(d=None, w=W, h=H, c=3, skip=(), m2_in=True, o=out, no=n, mo=m2, a=cam, b=pcam, null=()):
        d = d or desc()
        cur, prev = frames(skip, m2_in)
        return L.rr_temporal_reference(None if "desc" in null else C.byref(d), w, h, c, None if "cam" in null else C.byref(a),
                                       None if "cur" in null else C.byref(cur), None if "prev_cam" in null else C.byref(b),
                                       None if "prev" in null else C.byref(prev), ptr(o), ptr(no), ptr(mo))

    assert ref() == 0
    out[:], n[:], m2[:] = -12345.5, -77, -12345.5
    for what in ("desc", "cam", "cur", "prev_cam", "prev"):
        assert ref(null=(what,)) == ARG, what
    assert ref(o=None) == ARG and ref(no=None) == ARG
    for c in (0, 2, 4, -3):
        assert ref(c=c) == ARG and "channels" in err()
    for w, h in ((0, 5), (7, 0), (-1, 5), (7, -1)):
        assert ref(w=w, h=h) == ARG
    # either camera's size is not the frame's
    other = R.camera(W + 1, H, T.FOV, T.BASE)
    assert ref(a=other) == ARG and "camera" in err() and ref(b=other) == ARG and ref(b=R.camera(W, H + 1, T.FOV, T.BASE)) == ARG
    # a missing image, depth or previous count plane
    for k in ("image", "depth", "prev_image", "prev_depth", "prev_count"):
        assert ref(skip=(k,)) == ARG and "required" in err(), k
    # a term that is on without its planes; with the term off the plane may go
    terms = ((("normal",), dict(sigma_plane=0.0, sigma_normal=0.0)), (("prev_normal",), dict(sigma_normal=0.0)),
             (("object",), dict(flags=0)), (("prev_object",), dict(flags=0)))
    for skip, off in terms:
        assert ref(skip=skip) == ARG and "planes" in err(), skip
    assert ref(desc(sigma_normal=0.0), skip=("normal",)) == ARG  # the plane term needs the current normal
    assert (out == -12345.5).all() and (n == -77).all() and (m2 == -12345.5).all()
    for skip, off in terms:
        assert ref(desc(**off), skip=skip) == 0, skip
    out[:], n[:], m2[:] = -12345.5, -77, -12345.5
    # m2_out and prev.m2 go together
    assert ref(mo=None) == ARG and "m2" in err() and ref(m2_in=False) == ARG and "m2" in err()
    assert ref(mo=None, m2_in=False) == 0
    out[:], n[:] = -12345.5, -77
    # a field out of range or not finite, unknown flag bits
    bad = (dict(flags=2), dict(flags=3), dict(flags=-1), dict(max_history=0), dict(max_history=-1),
           dict(max_history=2**20 + 1), dict(alpha=-1e-300), dict(alpha=1.0000001), dict(alpha=math.nan), dict(alpha=math.inf),
           dict(sigma_plane=-1.0), dict(sigma_plane=math.nan), dict(sigma_plane=math.inf), dict(sigma_normal=-0.5),
           dict(sigma_normal=math.nan), dict(sigma_normal=math.inf))
    cur, prev = frames()
    for kw in bad:
        d = desc(**kw)
        assert ref(d) == ARG, kw
        # the device entries refuse the same before they touch the context or a buffer
        assert L.rr_temporal(None, C.byref(d), W, H, 3, C.byref(cam), C.byref(cur), C.byref(pcam), C.byref(prev), ptr(out),
                             ptr(n), ptr(m2)) == ARG, kw
        assert L.rr_temporal_device(None, C.byref(d), W, H, 3, C.byref(cam), C.byref(cur), C.byref(pcam), C.byref(prev), fake,
                                    fake, fake, None) == ARG, kw
    assert ref(desc(flags=2)) == ARG and "flag" in err()
    assert ref(desc(max_history=0)) == ARG and "max_history" in err()
    assert ref(desc(alpha=2.0)) == ARG and "alpha" in err()
    assert ref(desc(sigma_plane=math.nan)) == ARG and "sigma" in err()
    # a null context
    d = desc()
    assert L.rr_temporal(None, C.byref(d), W, H, 3, C.byref(cam), C.byref(cur), C.byref(pcam), C.byref(prev), ptr(out), ptr(n),
                         ptr(m2)) == ARG
    assert L.rr_temporal_device(None, C.byref(d), W, H, 3, C.byref(cam), C.byref(cur), C.byref(pcam), C.byref(prev),
                                C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), None) == ARG
    # an output overlapping any input (the image itself, its last double, the middle of every plane) or another output
    assert ref(o=f["img3"]) == ARG and "overlap" in err()

    class At:  # a pointer into the middle of an array
        def __init__(self, a, off):
            self.ctypes = type("P", (), {"data": a.ctypes.data + off})

    assert ref(o=At(f["img3"], f["img3"].nbytes - 8)) == ARG and "overlap" in err()
    for k in ("img3", "depth", "normal", "object", "prev_img3", "prev_depth", "prev_normal", "prev_object", "prev_n", "prev_m23"):
        for which in ("o", "no", "mo"):
            assert ref(**{which: At(f[k], 8)}) == ARG and "overlap" in err(), (k, which)
    assert ref(no=At(out, 16)) == ARG and ref(mo=At(out, out.nbytes - 8)) == ARG and ref(mo=At(n, 0)) == ARG
    # W * H >= 2^31
    big = lambda w, h: ref(w=w, h=h, a=R.camera(w, h, T.FOV, T.BASE), b=R.camera(w, h, T.FOV, T.BASE))  # noqa: E731
    assert big(2**16, 2**15) == LIM and "2^31" in err()
    assert big(2**31, 1) == LIM and big(1, 2**31) == LIM and big(2**40, 2**40) == LIM
    assert (out == -12345.5).all() and (n == -77).all()
    # the boundary values serve
    assert ref(desc(max_history=2**20, alpha=1.0, sigma_plane=5e-324, sigma_normal=1e300)) == 0
    assert ref(desc(max_history=1, alpha=0.0, sigma_plane=0.0, sigma_normal=0.0, flags=0)) == 0 and (n == 1).all()


@pytest.mark.parametrize("W,H", T.FRAMES, ids=[f"{w}x{h}" for w, h in T.FRAMES])
def test_reference_equals_the_numpy_mirror(R, W, H):
    cases = T.cases(W, H)
    assert len(cases) == 2 * 6 * 2 * 2 * 3 * 5
    for case in cases:
        args, kwargs = T.arguments(R, W, H, *case)
        got = R.temporal_reference(*args, **kwargs)
        want = T.expected(W, H, *case)
        assert got["out"].shape == args[0].shape and np.array_equal(got["out"], want["out"], equal_nan=True), case
        assert T.same_result(got, want), case
        assert (got["m2"] is not None) == case[2]


def test_the_cases_are_not_vacuous(R):
    """On the 13 x 9 frame every term rejects some taps and passes others, every camera but the one that looks away
    keeps some history and loses some, the caps and the floor of the blend factor bind, and the edge cases are there."""
    W, H = 13, 9
    f = T.frame(W, H)
    assert np.isinf(f["depth"]).sum() == 1 and np.isnan(f["depth"]).sum() == 1 and (f["object"] < 0).sum() == 1
    assert np.isnan(f["img3"]).any() and np.isinf(f["img3"]).any() and np.isnan(f["prev_img3"]).any()
    assert np.isnan(f["normal"]).any() and np.isnan(f["prev_normal"]).any()
    assert (f["prev_n"] == 0).sum() >= 5 and (f["prev_n"] > 2**20).sum() == 2 and (f["prev_n"] < 0).sum() == 1
    for C_ in T.CHANNELS:
        base = {cam: T.expected(W, H, C_, "none", True, 0.0, 2**20, cam) for cam in T.CAMERAS}
        assert (base["away"]["n"] == 1).all() and T.same_bits(base["away"]["out"], f[f"img{C_}"])
        for cam in ("static", "small", "large", "rotated"):
            kept = base[cam]["n"] > 1
            assert 0.15 < kept.mean() < 0.98, (cam, kept.mean())
            for combo in ("object", "plane", "normal", "all"):
                e = T.expected(W, H, C_, combo, True, 0.0, 2**20, cam)
                assert not T.same_bits(e["out"], base[cam]["out"]) and (e["n"] > 1).mean() > 0.04, (cam, combo, (e["n"] > 1).mean())
            assert not T.same_bits(T.expected(W, H, C_, "none", True, 0.2, 2**20, cam)["out"], base[cam]["out"])
            assert not np.array_equal(T.expected(W, H, C_, "none", True, 0.0, 4, cam)["n"], base[cam]["n"])
            assert T.expected(W, H, C_, "none", True, 0.0, 4, cam)["n"].max() == 4
            assert T.expected(W, H, C_, "none", True, 0.0, 1, cam)["n"].max() == 1
        assert base["static"]["n"].max() == 2**20 and (base["small"]["ws"] > 0).any()
        # under a moving camera the taps are resampled: fractional weights
        assert ((base["small"]["ws"] > 0) & (base["small"]["ws"] < 1)).any()


def test_first_frame_and_the_recurrence_with_a_static_camera(R):
    """prev=None is an all-zero history: out = in, n = 1, m2 = in^2.  Then N calls under a fixed camera: n counts
    1..max_history and out follows out + (in - out) * max(1/n, alpha) term by term; temporal_variance of a mean."""
    W, H = 7, 5
    f = T.frame(W, H)
    cam, _ = T.cameras(R, W, H, "static")
    rng = np.random.default_rng(5)
    live = np.isfinite(f["depth"]) & (f["object"] >= 0)
    for alpha, cap in ((0.0, 4), (0.3, 32)):
        tp = R.Temporal(max_history=cap, alpha=alpha, sigma_plane=0.01, sigma_normal=0.1)
        hist, want, want2 = None, None, None
        for k in range(1, 8):
            img = rng.random((H, W))
            hist = R.temporal_reference(img, tp, cam, cam, f["depth"], normal=f["normal"], object=f["object"], prev=hist,
                                        moments=True)
            n = min(k, cap)
            a = max(1.0 / n, alpha)
            want = img.copy() if k == 1 else np.where(live, want + (img - want) * a, img)
            want2 = img * img if k == 1 else np.where(live, want2 + (img * img - want2) * a, img * img)
            ok = ~np.isnan(f["normal"]).any(axis=2)  # a NaN normal rejects the tap: no history there
            assert np.array_equal(hist["n"], np.where(live & ok, n, 1)), k
            assert T.same_bits(hist["out"][ok], want[ok]) and T.same_bits(hist["m2"][ok], want2[ok]), k
            assert T.same_bits(hist["out"][~ok], img[~ok])
            want, want2 = np.where(ok, want, img), np.where(ok, want2, img * img)
        var = R.temporal_variance(hist["out"], hist["m2"])
        assert var.shape == (H, W) and (var >= 0.0).all() and var[live].max() > 0.001
        assert np.array_equal(var, np.maximum(hist["m2"] - hist["out"] * hist["out"], 0.0))


def test_native_check(tmp_path):
    """tests/native/temporal_check.cpp: temporal_tap.hpp under g++ on frames whose results are derived by hand."""
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path / "temporal_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-comment",
                    "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "rray_amd", "csrc"),
                    os.path.join(HERE, "native", "temporal_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines[-1] == "0 failures", r.stdout
    ok = {ln.split()[1] for ln in lines if ln.startswith("ok ")}
    assert len(ok) == len(lines) - 1 and {"wall_shift_1", "wall_shift_3", "wall_left_columns", "static_recurrence",
                                          "static_cap", "void_pixel", "behind_camera"} <= ok, r.stdout


# ---- geometry, on planes the CPU oracle produces ----
# Two views of the floor, cube and sphere scene: the current camera and a previous one moved sideways and turned a
# little, so that part of the current frame was outside the previous one and the cube and the sphere hid floor then.
CUR_VIEW = ((0.0, 2.0, -5.0), (0.0, 0.8, 0.0))
PREV_VIEW = ((0.9, 2.2, -4.8), (0.45, 0.8, 0.0))
# a previous camera far to the side looking past the scene: much of the current frame projects outside its frame or
# lies behind it
FAR_VIEW = ((4.0, 1.5, -1.0), (9.0, 1.0, 0.5))


@pytest.fixture(scope="module")
def geometry(R, oracle_mod):
    oracle = oracle_mod
    o = T.oracle_scene(oracle)
    out = {}
    for W, H in ((48, 32), (24, 16)):
        views = {}
        for name, (frm, to) in (("cur", CUR_VIEW), ("prev", PREV_VIEW), ("far", FAR_VIEW)):
            cam = R.camera(W, H, math.pi / 3, oracle.Oracle.mat.view_transform(frm, to, (0.0, 1.0, 0.0)))
            views[name] = (cam, T.oracle_planes(oracle, o, cam))
        out[(W, H)] = views
    return o, out


def _project(cam, P):
    """continuous pixel coordinates of world points in `cam`, and their camera-space z, in plain numpy"""
    Tm = np.array(list(cam.transform)).reshape(4, 4)
    c = P @ Tm[:3, :3].T + Tm[:3, 3]
    with np.errstate(all="ignore"):
        fx = (cam.half_width - c[..., 0] / -c[..., 2]) / cam.pixel_size - 0.5
        fy = (cam.half_height - c[..., 1] / -c[..., 2]) / cam.pixel_size - 0.5
    return fx, fy, c[..., 2]


def _history_of_points(R, cam, cur, pcam, prev):
    """temporal_reference and temporal_filter (with its history) where the history image is the previous view's world
    hit points and the current image is the current view's"""
    hist = {"out": prev["point"], "n": np.ones(prev["depth"].shape, np.int32), "m2": None, "depth": prev["depth"],
            "normal": prev["normal"], "object": prev["object"]}
    args = (cur["point"], R.Temporal(), cam, pcam, cur["depth"])
    kw = dict(normal=cur["normal"], object=cur["object"], prev=hist)
    got = R.temporal_reference(*args, **kw)
    mirror = R.temporal_filter(*args, return_history=True, **kw)
    assert T.same_result(got, mirror)
    return got, mirror


@pytest.mark.parametrize("size", ((48, 32), (24, 16)), ids=("48x32", "24x16"))
def test_the_history_comes_from_where_the_point_was(R, geometry, size):
    """For every pixel with a surviving tap, h — a convex combination of the previous view's hit points at the taps —
    projects through the previous camera within 1 + 1e-9 pixels of (fx, fy) in each axis: a projective map keeps a convex
    combination of points in front of the camera inside the hull of their projections, the tap centres."""
    _, views = geometry
    (cam, cur), (pcam, prev) = views[size]["cur"], views[size]["prev"]
    got, m = _history_of_points(R, cam, cur, pcam, prev)
    keep = got["n"] > 1
    assert keep.sum() > 0.5 * keep.size
    hx, hy, hz = _project(pcam, m["h"][keep])
    dx, dy = np.abs(hx - m["fx"][keep]), np.abs(hy - m["fy"][keep])
    print(f"{size}: {int(keep.sum())} pixels keep a history; |projection of h - (fx, fy)| max {dx.max():.4f}, {dy.max():.4f}")
    assert (hz < 0.0).all() and dx.max() <= 1.0 + 1e-9 and dy.max() <= 1.0 + 1e-9
    # and fx, fy are where the current hit points project
    px, py, _ = _project(pcam, cur["point"][keep])
    assert np.abs(px - m["fx"][keep]).max() < 1e-9 and np.abs(py - m["fy"][keep]).max() < 1e-9


@pytest.mark.parametrize("size", ((48, 32), (24, 16)), ids=("48x32", "24x16"))
def test_reuse_and_occlusion(R, geometry, size):
    """Of the current hits that are visible from the previous eye (an oracle occlusion query toward the previous origin)
    and project at least one pixel inside its frame, at least 0.95 keep a history with the Temporal() defaults.  The
    share of the hits occluded from the previous eye that keep one is printed, not asserted: thin disocclusion bands
    legitimately pick up coplanar floor taps."""
    o, views = geometry
    (cam, cur), (pcam, prev) = views[size]["cur"], views[size]["prev"]
    W, H = size
    got, _ = _history_of_points(R, cam, cur, pcam, prev)
    hit = cur["object"] >= 0
    fx, fy, cz = _project(pcam, cur["point"])
    # the previous frame covers [-0.5, W - 0.5] x [-0.5, H - 0.5] in these coordinates: one pixel inside it
    inside = hit & (cz < 0.0) & (fx >= 0.5) & (fx <= W - 1.5) & (fy >= 0.5) & (fy <= H - 1.5)
    eye = prev["origin"].tolist()
    # from over_point, the oracle's own offset hit point, as is_shadowed is asked when shading
    occluded = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(inside)):
        occluded[y, x] = o.is_shadowed(cur["over_point"][y, x].tolist(), eye)
    visible = inside & ~occluded
    kept = got["n"] > 1
    share = kept[visible].mean()
    occ = inside & occluded
    print(f"{size}: reuse share {share:.4f} over {int(visible.sum())} visible hits; "
          f"{int(kept[occ].sum())} of {int(occ.sum())} occluded hits keep a history "
          f"({(kept[occ].mean() if occ.any() else 0.0):.3f})")
    assert visible.sum() > 0.4 * W * H and occ.sum() > 0
    assert share >= 0.95


@pytest.mark.parametrize("size", ((48, 32), (24, 16)), ids=("48x32", "24x16"))
def test_rejection_outside_the_previous_frame(R, geometry, size):
    """Every current hit that projects more than one pixel outside the previous frame, or behind the previous camera,
    has n_out == 1."""
    _, views = geometry
    W, H = size
    (cam, cur) = views[size]["cur"]
    seen = 0
    for name in ("prev", "far"):
        pcam, prev = views[size][name]
        got, _ = _history_of_points(R, cam, cur, pcam, prev)
        hit = cur["object"] >= 0
        fx, fy, cz = _project(pcam, cur["point"])
        with np.errstate(invalid="ignore"):
            outside = hit & ((cz >= 0.0) | (fx < -1.5) | (fx > W + 0.5) | (fy < -1.5) | (fy > H + 0.5))
        seen += int(outside.sum())
        assert (got["n"][outside] == 1).all() and T.same_bits(got["out"][outside], cur["point"][outside]), name
        assert (got["n"][~hit] == 1).all()
        if name == "far":
            assert (hit & (cz >= 0.0)).sum() > 0 and outside.sum() > 0.2 * hit.sum()
    assert seen > 0
