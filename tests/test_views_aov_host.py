"""CPU-side tests of the first-hit planes of batches of views (rr_render_views_aov, additive to ABI 11): exports, the
header's RR_HAS_VIEWS_AOV, the Python mirror, the argument refusals that need no device, the pass split
(rray_amd/csrc/frame_plan.hpp plan_views_aov, compiled with g++ into tests/native/view_aov_plan_check.cpp; the
expectations below are derived by hand from the definition: a view takes its samples rounded up to whole 64-lane waves,
a pass holds whole views and at most min(batch, 2^31 - 64) events) and the documents.  The planes themselves are checked
on the GPU (tests/test_gpu_views_aov.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rray_amd", "csrc")
NAMES = ("rr_render_views_aov", "rr_render_views_aov_device")
RR_E_ARG, RR_E_LIMIT = -1, -5


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


def test_symbols_are_declared_exported_and_bound(R):
    L = R.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in R._lib.EXPORTS, n
        assert getattr(L, n).argtypes is not None, n
    hdr = open(os.path.join(ROOT, "include", "rray", "rray.h")).read()
    assert re.search(r"^#define RR_HAS_VIEWS_AOV 1\b", hdr, re.M)
    for n in NAMES:
        assert re.search(rf"^int {n}\(rr_ctx\* ctx, const rr_camera\* cams, int32_t n_views, const rr_render_opts\* opts,\s+"
                         r"int32_t planes,", hdr, re.M), n
    assert L.rr_abi_version() == 11  # additive: the version does not move
    assert len(L.rr_render_views_aov.argtypes) == 10 and len(L.rr_render_views_aov_device.argtypes) == 10
    for n in ("render_views_aov", "render_views_aov_device"):
        assert callable(getattr(R.Renderer, n))
    # the six units are part of the build, each built like the first-hit unit it mirrors: the same source file and
    # flags, and of the defines only the level-0 source differs
    from rray_amd import build

    for g in (0, 1, 2):
        for lc in ("lds", "gl"):
            u, like = f"render_views_hit_g{g}_{lc}.hip", f"render_hit_g{g}_{lc}.hip"
            assert u in build.SOURCES and like in build.SOURCES, u
            (src, defs, flags), (src_l, defs_l, flags_l) = build.UNITS[u], build.UNITS[like]
            assert flags == flags_l, u
            assert src == src_l and os.path.exists(os.path.join(CSRC, src)), u
            assert set(defs) ^ set(defs_l) == {"RR_UNIT_SRC=2", "RR_UNIT_SRC=0"}, u


def test_bad_arguments_are_refused_without_a_device(R):
    L, E = R.lib(), R._lib
    cams = (E.Camera * 3)(*[R.camera(16, 16, 1.0 - 0.1 * k) for k in range(3)])
    mixed = (E.Camera * 3)(R.camera(16, 16, 1.0), R.camera(16, 16, 0.9), R.camera(16, 8, 0.8))
    ok = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    depth, obj = np.zeros((3, 16, 16)), np.zeros((3, 16, 16), np.int32)
    DEPTH_OBJECT = E.RR_AOV_DEPTH | E.RR_AOV_OBJECT

    def host(c, n, o, planes=DEPTH_OBJECT, d=True, i=True):
        return L.rr_render_views_aov(None, c, n, o, planes, depth.ctypes.data_as(E._D) if d else None, None,
                                     obj.ctypes.data_as(E._I) if i else None, None, None)

    def dev(c, n, o, planes=DEPTH_OBJECT, d=True, i=True):
        return L.rr_render_views_aov_device(None, c, n, o, planes, C.c_void_p(depth.ctypes.data) if d else None, None,
                                            C.c_void_p(obj.ctypes.data) if i else None, None, None)

    def err():
        return L.rr_last_error().decode()

    for f in (host, dev):
        assert f(cams, 3, C.byref(ok)) == RR_E_ARG and "null context" in err()
        assert f(cams, 0, C.byref(ok)) == RR_E_ARG and "null context" in err()  # even an empty batch needs a context
        assert f(None, 3, C.byref(ok)) == RR_E_ARG and "null camera array" in err()
        assert f(cams, 3, None) == RR_E_ARG and "null options" in err()
        assert f(cams, -1, C.byref(ok)) == RR_E_ARG and "n_views is negative" in err()
        assert f(mixed, 3, C.byref(ok)) == RR_E_ARG
        assert "share hsize and vsize" in err() and "camera 2 is 16x8" in err()
        assert f(mixed, 2, C.byref(ok)) == RR_E_ARG and "null context" in err()  # the first two agree
        for bad in (E.RenderOpts(1, 0, 0, 0, 1, 2, 8, 0, 0, 0), E.RenderOpts(1, 0, 0, 0, 0, 2, 8, 0, 0, 0),
                    E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 4), E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 2, 4)):
            assert f(cams, 3, C.byref(bad)) == RR_E_ARG and "part 0 of 1, no band" in err()
        assert f(cams, 3, C.byref(ok), planes=0) == RR_E_ARG and "non-empty combination" in err()
        assert f(cams, 3, C.byref(ok), planes=16 | E.RR_AOV_DEPTH) == RR_E_ARG and "non-empty combination" in err()
        # a requested plane needs its buffer; an unrequested one's pointer is ignored
        assert f(cams, 3, C.byref(ok), i=False) == RR_E_ARG and "null buffer" in err()
        assert f(cams, 3, C.byref(ok), d=False) == RR_E_ARG and "null buffer" in err()
        assert f(cams, 3, C.byref(ok), planes=E.RR_AOV_DEPTH, i=False) == RR_E_ARG and "null context" in err()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path_factory.mktemp("view_aov_plan") / "view_aov_plan_check")
    # -Wno-comment: the public header's text names a glob ("csrc/*") inside a comment
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-I" + CSRC,
                    os.path.join(HERE, "native", "view_aov_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        head, _, msg = line.partition(" msg=")
        kind, name, *fields = head.split()
        row = {k: int(v) for k, v in (f.split("=") for f in fields)}
        row["msg"] = msg
        assert (kind, name) not in table
        table[(kind, name)] = row
    return table


def check(rows, kind, name, **want):
    row = rows[(kind, name)]
    assert {k: row[k] for k in want} == want, f"{kind} {name}"


def test_the_pass_cap_is_the_batch_or_the_32_bit_index(rows):
    check(rows, "cap", "limits", default=2**27, small=1024, huge=2**31 - 64)


def test_passes_hold_whole_views(rows):
    # 9 views of 256 events under a batch of 1024: 4, 4 and 1; 7 ragged views of 143 -> 192 events: 5 and 2
    check(rows, "plan", "nine_16x16_batch_1024", view_e=256, views_per_pass=4, passes=3, tile_fast=1, err=0, msg="")
    check(rows, "plan", "seven_13x11_batch_1024", view_e=192, views_per_pass=5, passes=2, tile_fast=0, err=0, msg="")
    check(rows, "plan", "three_16x16", views_per_pass=3, passes=1, err=0)  # never more than the batch has
    check(rows, "plan", "none", view_e=256, views_per_pass=0, passes=0, err=0)
    check(rows, "plan", "one_1x1", view_e=64, views_per_pass=1, passes=1, tile_fast=0, err=0)
    check(rows, "plan", "one_40x32_batch_2048", view_e=1280, views_per_pass=1, passes=1, err=0)
    check(rows, "plan", "bad_size", err=RR_E_ARG)
    check(rows, "plan", "negative_views", err=RR_E_ARG)


def test_a_view_that_fits_no_pass_is_refused(rows):
    check(rows, "plan", "two_40x32_batch_1024", err=RR_E_LIMIT, views_per_pass=0)  # 1280 events fit no pass of 1024
    msg = rows[("plan", "two_40x32_batch_1024")]["msg"]
    assert "one pass" in msg and "rr_render_aov" in msg
    # exactly the cap fits, one wave more does not: under the context's batch and under the 32-bit index limit
    check(rows, "plan", "exactly_batch_1024", view_e=1024, views_per_pass=1, passes=3, err=0)
    check(rows, "plan", "batch_1024_plus_64", view_e=1088, err=RR_E_LIMIT)
    check(rows, "plan", "exactly_cap31", view_e=2**31 - 64, views_per_pass=1, passes=2, err=0)
    check(rows, "plan", "cap31_plus_64", view_e=2**31, err=RR_E_LIMIT)
    assert "one pass" in rows[("plan", "cap31_plus_64")]["msg"]


def test_the_colour_batches_share_the_arithmetic(rows):
    for name in ("nine_16x16_batch_1024", "seven_13x11_batch_1024"):
        assert rows[("colour", name)]["views_per_pass"] == rows[("plan", name)]["views_per_pass"], name
        assert rows[("colour", name)]["err"] == 0
    check(rows, "colour", "two_40x32_batch_1024", err=RR_E_LIMIT, views_per_pass=0)
    assert "rr_render)" in rows[("colour", "two_40x32_batch_1024")]["msg"]  # each names its own single-frame call
    src = open(os.path.join(CSRC, "frame_plan.hpp")).read()
    assert src.count("<< 31) - 64") == 1  # stated once, in view_pass_cap


def test_documents_name_the_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert re.search(rf"\bfn {n}\s*\(", integ), n
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in NAMES:
        assert n in readme, n
        assert n in design, n
    assert "render_views_aov" in readme
    assert re.search(r"^### 3\.17 ", design, re.M)
