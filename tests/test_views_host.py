"""CPU-side tests of batches of views (rr_render_views, additive to ABI 11): exports, the header's RR_HAS_VIEWS, the
argument refusals that need no device, the plan of a batch (rray_amd/csrc/frame_plan.hpp, compiled with g++ into
tests/native/view_plan_check.cpp; the expectations below are derived by hand from the definition: a view takes its
samples rounded up to whole 64-lane waves, a pass holds whole views) and the documents.  The frames themselves are
checked on the GPU (tests/test_gpu_views.py)."""
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
NAMES = ("rr_render_views", "rr_render_views_device")
RR_E_ARG, RR_E_LIMIT = -1, -5


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


def test_symbols_are_exported_and_listed(R):
    L = R.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in R._lib.EXPORTS, n
    hdr = open(os.path.join(ROOT, "include", "rray", "rray.h")).read()
    assert re.search(r"^#define RR_HAS_VIEWS 1\b", hdr, re.M)
    for n in NAMES:
        assert re.search(rf"^int {n}\(rr_ctx\* ctx, const rr_camera\* cams, int32_t n_views,", hdr, re.M), n
    assert L.rr_abi_version() == 11  # additive: the version does not move
    for n in ("render_views", "render_views_device"):
        assert callable(getattr(R.Renderer, n))


def test_bad_arguments_are_refused_without_a_device(R):
    L, E = R.lib(), R._lib
    cams = (E.Camera * 3)(*[R.camera(16, 16, 1.0 - 0.1 * k) for k in range(3)])
    mixed = (E.Camera * 3)(R.camera(16, 16, 1.0), R.camera(16, 16, 0.9), R.camera(16, 8, 0.8))
    ok = E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 0, 0)
    avg = np.zeros((3, 8, 8, 3))
    cnv = np.zeros((3, 16, 16, 3))

    def host(c, n, o, canvas=True, image=True):
        return L.rr_render_views(None, c, n, o, cnv.ctypes.data_as(E._D) if canvas else None,
                                 avg.ctypes.data_as(E._D) if image else None, None)

    def dev(c, n, o, canvas=True, image=True):
        return L.rr_render_views_device(None, c, n, o, C.c_void_p(cnv.ctypes.data) if canvas else None,
                                        C.c_void_p(avg.ctypes.data) if image else None, None)

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
        for bad in (E.RenderOpts(2, 5, 0, 0, 1, 2, 8, E.RR_OUT_AVG, 0, 0), E.RenderOpts(2, 5, 0, 0, 0, 2, 8, E.RR_OUT_AVG, 0, 0),
                    E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 0, 4), E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG, 2, 4)):
            assert f(cams, 3, C.byref(bad)) == RR_E_ARG and "part 0 of 1, no band" in err()
        f32 = E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_OUT_AVG_F32, 0, 0)
        assert f(cams, 3, C.byref(f32)) == RR_E_ARG and "RR_OUT_AVG_F32" in err()
        inter = E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_PART_INTERLEAVE, 0, 0)
        assert f(cams, 3, C.byref(inter)) == RR_E_ARG and "RR_PART_INTERLEAVE" in err()
        # a requested output needs its buffer; an unrequested one's pointer is ignored
        assert f(cams, 3, C.byref(ok), image=False) == RR_E_ARG and "null image buffer" in err()
        both = E.RenderOpts(2, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_OUT_CANVAS, 0, 0)
        assert f(cams, 3, C.byref(both), canvas=False) == RR_E_ARG and "null canvas buffer" in err()
        assert f(cams, 3, C.byref(ok), canvas=False) == RR_E_ARG and "null context" in err()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path_factory.mktemp("view_plan") / "view_plan_check")
    # -Wno-comment: the public header's text names a glob ("csrc/*") inside a comment
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-I" + CSRC,
                    os.path.join(HERE, "native", "view_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        head, _, msg = line.partition(" msg=")
        kind, name, *fields = head.split()
        row = {}
        for f in fields:
            k, v = f.split("=")
            row[k] = v if k == "family" else int(v)
        row["msg"] = msg
        assert (kind, name) not in table
        table[(kind, name)] = row
    return table


def check(rows, kind, name, **want):
    row = rows[(kind, name)]
    assert {k: row[k] for k in want} == want, f"{kind} {name}"


def test_events_per_view(rows):
    # a view's samples rounded up to whole waves of 64: 256; 143 -> 192; 180 -> 192
    for name, e in (("16x16", 256), ("13x11", 192), ("15x12", 192), ("8x8", 64), ("1x1", 64), ("1920x1080", 2073600)):
        check(rows, "events", name, E=e)
    assert 1920 * 1080 % 64 == 0


def test_passes_hold_whole_views(rows):
    check(rows, "plan", "nine_16x16_batch_1024", views_per_pass=4, B=1024, tile_fast=1, err=0)
    check(rows, "plan", "seven_13x11_batch_1024", views_per_pass=5, B=960, tile_fast=0, err=0)  # 5 x 192 <= 1024 < 6 x 192
    check(rows, "plan", "three_16x16", views_per_pass=3, B=768, err=0)  # never more than the batch has
    check(rows, "plan", "two_32x32_batch_1024", views_per_pass=1, B=1024, err=0)
    check(rows, "plan", "one_40x32_batch_1024", err=RR_E_LIMIT)  # 1280 events fit no pass of 1024
    assert "one pass" in rows[("plan", "one_40x32_batch_1024")]["msg"]
    check(rows, "plan", "bad_total", err=RR_E_ARG)


def test_only_the_in_wave_families_serve(rows):
    for name, family in (("three_16x16", "Level0"), ("chain", "Chain"), ("tree", "Tree"), ("level0_depth0", "Level0")):
        check(rows, "plan", name, family=family, levels=1, zero_lcount=0, err=0, msg="")
    for name, family in (("fused_levels", "FusedLevels"), ("unfused", "Unfused")):
        check(rows, "plan", name, family=family, err=RR_E_ARG)
        assert "per-level" in rows[("plan", name)]["msg"]


def test_no_order_no_resident_loop_no_deep_queue(rows):
    for name in ("nine_16x16_batch_1024", "three_16x16", "chain", "tree", "grouped_64x64", "flat_64x64", "chain_deep"):
        check(rows, "plan", name, order=0, persist=0, spill=0, passes=0, err=0)
    # the same shapes as single frames do get them: the cases above prove something
    check(rows, "plan", "single_grouped_64x64", order=1, views_per_pass=0, err=0)
    check(rows, "plan", "single_flat_64x64", persist=1, views_per_pass=0, err=0)


def test_documents_name_the_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert re.search(rf"\bfn {n}\s*\(", integ), n
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in NAMES:
        assert n in readme, n
        assert n in design, n
    assert "render_views" in readme
    assert re.search(r"^### 3\.16 ", design, re.M)
