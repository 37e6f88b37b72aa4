"""CPU-side tests of the device-resident ray queries (rr_camera_rays_device, rr_color_at_device, rr_hit_at_device,
rr_is_shadowed_device; additive to ABI 11): declarations, exports, the header's RR_HAS_RAYS_DEVICE, the Python mirror,
the refusals that need no device, the record layout the device writes (hit_dtype), the pass split of rr_hit_at_device
(rray_amd/csrc/frame_plan.hpp plan_ray_passes, compiled with g++ into tests/native/ray_pass_check.cpp; the
expectations are derived by hand from the definition: passes of min(batch, 2^22, n) rays, the last one what is left)
and the documents.  The queries themselves are checked on the GPU (tests/test_gpu_rays.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rray_amd", "csrc")
# name: (arguments of the C declaration, its first parameters as the header spells them)
NAMES = {"rr_camera_rays_device": (4, r"rr_ctx\* ctx, const rr_camera\* cam, void\* d_rays, void\* hip_stream\)"),
         "rr_color_at_device": (8, r"rr_ctx\* ctx, int64_t n, const void\* d_rays, int32_t remaining, uint64_t seed,"),
         "rr_hit_at_device": (5, r"rr_ctx\* ctx, int64_t n, const void\* d_rays, void\* d_hits, void\* hip_stream\)"),
         "rr_is_shadowed_device": (6, r"rr_ctx\* ctx, int64_t n, const void\* d_points, const void\* d_light_positions,")}
RR_E_ARG = -1


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


def test_symbols_are_declared_exported_and_bound(R):
    L = R.lib()
    hdr = open(os.path.join(ROOT, "include", "rray", "rray.h")).read()
    assert re.search(r"^#define RR_HAS_RAYS_DEVICE 1\b", hdr, re.M)
    assert re.search(r"^#define RR_ABI_VERSION 11\b", hdr, re.M)
    assert L.rr_abi_version() == 11  # additive: the version does not move
    for n, (argc, params) in NAMES.items():
        assert hasattr(L, n), n
        assert n in R._lib.EXPORTS, n
        assert getattr(L, n).argtypes is not None and len(getattr(L, n).argtypes) == argc, n
        assert re.search(rf"^int {n}\({params}", hdr, re.M), n
    for n in ("camera_rays_device", "color_at_device", "hit_at_device", "is_shadowed_device"):
        assert callable(getattr(R.Renderer, n)), n
    from rray_amd import build

    assert "render_rays.hip" in build.SOURCES and os.path.exists(os.path.join(CSRC, "render_rays.hip"))
    # the mirror does not import torch: pointers are integers
    for f in ("render.py", "_lib.py"):
        assert not re.search(r"^\s*(import|from) torch\b", open(os.path.join(ROOT, "rray_amd", f)).read(), re.M), f


def test_a_null_context_is_refused_without_a_device(R):
    L, E = R.lib(), R._lib
    cam = R.camera(16, 16, 1.0)
    buf = (C.c_double * 64)()
    p = C.c_void_p(C.addressof(buf))
    assert L.rr_camera_rays_device(None, C.byref(cam), p, None) == RR_E_ARG
    assert L.rr_camera_rays_device(None, None, None, None) == RR_E_ARG
    for n in (1, 0, -1):  # a null context is refused whatever n is
        assert L.rr_color_at_device(None, n, p, 5, 0, 0, p, None) == RR_E_ARG
        assert "null context" in L.rr_last_error().decode()
        assert L.rr_hit_at_device(None, n, p, p, None) == RR_E_ARG
        assert L.rr_is_shadowed_device(None, n, p, p, p, None) == RR_E_ARG
    assert L.rr_color_at_device(None, 1, None, 5, 0, 0, None, None) == RR_E_ARG
    assert L.rr_color_at_device(None, 1, p, -1, 0, 0, p, None) == RR_E_ARG  # before `remaining` is looked at
    assert E.RR_E_ARG == RR_E_ARG


def test_the_record_layout_the_device_writes(R):
    dt = R._lib.hit_dtype()
    assert dt.itemsize == 192 == C.sizeof(R._lib.Hit)
    off = {n: dt.fields[n][1] for n in dt.names}
    assert (off["object"], off["inside"], off["t"], off["point"], off["n2"]) == (0, 4, 8, 32, 184)
    # word w of a record (8 bytes each): 0 = {object, inside}, then the double fields in the struct's order — the order
    # of hit_kernel's planes (kernels.hpp HitOut) that hit_records_kernel relies on
    words = ["t", "u", "v", "point", "eyev", "normalv", "over_point", "under_point", "reflectv", "n1", "n2"]
    assert list(dt.names) == ["object", "inside"] + words
    w = 1
    for n in words:
        assert off[n] == 8 * w, n
        w += 3 if dt.fields[n][0].shape == (3,) else 1
    assert w == 24
    # the torch idiom of the docstrings: columns of hits.view(float64)
    assert (off["t"] // 8, off["point"] // 8, off["normalv"] // 8, off["n1"] // 8, off["n2"] // 8) == (1, 4, 10, 22, 23)


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not available")
    exe = str(tmp_path_factory.mktemp("ray_pass") / "ray_pass_check")
    # -Wno-comment: the public header's text names a glob ("csrc/*") inside a comment
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-comment", "-I" + CSRC,
                    os.path.join(HERE, "native", "ray_pass_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        kind, name, *fields = line.split()
        assert (kind, name) not in table
        table[(kind, name)] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return table


def check(rows, name, **want):
    row = rows[("pass", name)]
    assert {k: row[k] for k in want} == want, name


def test_the_pass_sizes_sum_to_n_and_none_exceeds_the_cap(rows):
    assert rows[("pass_max", "limit")]["value"] == 2**22
    seen = 0
    for (kind, name), row in rows.items():
        if kind != "pass":
            continue
        seen += 1
        n, cap = max(row["n"], 0), min(row["batch"], 2**22)
        assert row["sum"] == n, name
        assert row["count"] == row["passes"], name
        assert row["largest"] <= cap and row["pass"] <= cap, name
        if n:
            assert 1 <= row["smallest"] and row["largest"] == row["pass"], name
            assert row["passes"] == -(-n // row["pass"]), name
            assert row["pass"] == min(cap, n), name  # as few passes as the cap allows
    assert seen >= 15


def test_the_edge_cases_of_the_pass_split(rows):
    check(rows, "none", passes=0, sum=0)
    check(rows, "negative", passes=0, sum=0)
    check(rows, "one", passes=1, largest=1)
    check(rows, "one_batch_1", passes=1, largest=1)
    check(rows, "seven_batch_1", passes=7, largest=1, smallest=1)
    check(rows, "n300_batch_128", passes=3, largest=128, smallest=44)
    check(rows, "n2500_batch_1024", passes=3, largest=1024, smallest=452)
    check(rows, "exactly_batch_1024", passes=1, largest=1024)
    check(rows, "batch_1024_minus_1", passes=1, largest=1023)
    check(rows, "batch_1024_plus_1", passes=2, largest=1024, smallest=1)
    check(rows, "three_batches_1024", passes=3, largest=1024, smallest=1024)
    check(rows, "exactly_cap", passes=1, largest=2**22)
    check(rows, "cap_minus_1", passes=1, largest=2**22 - 1)
    check(rows, "cap_plus_1", passes=2, largest=2**22, smallest=1)
    check(rows, "small_default", passes=1, largest=300)
    check(rows, "limit_32_bit", passes=1024, largest=2**22, smallest=2**22 - 1)
    check(rows, "batch_below_cap", passes=6, largest=2**21, smallest=2**21)


def test_documents_name_the_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in NAMES:
        assert re.search(rf"\bfn {n}\s*\(", integ), n
        assert n in readme, n
        assert n in design, n
    assert "color_at_device" in readme and "camera_rays_device" in readme
    assert re.search(r"^### 3\.18 ", design, re.M)
