"""CPU-side tests of the first-hit ABI (ABI 11: rr_hit, rr_hit_at, rr_render_aov, rr_render_aov_device): the record's
layout on both sides of the binding, argument refusals that never reach a device, and the documents."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rray", "rray.h")


@pytest.fixture(scope="module")
def R():
    from rray_amd import build

    build.build()
    import rray_amd

    return rray_amd


def header_hit_fields():
    """[(name, ctype, count)] of `rr_hit` in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*rr_hit\s*;", text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            fields.append((m.group(1), ctype, int(m.group(2) or 1)))
    return fields


def test_hit_struct_layout_matches_header(R):
    fields = header_hit_fields()
    assert [f[0] for f in fields] == ["object", "inside", "t", "u", "v", "point", "eyev", "normalv", "over_point",
                                      "under_point", "reflectv", "n1", "n2"]
    size = {"int32_t": 4, "double": 8}
    off, want = 0, {}
    for name, ctype, count in fields:  # natural alignment, as the C compiler lays the struct out
        off = (off + size[ctype] - 1) // size[ctype] * size[ctype]
        want[name] = off
        off += size[ctype] * count
    assert off == 192
    Hit = R._lib.Hit
    assert C.sizeof(Hit) == 192
    assert [n for n, _ in Hit._fields_] == [f[0] for f in fields]
    assert {n: getattr(Hit, n).offset for n, _ in Hit._fields_} == want
    dt = R._lib.hit_dtype()
    assert dt.itemsize == 192
    assert {n: dt.fields[n][1] for n in dt.names} == want
    assert dt["object"] == np.int32 and dt["t"] == np.float64 and dt["point"].shape == (3,)


def test_abi_version_and_exports(R):
    assert R.lib().rr_abi_version() == 11
    for name in ("rr_hit_at", "rr_render_aov", "rr_render_aov_device"):
        assert name in R._lib.EXPORTS and hasattr(R.lib(), name)
    hdr = open(HEADER).read()
    for name, value in (("RR_AOV_DEPTH", 1), ("RR_AOV_NORMAL", 2), ("RR_AOV_OBJECT", 4), ("RR_AOV_ALBEDO", 8)):
        assert int(re.search(rf"#define {name}\s+(\d+)", hdr).group(1)) == value == getattr(R._lib, name)


def test_null_arguments_are_refused_without_a_device(R):
    L, E = R.lib(), R._lib.RR_E_ARG
    o, d = np.zeros(3), np.array([0.0, 0.0, 1.0])
    out = np.zeros(1, R._lib.hit_dtype())
    D, Hp = R._lib._D, C.POINTER(R._lib.Hit)
    assert L.rr_hit_at(None, 1, o.ctypes.data_as(D), d.ctypes.data_as(D), out.ctypes.data_as(Hp)) == E
    assert L.rr_hit_at(None, 1, None, None, None) == E
    assert L.rr_hit_at(None, 0, None, None, None) == E  # a null context is refused whatever n is
    cam = R.camera(8, 8, 1.0)
    opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
    depth = np.zeros((8, 8))
    assert L.rr_render_aov(None, C.byref(cam), C.byref(opts), 1, depth.ctypes.data_as(D), None, None, None, None) == E
    assert L.rr_render_aov(None, C.byref(cam), C.byref(opts), 15, None, None, None, None, None) == E
    assert L.rr_render_aov(None, None, None, 1, None, None, None, None, None) == E
    assert L.rr_render_aov_device(None, C.byref(cam), C.byref(opts), 1, None, None, None, None, None) == E
    assert "null" in L.rr_last_error().decode()


def test_python_wrappers_exist(R):
    for name in ("hit_at", "render_aov", "render_aov_device"):
        assert callable(getattr(R.Renderer, name))
    with pytest.raises(ValueError):
        R.Renderer._aov_mask(("depth", "colour"))
    assert R.Renderer._aov_mask(("depth", "object")) == 5


def test_documents_name_the_new_entry_points():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("rr_hit_at", "rr_render_aov", "rr_render_aov_device"):
        assert re.search(rf"\bfn {name}\s*\(", integ), name
    assert re.search(r"#\[repr\(C\)\]\s*(?:#\[[^\]]*\]\s*)*pub struct rr_hit\b", integ)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "render_aov" in readme and "hit_at" in readme and "--aov" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "hit_kernel" in design
