"""Host side of the exact-cull fuzz (tests/scene_fuzz.py): every seeded adversarial scene builds the same
scene on both sides — the product's flattening (rr_scene_inspect, no device) holds the inverse the oracle
computes for every object (matrix.rs:389-412 restated twice) — and the oracle renders it to finite
values.  The GPU comparison itself is tests/test_gpu_fuzz.py."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import scene_fuzz as F  # noqa: E402

SEEDS = range(96)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_scene_builds_identically(oracle_mod, seed):
    import rray_amd as R

    P, spec, depth, cat = F.build(seed)
    desc = P.b.desc()
    n = desc.n_objects
    inv = np.zeros((n, 16))
    node = np.zeros(n, np.int32)
    R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), None,
                                          node.ctypes.data_as(R._lib._I)))
    for bid, oid in P.ids.items():
        assert np.array_equal(inv[bid], np.array(P.o.inverse_of(oid))), (seed, cat, bid)
    assert (node >= 0).all()
    t = time.perf_counter()
    cam, ocam = F.cameras(P, spec, 24, 16)
    canvas, st = P.o.render(ocam, max_depth=depth, threads=min(4, os.cpu_count() or 1))
    assert np.isfinite(canvas).all(), (seed, cat)
    assert time.perf_counter() - t < 30
    print(f"seed {seed} {cat}: {n} objects, rays {st['rays']}, shade {st['shade_events']}, "
          f"lit px {float(np.mean(canvas.sum(axis=2) > 0)):.2f}")


@pytest.mark.parametrize("seed", range(32))
def test_area_fuzz_scene_builds_identically(oracle_mod, seed):
    """The area-light fuzz scenes (scene_fuzz.build_area) hold the same inverses on both sides and render to
    finite values with some light and some shadow."""
    import rray_amd as R

    P, spec, depth, cat = F.build_area(seed)
    desc = P.b.desc()
    n = desc.n_objects
    inv = np.zeros((n, 16))
    R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), None, None))
    for bid, oid in P.ids.items():
        assert np.array_equal(inv[bid], np.array(P.o.inverse_of(oid))), (seed, cat, bid)
    cam, ocam = F.cameras(P, spec, 24, 16)
    canvas, st = P.o.render(ocam, max_depth=depth, seed=seed)
    assert np.isfinite(canvas).all(), (seed, cat)
    assert st["shadow_rays"] > 0, (seed, cat)


def _inspect(R, P):
    desc = P.b.desc()
    n = desc.n_objects
    inv, box, node = np.zeros((n, 16)), np.zeros((n, 6)), np.zeros(n, np.int32)
    rc = R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), box.ctypes.data_as(R._lib._D),
                                  node.ctypes.data_as(R._lib._I))
    return rc, inv, box, node


@pytest.mark.parametrize("seed", F.GENERAL_SEEDS)
def test_general_fuzz_scene_builds_identically(oracle_mod, seed):
    """The general-shape fuzz scenes (scene_fuzz.build_general): the same inverses on both sides, the group and CSG
    bounding boxes of the flattening equal the oracle's (group.rs:128-149, csg.rs get_aabb; one-sided cones have
    infinite boxes), the oracle renders finite values, and the family's featured kind fills at least 5 % of the frame."""
    import rray_amd as R

    P, spec, depth, cat = F.build_general(seed)
    rc, inv, box, node = _inspect(R, P)
    R._lib.check(rc)
    assert (node >= 0).all()
    for bid, oid in P.ids.items():
        assert np.array_equal(inv[bid], np.array(P.o.inverse_of(oid))), (seed, cat, bid)
        if P.b.kind[bid] in (R._lib.GROUP, R._lib.CSG):
            assert np.array_equal(box[bid], np.array(P.o.group_aabb(oid))), (seed, cat, bid, box[bid], P.o.group_aabb(oid))
    cam, ocam = F.cameras(P, spec, 24, 16)
    canvas, st = P.o.render(ocam, max_depth=depth, threads=min(4, os.cpu_count() or 1))
    assert np.isfinite(canvas).all(), (seed, cat)
    feat = {P.ids[i] for i in P.featured}
    seen = n = 0
    for y in range(16):
        for x in range(24):
            ro, rd = oracle_mod.Oracle.ray_for_pixel(ocam, x, y)
            hit = next((e for e in P.o.intersect(ro[:3], rd[:3]) if e[0] >= 0.0), None)
            seen += hit is not None and hit[1] in feat
            n += 1
    print(f"seed {seed} {cat}: {len(P.ids)} objects, featured in {seen / n:.2f} of the samples, rays {st['rays']}")
    assert seen / n >= 0.05, (seed, cat, seen / n)


@pytest.mark.parametrize("leaves,code", [(8, 0), (9, "RR_E_LIMIT")])
def test_csg_entry_limit(oracle_mod, leaves, code):
    """Eight cylinders under one CSG can leave RR_MAX_CSG_ENTRIES = 32 entries and flatten.  Leaves count two or four
    entries each, so the first subtree past the limit holds 34 (a sphere sharing a group with the last cylinder); that
    one and one of 36 (a ninth cylinder) are refused with RR_E_LIMIT."""
    import rray_amd as R

    for extra in (["cylinder"], ["sphere"]) if leaves == 9 else ([],):
        P = F.Pair()
        I = P.M.identity()
        top = P.csg("union", I)
        n = 0
        for a in range(2):
            mid = P.csg("union", I, top)
            for b in range(2):
                low = P.csg("union", I, mid)
                for c in range(2):
                    parent = low
                    if extra and n == 7:  # the last leaf shares a group with the extra one
                        parent = P.obj("group", I, parent=low)
                        if extra[0] == "sphere":
                            P.obj("sphere", I, F._material(np.random.default_rng(0)), (1, 1, 1), parent)
                        else:
                            P.cylinder(I, F._material(np.random.default_rng(0)), (1, 1, 1), -1.0, 1.0, True, parent)
                    P.cylinder(P.M.translate(0.1 * n, 0.0, 0.0), F._material(np.random.default_rng(0)), (1, 1, 1), -1.0, 1.0,
                               True, parent)
                    n += 1
        P.light((0.0, 5.0, -5.0))
        rc, _, _, _ = _inspect(R, P)
        assert rc == (0 if code == 0 else R._lib.RR_E_LIMIT), (leaves, extra, rc)
