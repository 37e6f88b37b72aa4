"""Host side of the area-light mix fuzz (scene_fuzz.build_area_mix, tests/test_gpu_fuzz.py
test_area_mix_fuzz_bit_exact and the tests after it), on the oracle and the builder's descriptor alone:

  (i)   every one of the 64 scenes flattens (rr_scene_inspect, no device) to the oracle's inverses and group boxes, the
        oracle renders it to finite values, and the `nodes` family flattens to exactly 8, 9, 32, 33, 64, 65, 150 and
        600 nodes (1 + the largest node_of_object)
  (ii)  the coverage table: the key (G, PRE, CP, family at the frame's depth, AR = 1) of every compared frame — the 64
        scenes at their depth and scene_fuzz.MIX_DEPTH0_SEEDS at depth 0 — serves all 36 keys G x PRE x CP x {Level0,
        Chain, Tree}; the `lights` family holds area + area, area + point and point + area.  The table is committed as
        profiles/area_mix/keys.txt (`python tests/test_area_mix_host.py` writes it again)
  (iii) the scenes are not vacuous.  Per family, over its eight scenes, for every first-hit sample of the 16 x 12 test
        camera and every area light, f = the share of the light's level^2 cell-centre points that Oracle.is_shadowed
        reports shadowed from the sample's over_point.  One scene is sampled: at level 181 (`levels`, seed 58) f is taken
        over the evenly spaced 64 x 64 of its 32761 cells; all of them would be 6.2 million calls from Python, 75 s for
        that one scene at the 12 us a call measured here, against 25 s for this whole file.  A penumbra thinner than a
        third of a cell row can then count as f = 0 or f = 1; levels 33 and 64 are computed in full.  At least
        10 % of the pairs are partly shadowed (0 < f < 1), at least 3 % wholly (f = 1), at least 10 % not at all
        (f = 0), and in at least 2 % the light's centre lies strictly behind the surface (the lanes whose rays are
        counted but not walked, light.rs:112-116); in `umbra` at least 5 % of the pairs are claimed by the umbra rule
        as tests/test_area_umbra.py restates it.  Black lights are kept off the lights a scene is about, and the
        `nodes` occluders' node indices are asserted (test_black_light_is_not_a_named_light,
        test_occluders_past_node_32).  Measured (partly, wholly, not, behind; pairs):

          nodes       0.47 0.11 0.42 0.11  (2089)
          lights      0.23 0.10 0.67 0.08  (3072)
          levels      0.24 0.13 0.63 0.08  (1460)
          general     0.24 0.30 0.47 0.19  (2304)
          patterns    0.19 0.14 0.67 0.12  (2464)
          glass       0.22 0.10 0.68 0.08  (2005)
          degenerate  0.21 0.27 0.52 0.15  (1656)
          umbra       0.12 0.46 0.42 0.17  (1567), 0.07 claimed by the umbra rule
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import scene_fuzz as F  # noqa: E402
from test_area_umbra import affine_of, inner_ball, umbra  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = os.path.join(ROOT, "profiles", "area_mix", "keys.txt")
CAMERA = (16, 12)
GRID = 64  # cell-centre points per side for levels above it (level 181 alone)


@functools.lru_cache(maxsize=None)
def scene(seed):
    return F.build_area_mix(seed)


@pytest.mark.parametrize("seed", F.AREA_MIX_SEEDS)
def test_area_mix_scene_builds_identically(oracle_mod, seed):
    import rray_amd as R

    P, spec, depth, cat = scene(seed)
    desc = P.b.desc()
    n = desc.n_objects
    inv, box, node = np.zeros((n, 16)), np.zeros((n, 6)), np.zeros(n, np.int32)
    R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), box.ctypes.data_as(R._lib._D),
                                          node.ctypes.data_as(R._lib._I)))
    assert (node >= 0).all()
    for bid, oid in P.ids.items():
        assert np.array_equal(inv[bid], np.array(P.o.inverse_of(oid))), (seed, cat, bid)
        if P.b.kind[bid] in (R._lib.GROUP, R._lib.CSG):
            assert np.array_equal(box[bid], np.array(P.o.group_aabb(oid))), (seed, cat, bid)
    if cat == "nodes":
        assert int(node.max()) + 1 == F.MIX_NODE_COUNTS[seed // 8], (seed, int(node.max()) + 1)
    if cat == "umbra":
        assert int(node.max()) + 1 <= 8, (seed, int(node.max()) + 1)
    W, H = F.MIX_LEVELS_SIZE if cat == "levels" else (24, 16)
    _, ocam = F.cameras(P, spec, W, H)
    canvas, st = P.o.render(ocam, max_depth=depth, seed=seed)
    assert np.isfinite(canvas).all(), (seed, cat)
    assert st["shadow_rays"] > 0, (seed, cat)
    assert len(P.log) >= n + len(P.b.light_kind)  # every object and light is described


def key_table():
    """[(seed, family, frame depth, key, light kinds)] of every compared frame"""
    rows = []
    for seed in F.AREA_MIX_SEEDS:
        P, spec, depth, cat = scene(seed)
        rows.append((seed, cat, depth, F.mix_key(P, depth), F.light_kinds(P)))
    for seed in F.MIX_DEPTH0_SEEDS:
        P, spec, depth, cat = scene(seed)
        rows.append((seed, cat, 0, F.mix_key(P, 0), F.light_kinds(P)))
    return rows


def table_text(rows):
    lines = ["seed family depth G PRE CP kernel AR lights"]
    lines += [f"{s} {cat} {d} {k[0]} {k[1]} {k[2]} {k[3]} {k[4]} {kinds}" for s, cat, d, k, kinds in rows]
    return "\n".join(lines) + "\n"


def test_coverage_table(oracle_mod):
    rows = key_table()
    served = {k for _, _, _, k, _ in rows}
    want = {(g, pre, cp, fam, 1) for g in (0, 1, 2) for pre in (0, 1) for cp in (0, 1) for fam in ("Level0", "Chain", "Tree")}
    assert len(want) == 36 and not want - served, sorted(want - served)
    # the scene's attributes are the ones its family sets for its seed
    for seed, cat, depth, key, kinds in rows[:64]:
        g, want_kinds, cp, glass = F.mix_attrs(seed)
        assert key[0] == g and key[2] == cp and (key[3] == "Tree") == bool(glass) and key[4] == 1, (seed, key)
        assert kinds == want_kinds if isinstance(want_kinds, str) else len(kinds) == want_kinds, (seed, kinds)
        assert "A" in kinds
        if cat == "lights" and len(kinds) >= 3:
            levels = {lv for lv, kd in zip(scene(seed)[0].b.light_level, kinds) if kd == "A"}
            assert kinds.count("A") >= 2 and len(levels) >= 2, (seed, kinds, levels)
        if cat == "levels":
            assert F.MIX_LEVELS[seed // 8] in scene(seed)[0].b.light_level
    # the depth-0 frames: one scene per (G, PRE, CP), none transparent
    assert sorted(k[:3] for _, _, d, k, _ in rows[64:]) == sorted((g, pre, cp) for g in (0, 1, 2) for pre in (0, 1) for cp in (0, 1))
    assert all(k[3] == "Level0" for _, _, _, k, _ in rows[64:])
    two = {kinds for _, cat, _, _, kinds in rows[:64] if cat == "lights" and len(kinds) == 2}
    assert two == {"AA", "Ap", "pA"}, two
    assert {len(kinds) for _, cat, _, _, kinds in rows[:64] if cat == "lights"} == {2, 3, 4, 5}
    assert open(KEYS).read() == table_text(rows), "profiles/area_mix/keys.txt is stale"


def test_black_lights_and_surfaces(oracle_mod):
    """every family holds an all-black light, an all-black surface and a light colour with a zero channel"""
    for fam in range(8):
        lights = np.concatenate([np.array(scene(8 * k + fam)[0].b.light).reshape(-1, 15)[:, 3:6] for k in range(8)])
        assert (lights == 0.0).all(axis=1).any(), F.AREA_MIX[fam]
        assert ((lights == 0.0).any(axis=1) & ~(lights == 0.0).all(axis=1)).any(), F.AREA_MIX[fam]
        P = scene(8 * F.MIX_BLACK_SURFACE + fam)[0]
        mats = np.array(P.b.mats).reshape(-1, 7)
        assert ((mats[:, 2] == 0.0) & (mats[:, 4] == 0.0)).any(), F.AREA_MIX[fam]


def front_samples(seed, light):
    """how many first-hit samples of the test camera have light number `light`'s centre strictly in front of the surface
    (a non-zero diffuse term under a coloured light: the lanes that walk their shadow rays)"""
    import oracle

    P, spec, depth, cat = scene(seed)
    _, ocam = F.cameras(P, spec, *CAMERA)
    centre = np.array(P.b.light[15 * light:15 * light + 3])
    n = 0
    for y in range(ocam.vsize):
        for x in range(ocam.hsize):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            xs = P.o.intersect(ro[:3], rd[:3])
            hit = next((i for i, e in enumerate(xs) if e[0] >= 0.0), None)
            if hit is not None:
                c = P.o.prepare_computations(ro[:3], rd[:3], xs, hit)
                n += float((centre - np.array(c["over_point"][:3])) @ np.array(c["normalv"][:3])) > 0.0
    return n


def test_black_light_is_not_a_named_light(oracle_mod):
    """A black light's lanes are counted and never walked (render_levels.inc: `lit` is false for all of them), so the
    family's black light must not be a light the scene is about.  It is a point light in every family but `umbra`
    (there the second, plain light above the scene); every area light of `nodes` and `degenerate` has a colour and
    first-hit samples that see it from the front, so each of them walks: both lights of the 33-node scene, the in-plane
    light and the light inside the sphere of `degenerate` k = 3."""
    import rray_amd as R

    for fam, name in enumerate(F.AREA_MIX):
        P = scene(8 * F.MIX_BLACK_LIGHT + fam)[0]
        col = np.array(P.b.light).reshape(-1, 15)[:, 3:6]
        black = [i for i in range(len(col)) if (col[i] == 0.0).all()]
        assert len(black) == 1, (name, black)
        if name != "umbra":
            assert P.b.light_kind[black[0]] == R._lib.LIGHT_POINT, name
        else:
            assert black[0] == 1 and F.light_kinds(P) == "AA"
    for name in ("nodes", "degenerate"):
        for k in range(8):
            seed = 8 * k + F.AREA_MIX.index(name)
            P = scene(seed)[0]
            col = np.array(P.b.light).reshape(-1, 15)[:, 3:6]
            for i, kd in enumerate(P.b.light_kind):
                if kd == R._lib.LIGHT_AREA:
                    assert (col[i] != 0.0).any(), (seed, i)
                    if not (name == "degenerate" and k == 6):  # the light below the floor: behind nearly every surface
                        assert front_samples(seed, i) >= 20, (seed, i, front_samples(seed, i))
    # the light inside the sphere: light 1 of degenerate k = 3, inside object 1 (the first occluder)
    P = scene(8 * 3 + F.AREA_MIX.index("degenerate"))[0]
    assert F.light_kinds(P) == "AAp"
    tr = np.array(P.b.transform[16:32]).reshape(4, 4)
    assert P.b.kind[1] == R._lib.SPHERE
    centre = np.array(P.b.light[15:18])
    assert np.linalg.norm(centre - tr[:3, 3]) < 0.5 * tr[0, 0]
    for a in (0.0, 1.0):
        for b in (0.0, 1.0):
            q = np.array(P.b.light[21:24]) + a * np.array(P.b.light[24:27]) + b * np.array(P.b.light[27:30])
            assert np.linalg.norm(q - tr[:3, 3]) < tr[0, 0]
    assert F.light_kinds(scene(8 * 3 + F.AREA_MIX.index("nodes"))[0]) == "AAp"


def test_occluders_past_node_32(oracle_mod):
    """`nodes`: the flattening orders the nodes itself (leaves in Morton order, the planes last), so where the capsule-rule
    occluders (the first 3 and the last 6 spheres added) land follows from their positions.  From 64 nodes on at least
    one of them is a node of index >= 32; in the 33-node scene nodes 31 and 32 are the two planes."""
    import rray_amd as R

    for k, total in enumerate(F.MIX_NODE_COUNTS):
        P = scene(8 * k)[0]
        desc = P.b.desc()
        node = np.zeros(desc.n_objects, np.int32)
        R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), None, None, node.ctypes.data_as(R._lib._I)))
        first = 1 + total % 2
        spheres = list(range(first, total))
        capsule = spheres[:3] + spheres[-6:]
        print(f"{total} nodes: capsule occluders at nodes {sorted(int(node[i]) for i in capsule)}")
        if total >= 64:
            assert max(node[i] for i in capsule) >= 32, total
        if total == 33:
            assert sorted(int(node[i]) for i in (0, 1)) == [31, 32]


def shares(seed):
    """-> (pairs, partly, wholly, unshadowed, behind, umbra claims) over the first-hit samples x area lights of a scene"""
    import oracle
    import rray_amd as R

    P, spec, depth, cat = scene(seed)
    _, ocam = F.cameras(P, spec, *CAMERA)
    lights = [(np.array(P.b.light[15 * i:15 * i + 15]), P.b.light_level[i]) for i, kd in enumerate(P.b.light_kind)
              if kd == R._lib.LIGHT_AREA]
    balls = []
    if cat == "umbra":
        for bid, oid in P.ids.items():
            if P.b.kind[bid] == R._lib.SPHERE:
                al, at = affine_of(P.o, oid)
                ball = inner_ball(al, at)
                if ball is not None:
                    balls.append((ball, float(np.linalg.svd(np.linalg.inv(al), compute_uv=False)[0])))
    out = np.zeros(6, np.int64)
    for y in range(ocam.vsize):
        for x in range(ocam.hsize):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            xs = P.o.intersect(ro[:3], rd[:3])
            hit = next((i for i, e in enumerate(xs) if e[0] >= 0.0), None)
            if hit is None:
                continue
            c = P.o.prepare_computations(ro[:3], rd[:3], xs, hit)
            over, nrm = np.array(c["over_point"][:3]), np.array(c["normalv"][:3])
            for l, level in lights:
                centre, corner, u, v = l[0:3], l[6:9], l[9:12], l[12:15]
                cells = np.arange(level) if level <= GRID else (np.arange(GRID) * level) // GRID
                sh = sum(P.o.is_shadowed(tuple(over), tuple(corner + u * ((a + 0.5) / level) + v * ((b + 0.5) / level)))
                         for a in cells for b in cells)
                n = len(cells) ** 2
                behind = float((centre - over) @ nrm) < 0.0
                corners = [corner, corner + u, corner + v, corner + u + v]
                claimed = not behind and any(umbra(over, ball, r_out, corners) for ball, r_out in balls)
                out += (1, 0 < sh < n, sh == n, sh == 0, behind, claimed)
    return out


@pytest.mark.parametrize("fam", range(8), ids=F.AREA_MIX)
def test_family_is_not_vacuous(oracle_mod, fam):
    tot = sum(shares(8 * k + fam) for k in range(8))
    n = int(tot[0])
    partly, wholly, none, behind, claimed = (float(x) / n for x in tot[1:])
    print(f"{F.AREA_MIX[fam]}: {n} (sample, area light) pairs: partly {partly:.2f} wholly {wholly:.2f} unshadowed {none:.2f} "
          f"behind {behind:.2f} umbra rule {claimed:.2f}")
    assert n >= 500
    assert partly >= 0.10 and wholly >= 0.03 and none >= 0.10 and behind >= 0.02, (partly, wholly, none, behind)
    if F.AREA_MIX[fam] == "umbra":
        assert claimed >= 0.05, claimed


def test_mix_thresholds_list_part_of_the_frame(oracle_mod):
    """the listed-pixel mode's thresholds of scene_fuzz.MIX_PATH_SCENES (tests/golden/fuzz_paths_thresholds.json, keys
    mix-*): what scene_fuzz.adaptive_threshold gives on the oracle's 14 x 10 aa 1 frame, listing 5 % to 95 % of it"""
    from test_fuzz_paths_host import THRESHOLDS, threshold_of

    table = json.load(open(THRESHOLDS))
    for name, seed in F.MIX_PATH_SCENES:
        thr, frac, colours = threshold_of(name, seed)
        print(f"{name}-{seed}: threshold {thr!r} lists {frac:.3f} ({colours} distinct colours)")
        assert thr is not None and table[f"{name}-{seed}"] == thr and 0.05 <= frac <= 0.95, (name, seed, thr, frac)


def test_mix_query_batches_are_not_vacuous(oracle_mod):
    """the query mode's batches hit with at least 25 % of their rays in every scene of the mix, as the other lists' do"""
    from test_fuzz_paths_host import facts

    for name, seed in F.MIX_PATH_SCENES:
        f = facts(name, seed)
        print(f"{name}-{seed} ({f['cat']}): {f['batch']} rays, {f['batch_hits']} hit, {f['replaced']} replaced, "
              f"{f['hit_fraction']:.2f} of 32 x 24 samples hit")
        assert f["batch_hits"] >= 0.25 * f["batch"] and f["replaced"] <= 0.01 * f["batch"] and f["hit_fraction"] >= 0.10


if __name__ == "__main__":
    import sys

    sys.path.insert(0, ROOT)
    from test_fuzz_paths_host import THRESHOLDS, threshold_of

    table = json.load(open(THRESHOLDS))
    for name, seed in F.MIX_PATH_SCENES:
        table[f"{name}-{seed}"] = threshold_of(name, seed)[0]
    with open(THRESHOLDS, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    os.makedirs(os.path.dirname(KEYS), exist_ok=True)
    with open(KEYS, "w") as f:
        f.write(table_text(key_table()))
    print(open(KEYS).read())
