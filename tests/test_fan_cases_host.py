"""Host side of the fan fuzz (tests/test_gpu_fan_fuzz.py): on the oracle alone, the conditions that keep its comparison
from passing vacuously over fan_cases.SCENES (72 scenes).  Everything is computed from the oracle and printed; the
bounds are conditions, not measurements.

  (i)    every scene yields at least 32 distinct hit points of the 33 x 17 query camera
  (ii)   per scene, over the K = 16 `spread` batteries at 0.3 S and 3 S together, at least 2 % of the pairs are occluded
         and at least 2 % free.  A scene that misses this is tried on its `inside` battery (K = 16, 0.3 S), whose segments
         start under the surface; a scene that misses there too is named in ONE_ANSWER with the reason (at most 6)
  (iii)  each builder has at least four scenes with >= 10 % occluded and >= 10 % free at 0.3 S (`spread`, K = 16); a
         builder that cannot is named in FEW_MIXED with the reason
  (iv)   the 1e-6 S battery holds occluded pairs in at least two scenes (points inside their own sphere by the
         reference's rounding: the occluder is at t ~ 0 of a segment of any length); the 1e39 battery answers both ways
         in at least 40 scenes
  (v)    at most 5 % of a scene's points are replaced for a NaN t, and no battery is one repeated point
  (vi)   `inside`: at least 90 % of the pairs of the points under a closed leaf's surface are occluded, in at least 20
         scenes (planes have no inside; the two special records are not counted)
  (vii)  indirect: per scene at least 25 % of the rays hit something, or the scene is named in OPEN_SKY with the reason;
         across scenes the expected colours are not all equal; for remaining = 2 at least 30 scenes have a ray whose
         colour differs from its remaining = 0 colour
  (viii) every scene's materials share one shininess: the indirect comparison's exactness rests on it
  (ix)   G = 0, 1 and 2 (flat, groups, general) each serve at least 10 scenes"""
import functools

import numpy as np
import pytest

import fan_cases as FC  # noqa: E402
import scene_fuzz as F  # noqa: E402

SCENES = pytest.mark.parametrize("name,seed", FC.SCENES, ids=FC.IDS)
# (ii): scenes whose spread and inside batteries answer one way (nearly) everywhere, with the reason.  At most 6.
ONE_ANSWER = {("build", 4): "grazing: the camera skims a floor 205 units long with spheres of 0.01 to 2 units hundreds of "
                           "units apart: no pair of the spread batteries is occluded at any radius, 15 of 1024 inside"}
MAX_ONE_ANSWER = 6
# (iii): build_area's occluders are a few small spheres and cubes by the capsule rule, high between a floor and a light
# at 4 to 9 units, seen from S ~ 8.5: at 0.3 S = 2.5 units the floor's fans pass under them.  Only its wall scenes
# (seed % 4 == 1) hold something near the visible points; of the seeds 0 .. 27 only 5, 13 and 21 reach 10 %.
FEW_MIXED = {"area": "small occluders high above an open floor; only the wall scenes occlude at 0.3 S"}
# (vii): scenes whose visible points lie mostly on an open floor (or on convex shapes over one) under a black sky: most
# cosine-weighted rays leave upwards and hit nothing, and the `inside` rays under a plane leave downwards.  The misses
# are compared like the hits (a miss is black, and a cull that kept too much would make it a hit).
OPEN_SKY = (("build", 3), ("build", 4), ("build", 5), ("build", 7), ("build", 11), ("build", 12), ("build", 13), ("build", 15),
            ("general", 2), ("general", 4), ("general", 5), ("general", 8), ("general", 9), ("general", 10), ("general", 11),
            ("area", 0), ("area", 2), ("area", 3), ("area", 4), ("area", 6), ("area", 7), ("own", 1), ("own", 4), ("own", 6),
            ("own", 11), ("mix", 0), ("mix", 1), ("mix", 2), ("mix", 5), ("mix", 6), ("mix", 12), ("mix", 14), ("mix", 32))


def share(cases, sname, K, label):
    """(occluded pairs, pairs) of one battery; (0, 0) when it was left out"""
    c = next(c for c in cases if (c["set"], c["K"], c["radius_label"]) == (sname, K, label))
    return (0, 0) if c["left_out"] else (int(c["occluded"].sum()), c["occluded"].size)


@functools.lru_cache(maxsize=None)
def facts(name, seed):
    """everything the tests below read of one scene, computed once"""
    P, _, _, cat, _, size, _ = FC.scene(name, seed)
    sets, closed, hits, distinct = FC.point_sets(name, seed)
    ao = FC.ao_cases(name, seed)
    ind = FC.indirect_cases(name, seed)
    f = {"cat": cat, "size": size, "hits": hits, "distinct": distinct, "traits": F.traits(P)}
    f["by_radius"] = {r: share(ao, "spread", 16, r) for r, _ in FC.RADII}
    f["inside16"] = share(ao, "inside", 16, "0.3 S")
    c = next(c for c in ao if (c["set"], c["K"], c["radius_label"]) == ("inside", 16, "0.3 S"))
    f["closed"] = (0, 0) if c["left_out"] else (int(c["occluded"][closed].sum()), int(closed.sum()) * 16)
    f["left_out"] = sum(c["left_out"] for c in ao)
    f["ao_points"] = FC.N_POINTS * len(ao)
    f["ao_replaced"] = sum(c["replaced"] for c in ao)
    f["ao_pairs"] = sum(c["occluded"].size for c in ao if not c["left_out"])
    f["ao_occluded"] = sum(int(c["occluded"].sum()) for c in ao if not c["left_out"])
    f["one_point"] = [(c["set"], c["K"], c["radius_label"]) for c in ao
                      if not c["left_out"] and len(np.unique(c["points"], axis=0)) == 1]
    f["one_point"] += [(c["set"], c["K"], c["remaining"]) for c in ind if len(np.unique(c["points"], axis=0)) == 1]
    f["ind_points"] = FC.N_POINTS * len(ind)
    f["ind_replaced"] = sum(c["replaced"] for c in ind)
    f["ind_rays"] = sum(len(c["rays"]) for c in ind)
    f["ind_hit"] = sum(c["hit_share"] * len(c["rays"]) for c in ind) / f["ind_rays"]
    f["colours"] = np.unique(np.concatenate([c["L"] for c in ind]), axis=0)
    pairs = {}
    for c in ind:
        pairs.setdefault((c["set"], c["K"]), {})[c["remaining"]] = c
    f["deeper"] = sum(int((p[0]["L"] != p[2]["L"]).any(axis=1).sum()) for p in pairs.values()
                      if np.array_equal(p[0]["rays"], p[2]["rays"]))
    f["shininess"] = sorted(set(np.array(P.b.mats).reshape(-1, 7)[:, 3].tolist()))
    return f


def both_ways(occ, n, floor):
    return n > 0 and floor * n <= occ <= (1.0 - floor) * n


@SCENES
def test_scene_yields_points_and_both_answers(oracle_mod, name, seed):
    f = facts(name, seed)
    shares = " / ".join("left out" if n == 0 else f"{o / n:.3f}" for o, n in f["by_radius"].values())
    print(f"{name}-{seed} ({f['cat']}): S = {f['size']:.4g}, {f['hits']} hits ({f['distinct']} distinct); occluded share at "
          f"{' / '.join(r for r, _ in FC.RADII)} (spread, K = 16): {shares}; inside {f['inside16'][0]} of {f['inside16'][1]}, "
          f"under closed leaves {f['closed'][0]} of {f['closed'][1]}; {f['ao_occluded']} of {f['ao_pairs']} AO pairs occluded, "
          f"{f['left_out']} batteries left out, {f['ao_replaced']} + {f['ind_replaced']} points replaced for a NaN t; "
          f"indirect: {f['ind_rays']} rays, {f['ind_hit']:.2f} hit, {len(f['colours'])} distinct colours, {f['deeper']} rays "
          f"differ between remaining 0 and 2; shininess {f['shininess']}")
    assert f["distinct"] >= 32  # (i)
    assert f["ao_replaced"] <= 0.05 * f["ao_points"] and f["ind_replaced"] <= 0.05 * f["ind_points"]  # (v)
    assert not f["one_point"], f["one_point"]
    assert (f["ind_hit"] >= 0.25) != ((name, seed) in OPEN_SKY), f["ind_hit"]  # (vii)
    assert len(f["shininess"]) == 1  # (viii)
    # (ii)
    o = f["by_radius"]["0.3 S"][0] + f["by_radius"]["3 S"][0]
    n = f["by_radius"]["0.3 S"][1] + f["by_radius"]["3 S"][1]
    ok = both_ways(o, n, 0.02) or both_ways(*f["inside16"], 0.02)
    if (name, seed) in ONE_ANSWER:
        assert not ok, f"{name}-{seed} answers both ways: take it off ONE_ANSWER"
    else:
        assert ok, (name, seed, o, n, f["inside16"])


def test_the_named_exceptions_are_few():
    for s, why in list(ONE_ANSWER.items()) + list(FEW_MIXED.items()):
        print(f"{s}: {why}")
    print(f"open sky: {['%s-%d' % s for s in OPEN_SKY]}")
    assert all(s in FC.SCENES for s in OPEN_SKY) and 2 * len(OPEN_SKY) < len(FC.SCENES)
    assert len(ONE_ANSWER) <= MAX_ONE_ANSWER and all(s in FC.SCENES for s in ONE_ANSWER)
    assert len(FC.SCENES) == len(set(FC.SCENES)) == 69 + len(FC.MIX_GROUP_SEEDS)
    assert len(FC.AO_BATTERIES) == len(set(FC.AO_BATTERIES)) == 33 and len(FC.IND_BATTERIES) == 24


def test_every_builder_has_mixed_scenes(oracle_mod):
    for b in FC.BUILDERS:  # (iii)
        mixed = [s for s in FC.SCENES if s[0] == b and both_ways(*facts(*s)["by_radius"]["0.3 S"], 0.10)]
        print(f"{b}: {len(mixed)} of {sum(s[0] == b for s in FC.SCENES)} scenes with >= 10 % occluded and >= 10 % free at "
              f"0.3 S: {[s[1] for s in mixed]}")
        assert len(mixed) >= (1 if b in FEW_MIXED else 4), b


def test_the_shortest_and_the_longest_segments(oracle_mod):
    short = [s for s in FC.SCENES if facts(*s)["by_radius"]["1e-6 S"][0] > 0]  # (iv)
    long_ = [s for s in FC.SCENES if 0 < facts(*s)["by_radius"]["1e39"][0] < facts(*s)["by_radius"]["1e39"][1]]
    print(f"1e-6 S: occluded pairs in {len(short)} scenes: "
          f"{['%s-%d: %d' % (s + (facts(*s)['by_radius']['1e-6 S'][0],)) for s in short]}")
    print(f"1e39: both answers in {len(long_)} scenes")
    assert len(short) >= 2 and len(long_) >= 40


def test_points_under_closed_surfaces_are_occluded(oracle_mod):
    full = [s for s in FC.SCENES if facts(*s)["closed"][1] > 0 and
            facts(*s)["closed"][0] >= 0.9 * facts(*s)["closed"][1]]  # (vi)
    print(f"inside: >= 90 % of the pairs under a closed leaf occluded in {len(full)} scenes: {['%s-%d' % s for s in full]}")
    assert len(full) >= 20


def test_indirect_light_is_not_one_colour(oracle_mod):
    colours = np.unique(np.concatenate([facts(*s)["colours"] for s in FC.SCENES]), axis=0)  # (vii)
    deeper = [s for s in FC.SCENES if facts(*s)["deeper"] > 0]
    print(f"indirect: {len(colours)} distinct expected colours over all scenes; remaining 2 differs from remaining 0 in "
          f"{len(deeper)} scenes")
    assert len(colours) > 1 and len(deeper) >= 30


def test_every_walk_variant_serves_scenes(oracle_mod):
    g = [2 if t["general"] else 1 if t["groups"] else 0 for t in (facts(*s)["traits"] for s in FC.SCENES)]  # (ix)
    print(f"G = 0 / 1 / 2: {g.count(0)} / {g.count(1)} / {g.count(2)} scenes")
    assert min(g.count(0), g.count(1), g.count(2)) >= 10


def test_the_totals(oracle_mod):
    pairs = sum(facts(*s)["ao_pairs"] for s in FC.SCENES)
    occ = sum(facts(*s)["ao_occluded"] for s in FC.SCENES)
    print(f"{len(FC.SCENES)} scenes, {pairs} AO pairs, {occ} occluded ({occ / pairs:.3f}), "
          f"{sum(facts(*s)['left_out'] for s in FC.SCENES)} batteries left out, "
          f"{sum(facts(*s)['ao_replaced'] for s in FC.SCENES)} AO points and "
          f"{sum(facts(*s)['ind_replaced'] for s in FC.SCENES)} indirect points replaced for a NaN t, "
          f"{sum(facts(*s)['ind_rays'] for s in FC.SCENES)} indirect rays")
    full = FC.N_POINTS * sum(k for _, k, _ in FC.AO_BATTERIES) * len(FC.SCENES)
    assert pairs == full - FC.N_POINTS * sum(c["K"] for s in FC.SCENES for c in FC.ao_cases(*s) if c["left_out"])
