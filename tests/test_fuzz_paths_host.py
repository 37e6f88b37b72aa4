"""Host side of the dispatch-path fuzz (tests/test_gpu_fuzz_paths.py): on the oracle and the builder's descriptor alone,
the conditions that keep its six modes from passing vacuously over scene_fuzz.PATH_SCENES (48 scenes: the first two
seeds of every category of every builder).

  (i)   at least 40 scenes hold a reflective or transparent material (they take the chain / tree kernels and, at aa 3,
        the pixel waves); measured 46: all but the two `textures` scenes
  (ii)  at depth 0 and 32 x 24 every scene hits something with at least 10 % of its samples
  (iii) scenes with an 8 x 8 tile of 32 x 24 whose 64 first hits are one object (the hit-uniform tiles of
        shade_body.inc): measured 41, 22 of them flat; asserted at least 40 and 20
  (iv)  per scene, the query batch hits with at least 25 % of its rays and leaves out at most 1 % of them for a NaN t;
        is_shadowed answers both ways across the scenes
  (v)   the committed thresholds (tests/golden/fuzz_paths_thresholds.json) are what scene_fuzz.adaptive_threshold
        gives on the oracle's aa 1 frame, and list between 5 % and 95 % of each scene's pixels
  (vi)  every descriptor flattens (rr_scene_inspect, no device) to the oracle's inverses

The printed fractions and counts are the measured values behind the bounds.

(iv) is tightest for build-9 (far_cam): its camera sees the scene in 108 of the 33 x 17 samples (0.19; four of the eight
full tiles are empty, the fullest holds 33 hits).  With the fans on four different tiles its batch hit with 348 of 1472
rays (0.236, under the bound); the four fans now share the fullest tile in every scene (scene_fuzz.query_batch), which
is also the cleaner experiment: the same 63 rays under each outlier.  The printed fractions are the measured ones.

`python tests/test_fuzz_paths_host.py` writes the thresholds file again."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

import scene_fuzz as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = os.path.join(ROOT, "tests", "golden", "fuzz_paths_thresholds.json")
ADAPTIVE_SIZE = (14, 10)  # the adaptive mode's output frame (tests/test_gpu_fuzz_paths.py)
# scenes whose 14 x 10 frame holds one colour (area-1: a wall in front of the camera with the light behind it; own-10:
# one sphere fills the view, lit by its ambient term alone): no threshold lists a part of such a frame
ONE_COLOUR = (("area", 1), ("own", 10))
SCENES = pytest.mark.parametrize("name,seed", F.PATH_SCENES, ids=F.PATH_IDS)


@functools.lru_cache(maxsize=None)
def facts(name, seed):
    """everything the tests below read of one scene, computed once"""
    P, spec, depth, cat, js = F.build_path(name, seed)
    t = F.traits(P)
    _, ocam = F.cameras(P, spec, 32, 24)
    first = F.first_hits(P, ocam)
    uniform = [(tx, ty) for ty in range(3) for tx in range(4)
               if first[ty * 8, tx * 8] >= 0 and (first[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] == first[ty * 8, tx * 8]).all()]
    O, D, replaced = F.query_batch(P, spec, seed)
    hits = []
    for o, d in zip(O, D):
        xs = P.o.intersect(tuple(o), tuple(d))
        k = next((k for k, x in enumerate(xs) if x[0] >= 0.0), None)
        if k is not None:
            hits.append(P.o.prepare_computations(tuple(o), tuple(d), xs, k)["over_point"][:3])
    p, l = F.shadow_pairs(P, spec, seed, hits)
    shadowed = [P.o.is_shadowed(tuple(a), tuple(b)) for a, b in zip(p, l)]
    return {"cat": cat, "traits": t, "hit_fraction": float((first >= 0).mean()), "uniform_tiles": len(uniform),
            "batch": len(O), "batch_hits": len(hits), "replaced": replaced, "shadowed": int(sum(shadowed)),
            "pairs": len(shadowed), "nan_sorts": P.o.stats()["nan_sorts"]}


def threshold_of(name, seed):
    """(threshold, listed fraction) from the oracle's aa 1 frame (correctly rounded powers, the scene's own depth)"""
    P, spec, depth, cat, js = F.build_path(name, seed)
    W, H = ADAPTIVE_SIZE
    _, ocam = F.cameras(P, spec, W, H)
    canvas, _ = F.oracle_frame(P, ocam, depth, js)
    return F.adaptive_threshold(canvas) + (len(np.unique(canvas.reshape(-1, 3), axis=0)),)


def test_most_scenes_spawn_secondary_rays(oracle_mod):
    n = sum(facts(*s)["traits"]["reflective"] or facts(*s)["traits"]["transparent"] for s in F.PATH_SCENES)
    flat = sum(facts(*s)["traits"]["flat"] for s in F.PATH_SCENES)
    loop = sum(facts(*s)["traits"]["loop"] for s in F.PATH_SCENES)
    print(f"{n} of {len(F.PATH_SCENES)} scenes hold a reflective or transparent material; {flat} are flat, {loop} of "
          f"them may take the resident tile loop")
    assert len(F.PATH_SCENES) == 48 and n >= 40
    assert loop >= 10  # the resident launch's assertion is made somewhere (measured 20)


@SCENES
def test_depth0_frames_see_the_scene(oracle_mod, name, seed):
    f = facts(name, seed)
    print(f"{name}-{seed} ({f['cat']}): {f['hit_fraction']:.2f} of 32 x 24 samples hit, {f['uniform_tiles']} of 12 tiles "
          f"hit one object")
    assert f["hit_fraction"] >= 0.10


def test_hit_uniform_tiles_exist(oracle_mod):
    have = [s for s in F.PATH_SCENES if facts(*s)["uniform_tiles"] > 0]
    flat = [s for s in have if facts(*s)["traits"]["flat"]]
    print(f"{len(have)} of {len(F.PATH_SCENES)} scenes hold a tile whose 64 first hits are one object, {len(flat)} of them "
          f"flat: {['%s-%d' % s for s in flat]}")
    assert len(have) >= 40 and len(flat) >= 20  # measured 41 and 22 (the issue's floors: 20 and 4)


@SCENES
def test_query_batch_is_not_vacuous(oracle_mod, name, seed):
    f = facts(name, seed)
    frac = f["batch_hits"] / f["batch"]
    print(f"{name}-{seed} ({f['cat']}): {f['batch']} rays, {f['batch_hits']} hit ({frac:.2f}), {f['replaced']} replaced for "
          f"a NaN t, {f['shadowed']} of {f['pairs']} pairs shadowed")
    assert 1000 <= f["batch"] <= 1500 and max(F.QUERY_PREFIXES) < f["batch"]
    assert f["replaced"] <= 0.01 * f["batch"] and f["nan_sorts"] == 0
    assert frac >= 0.25, (name, seed, frac)


def test_shadow_queries_answer_both_ways(oracle_mod):
    sh = sum(facts(*s)["shadowed"] for s in F.PATH_SCENES)
    n = sum(facts(*s)["pairs"] for s in F.PATH_SCENES)
    both = sum(0 < facts(*s)["shadowed"] < facts(*s)["pairs"] for s in F.PATH_SCENES)
    print(f"{sh} of {n} pairs shadowed; {both} of {len(F.PATH_SCENES)} scenes answer both ways")
    assert 0.05 * n <= sh <= 0.95 * n and both >= 40


@SCENES
def test_adaptive_threshold_lists_part_of_the_frame(oracle_mod, name, seed):
    table = json.load(open(THRESHOLDS))
    thr, frac, colours = threshold_of(name, seed)
    print(f"{name}-{seed}: threshold {thr!r} lists {frac:.3f} of {ADAPTIVE_SIZE[0]} x {ADAPTIVE_SIZE[1]} pixels "
          f"({colours} distinct colours)")
    assert table[f"{name}-{seed}"] == thr
    if (name, seed) in ONE_COLOUR:  # adaptive_mask compares colours: one colour lists every pixel or none
        assert thr is None and colours == 1
        return
    assert thr is not None and 0.05 <= frac <= 0.95


@SCENES
def test_path_scene_builds_identically(oracle_mod, name, seed):
    import rray_amd as R

    P, spec, depth, cat, js = F.build_path(name, seed)
    desc = P.b.desc()
    n = desc.n_objects
    inv = np.zeros((n, 16))
    node = np.zeros(n, np.int32)
    R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), None,
                                          node.ctypes.data_as(R._lib._I)))
    assert (node >= 0).all()
    for bid, oid in P.ids.items():
        assert np.array_equal(inv[bid], np.array(P.o.inverse_of(oid))), (name, seed, cat, bid)


if __name__ == "__main__":
    import sys

    sys.path.insert(0, ROOT)
    out = json.load(open(THRESHOLDS))  # other lists' keys stay (mix-*: tests/test_area_mix_host.py)
    for scene in F.PATH_SCENES:
        thr, frac, colours = threshold_of(*scene)
        assert (thr is None and scene in ONE_COLOUR) or math.isfinite(thr), scene
        out["%s-%d" % scene] = thr
        print("%s-%d" % scene, repr(thr), round(frac, 3))
    with open(THRESHOLDS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
