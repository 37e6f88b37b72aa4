"""The adversarial scenes of tests/scene_fuzz.py through every production dispatch path (api.cpp run_levels,
rr_render_device, rr_render_adaptive, rr_color_at, rr_is_shadowed), each path asserted from what the ABI reports.

tests/test_gpu_fuzz.py renders every seeded scene one way: a whole frame of full 8 x 8 tiles at aa 1 or 2 and the scene's
own depth, which for nearly all of them is the chain or the tree kernel.  Here scene_fuzz.PATH_SCENES (48 scenes: the first
two seeds of every category of every builder) go through six modes, compared with the oracle (correctly rounded powers,
DESIGN.md §3.2) by scene_fuzz.check_frame — the canvas bit for bit, rays / shadow_rays / shade_events equal:

  1 depth 0    max_depth 0 at 32 x 24 aa 1 and 24 x 16 aa 2 under the default switches, under RRAY_GLOBAL_CULLS=1 and
               under RRAY_PERSIST_BLOCKS=2 with RRAY_GLOBAL_CULLS=1: the fused level-0 kernels, the resident tile loop
               and the hit-uniform tiles.  Every launch is a trace_shade launch, except in transparent scenes, which
               keep the tree kernel at depth 0 (tree_levels reads the scene alone); the loop serves the scenes
               scene_fuzz.traits marks `loop` (flat, no area light, at most two lights, solid patterns) and no other
  2 aa 3       14 x 10 pixels at the scene's depth, scenes with a reflective or transparent material (46 of 48; the
               two `textures` scenes have none, so their aa 3 frames average a canvas): pixel waves.  The avg-only
               frame launches a chain kernel and no canvas average; under RRAY_NO_PW=1 the average kernel appears and
               the image is the same bit for bit
  3 ragged     29 x 19 aa 1 and 13 x 9 aa 2: no full tiles, bundles built over partial waves
  4 bands      24 x 16 aa 2 and 14 x 16 aa 3: four bands and the three parts of an interleaved frame (block_rows 2)
               equal those rows of the whole, oracle-checked frame bit for bit, and the parts' counters add up
  5 listed     render_adaptive at aa 2 and 3 on 14 x 10 pixels against the GPU's own F1 and FN frames: threshold -1
               lists every pixel (the frame is FN, the counters F1's plus FN's), and the scene's threshold of
               tests/golden/fuzz_paths_thresholds.json lists a part of them.  area-1 and own-10 have no such
               threshold: their frames hold one colour (tests/test_fuzz_paths_host.py proves it), so any threshold
               lists every pixel or none; they are rendered at threshold 0, which must list none
  6 queries    hit_at, color_at (remaining 3) and is_shadowed on scene_fuzz.query_batch / shadow_pairs (shuffled camera
               rays, scaled directions, secondary-like rays, fans with a far or reversed outlier lane), ray by ray and
               bit for bit, and on prefixes of 1, 63, 65 and 257 rays.  Both sides key an area light's jitter by the
               ray's index in the batch (Oracle.set_context per ray)

scene_fuzz.MIX_PATH_SCENES (16 scenes: the first two seeds of every family of build_area_mix — two area lights, lights
of every order, general shapes, patterns, glass, degenerate light geometry, umbrae) go through the same six modes as a
list of their own (the test_mix_* tests below), with thresholds under the keys mix-0 .. mix-15.

The kernel names of rr_kernel_times do not tell the tree kernel from the chain kernel: both count as `chain`.  The last
test prints mode x builder x (scenes, launches per kernel, loop or per-tile frames) and asserts no row is empty."""
import collections
import contextlib
import json
import os

import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import scene_fuzz as F  # noqa: E402
from test_gpu_adaptive import check_identity  # noqa: E402
from test_gpu_hit import assert_records_equal, oracle_hits, same  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = os.path.join(ROOT, "tests", "golden", "fuzz_paths_thresholds.json")
SWITCHES = ("RRAY_NO_PERSIST", "RRAY_PERSIST_BLOCKS", "RRAY_PERSIST_HEADS", "RRAY_NO_UNIFORM_HIT", "RRAY_GLOBAL_CULLS",
            "RRAY_NO_PW")
COUNTS = ("rays", "shadow_rays", "shade_events")
ADAPTIVE_COUNTS = ("rays", "shadow_rays", "shade_events", "n1n2_scans", "samples")  # tests/test_gpu_adaptive.py
SCENES = pytest.mark.parametrize("name,seed", F.PATH_SCENES, ids=F.PATH_IDS)
MODES = ("1 depth 0", "2 aa 3", "3 ragged", "4 bands", "5 listed", "6 queries")
TABLE = collections.defaultdict(lambda: {"scenes": set(), "launches": collections.Counter(), "loop": 0, "per_tile": 0})


def secondary_scenes():
    """PATH_SCENES with a reflective or transparent material, from the builder's descriptor"""
    keep = []
    for name, seed in F.PATH_SCENES:
        t = F.traits(F.build_path(name, seed)[0])
        if t["reflective"] or t["transparent"]:
            keep.append((name, seed))
    return keep


AA3_SCENES = secondary_scenes()


@pytest.fixture(scope="module")
def R():
    import rray_amd

    if rray_amd.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")
    return rray_amd


@pytest.fixture(scope="module")
def renderer(R):
    r = R.Renderer(0)
    yield r
    r.close()


@contextlib.contextmanager
def switches(**kw):
    """the launch switches set for the block (None: unset), every one restored after it (tests/test_gpu_uniform_hit.py)"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in kw.items():
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def profiled(renderer, call):
    """call() with the kernel profile on -> (its result, {kernel: launches})"""
    renderer.kernel_profile(True)
    try:
        out = call()
        kt = renderer.kernel_times()
    finally:
        renderer.kernel_profile(False)
    return out, {k: v[1] for k, v in kt.items()}


def record(mode, name, seed, launches=None, resident=None):
    row = TABLE[(mode, name)]
    row["scenes"].add(seed)
    row["launches"].update({k: v for k, v in (launches or {}).items() if v})
    if resident is not None:
        row["loop" if resident[0] > 0 else "per_tile"] += 1


def counts(st):
    return {k: st[k] for k in COUNTS}


def avg_error(got, P, canvas, aa):
    return float(np.max(np.abs(got["avg"] - P.o.aa_average(canvas, aa))))


@SCENES
def test_depth0_fused_level0(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    t = F.traits(P)
    for aa, (W, H) in ((1, (32, 24)), (2, (24, 16))):
        cam, ocam = F.cameras(P, spec, W * aa, H * aa)
        canvas_cr, st_cr = F.oracle_frame(P, ocam, 0, js)
        frames = {}
        for variant, at_upload, at_launch in (("default", {}, {}), ("global_culls", {"RRAY_GLOBAL_CULLS": "1"}, {}),
                                              ("loop", {"RRAY_GLOBAL_CULLS": "1"}, {"RRAY_PERSIST_BLOCKS": "2"})):
            what = f"{name}-{seed} ({cat}) depth 0 {W}x{H} aa{aa} {variant}"
            with switches(**at_upload):
                renderer.upload(P.b)
            with switches(**at_launch):
                got, kt = profiled(renderer, lambda: renderer.render(cam, aa=aa, max_depth=0, seed=js, canvas=True))
                resident = renderer.resident_launch()
            frames[variant] = got
            F.check_frame(got, P, what, canvas_cr, st_cr)
            assert avg_error(got, P, canvas_cr, aa) <= 1e-12, what
            # which kernels ran: one fused level; transparent scenes keep the tree kernel (counted as `chain`)
            others = {k: v for k, v in kt.items() if v and k not in ("trace_shade", "chain")}
            assert not others, (what, kt)
            if t["transparent"]:
                assert kt["chain"] >= 1 and kt["trace_shade"] == 0, (what, kt)
            else:
                assert kt["trace_shade"] >= 1 and kt["chain"] == 0, (what, kt)
            if variant == "loop":
                assert resident == ((2, 8) if t["loop"] else (0, 0)), (what, resident, t)
            record(MODES[0], name, seed, kt, resident)
        for variant, got in frames.items():
            assert np.array_equal(got["canvas"], frames["default"]["canvas"]), (name, seed, aa, variant)
            assert np.array_equal(got["avg"], frames["default"]["avg"]), (name, seed, aa, variant)
            assert counts(got["stats"]) == counts(frames["default"]["stats"]), (name, seed, aa, variant)


def test_aa3_restriction_keeps_most_scenes():
    assert len(AA3_SCENES) >= 40, len(AA3_SCENES)


@pytest.mark.parametrize("name,seed", AA3_SCENES, ids=[f"{b}-{s}" for b, s in AA3_SCENES])
def test_aa3_pixel_waves(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    W, H, aa = 14, 10, 3
    what = f"{name}-{seed} ({cat}) {W}x{H} aa{aa}"
    cam, ocam = F.cameras(P, spec, W * aa, H * aa)
    canvas_cr, st_cr = F.oracle_frame(P, ocam, depth, js)
    renderer.upload(P.b)
    with switches():
        avg_only, kt = profiled(renderer, lambda: renderer.render(cam, aa=aa, max_depth=depth, seed=js))
        assert kt["chain"] >= 1 and kt["aa"] == 0, (what, kt)  # the pixel waves average in the wave
        assert not {k: v for k, v in kt.items() if v and k != "chain"}, (what, kt)
        assert avg_error(avg_only, P, canvas_cr, aa) <= 1e-12, what
        assert counts(avg_only["stats"]) == F.oracle_counts(st_cr), what
        record(MODES[1], name, seed, kt)
        full = renderer.render(cam, aa=aa, max_depth=depth, seed=js, canvas=True)
        F.check_frame(full, P, what + " with the canvas", canvas_cr, st_cr)
        assert avg_error(full, P, canvas_cr, aa) <= 1e-12, what
    with switches(RRAY_NO_PW="1"):
        plain, kt = profiled(renderer, lambda: renderer.render(cam, aa=aa, max_depth=depth, seed=js))
    assert kt["aa"] >= 1 and kt["chain"] >= 1, (what, kt)
    assert np.array_equal(plain["avg"], avg_only["avg"]), what
    assert counts(plain["stats"]) == counts(avg_only["stats"]), what


@SCENES
def test_ragged_frames(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    renderer.upload(P.b)
    for aa, (W, H) in ((1, (29, 19)), (2, (13, 9))):
        what = f"{name}-{seed} ({cat}) {W}x{H} aa{aa}"
        cam, ocam = F.cameras(P, spec, W * aa, H * aa)
        canvas_cr, st_cr = F.oracle_frame(P, ocam, depth, js)
        got, kt = profiled(renderer, lambda: renderer.render(cam, aa=aa, max_depth=depth, seed=js, canvas=True))
        F.check_frame(got, P, what, canvas_cr, st_cr)
        assert avg_error(got, P, canvas_cr, aa) <= 1e-12, what
        assert renderer.resident_launch() == (0, 0), what  # the loop takes frames of whole tiles only
        record(MODES[2], name, seed, kt)


def sample_rows(rows, aa):
    return (np.asarray(rows)[:, None] * aa + np.arange(aa)[None, :]).reshape(-1)


@SCENES
def test_bands_and_parts(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    renderer.upload(P.b)
    for aa, (W, H) in ((2, (24, 16)), (3, (14, 16))):
        what = f"{name}-{seed} ({cat}) {W}x{H} aa{aa}"
        cam, ocam = F.cameras(P, spec, W * aa, H * aa)
        canvas_cr, st_cr = F.oracle_frame(P, ocam, depth, js)
        kw = dict(aa=aa, max_depth=depth, seed=js, canvas=True)
        whole, kt = profiled(renderer, lambda: renderer.render(cam, **kw))
        F.check_frame(whole, P, what, canvas_cr, st_cr)
        record(MODES[3], name, seed, kt)
        pieces = {}
        for band in ((0, 8), (8, 16), (2, 5), (5, 16)):
            got = renderer.render(cam, band=band, **kw)
            rows = np.arange(*band)
            assert same(got["avg"], whole["avg"][rows]), (what, band, "avg")
            assert same(got["canvas"], whole["canvas"][sample_rows(rows, aa)]), (what, band, "canvas")
            pieces[band] = got["stats"]
        covered = np.zeros(H, int)
        for p in range(3):
            got = renderer.render(cam, part=p, nparts=3, block_rows=2, **kw)
            rows = R.part_rows(H, p, 3, 2)
            covered[rows] += 1
            assert same(got["avg"], whole["avg"][rows]), (what, p, "avg")
            assert same(got["canvas"], whole["canvas"][sample_rows(rows, aa)]), (what, p, "canvas")
            pieces[p] = got["stats"]
        assert (covered == 1).all()
        for k in COUNTS:
            assert sum(pieces[p][k] for p in range(3)) == whole["stats"][k], (what, "parts", k)
            assert pieces[(0, 8)][k] + pieces[(8, 16)][k] == whole["stats"][k], (what, "bands", k)


@SCENES
def test_listed_pixels(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    thr = json.load(open(THRESHOLDS))[f"{name}-{seed}"]
    renderer.upload(P.b)
    W, H = 14, 10
    t = P.M.view_transform(spec["from_"], spec["to"], spec["up"])
    c1 = R.camera(W, H, spec["fov"], t)
    f1 = renderer.render(c1, aa=1, max_depth=depth, seed=js)
    for aa in (2, 3):
        what = f"{name}-{seed} ({cat}) {W}x{H} aa{aa}"
        cn = R.camera(W * aa, H * aa, spec["fov"], t)
        fn = renderer.render(cn, aa=aa, max_depth=depth, seed=js)
        every, kt = profiled(renderer, lambda: renderer.render_adaptive(cn, aa, -1.0, max_depth=depth, seed=js))
        record(MODES[4], name, seed, kt)
        assert same(every["avg"], fn["avg"]) and every["mask"].all() and every["n_refined"] == W * H, what
        for k in ADAPTIVE_COUNTS:  # the probe's plus the refine pass's, which is the full frame's work
            assert every["stats"][k] == f1["stats"][k] + fn["stats"][k], (what, k)
        if thr is None:  # a frame of one colour: nothing to refine at any threshold >= 0
            assert len(np.unique(f1["avg"].reshape(-1, 3), axis=0)) == 1, what
            none = renderer.render_adaptive(cn, aa, 0.0, max_depth=depth, seed=js)
            assert same(none["avg"], f1["avg"]) and not none["mask"].any() and none["n_refined"] == 0, what
            continue
        got = renderer.render_adaptive(cn, aa, thr, max_depth=depth, seed=js)
        check_identity(R, got, f1, fn, thr, what, partial=True)
        assert 0 < got["n_refined"] < W * H, what


def first_difference(got, want, o, d, what):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(len(got), -1).all(axis=1)).reshape(-1)
    for k in bad[:8]:
        print(f"{what}: ray {k} o={o[k].tolist()} d={d[k].tolist()}: gpu {got[k].tolist()} oracle {want[k].tolist()}")
    return len(bad)


@SCENES
def test_query_batches(R, renderer, name, seed):
    P, spec, depth, cat, js = F.build_path(name, seed)
    what = f"{name}-{seed} ({cat})"
    O, D, _ = F.query_batch(P, spec, seed)
    rays = list(zip(O.tolist(), D.tolist()))
    renderer.upload(P.b)
    try:
        want = oracle_hits(R, P.o, rays, {v: k for k, v in P.ids.items()})
        (got, st), kt = profiled(renderer, lambda: (renderer.hit_at(O, D), renderer.last_stats()))
        assert_records_equal(got, want, what + " hit_at")
        hits = int((want["object"] >= 0).sum())
        assert (st["rays"], st["samples"], st["n1n2_scans"]) == (len(rays), len(rays), hits), st
        assert st["nan_rays"] == 0 and P.o.stats()["nan_sorts"] == 0
        P.o.set_pow_mode(1)
        want_c = np.zeros((len(rays), 3))
        for i, (o, d) in enumerate(rays):  # an area light's jitter identity: the ray's index in the batch
            P.o.set_context(js, 0, i)
            want_c[i] = P.o.color_at(o, d, 3)
        got_c, kt_c = profiled(renderer, lambda: renderer.color_at(O, D, remaining=3, seed=js))
        record(MODES[5], name, seed, {k: kt[k] + kt_c[k] for k in kt})
        assert first_difference(got_c, want_c, O, D, what + " color_at") == 0
        assert renderer.last_stats()["nan_rays"] == 0
        p, lights = F.shadow_pairs(P, spec, seed, want["over_point"][want["object"] >= 0])
        want_s = np.array([P.o.is_shadowed(tuple(a), tuple(b)) for a, b in zip(p, lights)])
        got_s = renderer.is_shadowed(p, lights)
        bad = np.argwhere(got_s != want_s).reshape(-1)
        for k in bad[:8]:
            print(f"{what} is_shadowed: pair {k} p={p[k].tolist()} light={lights[k].tolist()}: gpu {got_s[k]} "
                  f"oracle {want_s[k]}")
        assert len(bad) == 0
        for n in F.QUERY_PREFIXES:  # a short wave, one lane less and one more than a wave, more than a block
            assert_records_equal(renderer.hit_at(O[:n], D[:n]), want[:n], f"{what} hit_at, first {n}")
            assert first_difference(renderer.color_at(O[:n], D[:n], remaining=3, seed=js), want_c[:n], O, D,
                                    f"{what} color_at, first {n}") == 0
            m = min(n, len(p))
            assert np.array_equal(renderer.is_shadowed(p[:m], lights[:m]), want_s[:m]), f"{what} is_shadowed, first {m}"
    except AssertionError:
        print("\n".join(P.log))
        raise
    finally:
        P.o.set_pow_mode(0)


# --- the area-light mix (scene_fuzz.MIX_PATH_SCENES: the first two seeds of every family of build_area_mix) through
# the same six modes: the mode functions above, scene by scene

MIX_SCENES = pytest.mark.parametrize("name,seed", F.MIX_PATH_SCENES, ids=F.MIX_PATH_IDS)


@MIX_SCENES
def test_mix_depth0_fused_level0(R, renderer, name, seed):
    test_depth0_fused_level0(R, renderer, name, seed)


@MIX_SCENES
def test_mix_aa3_pixel_waves(R, renderer, name, seed):
    t = F.traits(F.build_path(name, seed)[0])
    assert t["reflective"] or t["transparent"]  # every scene of the mix has a mirror floor
    test_aa3_pixel_waves(R, renderer, name, seed)


@MIX_SCENES
def test_mix_ragged_frames(R, renderer, name, seed):
    test_ragged_frames(R, renderer, name, seed)


@MIX_SCENES
def test_mix_bands_and_parts(R, renderer, name, seed):
    test_bands_and_parts(R, renderer, name, seed)


@MIX_SCENES
def test_mix_listed_pixels(R, renderer, name, seed):
    assert json.load(open(THRESHOLDS))[f"{name}-{seed}"] is not None  # no frame of the mix holds one colour
    test_listed_pixels(R, renderer, name, seed)


@MIX_SCENES
def test_mix_query_batches(R, renderer, name, seed):
    test_query_batches(R, renderer, name, seed)


def test_every_mode_saw_the_mix():
    """mode x the mix: every mode recorded all 16 scenes, area lights in every one"""
    for mode in MODES:
        row = TABLE.get((mode, "mix"))
        assert row is not None and len(row["scenes"]) == len(F.MIX_PATH_SCENES), (mode, row)
        print(f"{mode:<10} mix      {len(row['scenes']):>6}  " + " ".join(f"{k}={v}" for k, v in sorted(row["launches"].items())))


def test_every_mode_saw_every_builder():
    """mode x builder: scenes, launches per kernel of the profiled frames, frames served by the loop / per tile"""
    print(f"\n{'mode':<10} {'builder':<8} {'scenes':>6}  {'loop':>4} {'per-tile':>8}  launches")
    empty = []
    for mode in MODES:
        for name in F.BUILDERS:
            row = TABLE.get((mode, name))
            if row is None or not row["scenes"]:
                empty.append((mode, name))
                continue
            launches = " ".join(f"{k}={v}" for k, v in sorted(row["launches"].items()))
            print(f"{mode:<10} {name:<8} {len(row['scenes']):>6}  {row['loop']:>4} {row['per_tile']:>8}  {launches}")
    assert not empty, empty
