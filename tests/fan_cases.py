"""Fans on the adversarial scenes of tests/scene_fuzz.py, from the oracle alone (no GPU, no torch): the cases of
tests/test_fan_cases_host.py and tests/test_gpu_fan_fuzz.py.

A fan is K segments (ambient occlusion) or K rays (indirect light) from one origin, spread over the hemisphere around
its normal: what rr_ao_at_device, rr_render_ao, rr_indirect_at_device and rr_render_indirect put into a wave, 64 / K
origins at a time.  The composition tests (tests/test_gpu_ao.py, tests/test_gpu_indirect.py) compare those entries with
the public ray entries over the same pairs in the same order, so both sides hold the same lanes in every wave and a cull
that is wrong for such waves is wrong on both.  Here every expected value is the oracle's: Oracle.is_shadowed pair by
pair, Oracle.color_at ray by ray.

Scenes (SCENES, 72): scene_fuzz.PATH_SCENES, scene_fuzz.MIX_PATH_SCENES, ("mix", 24 .. 56 step 8), the `nodes` family at
32, 33, 64, 65, 150 and 600 flattened nodes, and three grouped scenes of the mix (MIX_GROUP_SEEDS).  Per scene, from the
oracle's first hits (t >= 0) of the 33 x 17 query camera, four sets of 64 origins (point_sets):

  spread    hits linspace(0, n - 1, 64) in row-major order (cycled when there are fewer than 64): coherent neighbours
  shuffled  a seeded permutation of spread: at K <= 16 a wave's origins are far apart while its segments stay short
  outlier   spread with its first or its last point 1e5 scene sizes away, its normal aimed at the scene
  inside    under_point and -normalv of the same hits: just inside what the camera sees; record INSIDE_ZERO is a miss's
            zero record (point 0, normal 0) and record INSIDE_DOWN has N = (0, 0, -1) exactly

Batteries (AO_BATTERIES, 33): every radius of RADII at K = 16 on spread; every K of KS at 0.3 S on every set; shuffled and
outlier at 0.02 S and 1e39 with K = 3 and 16.  S = |from - to| of the scene's camera; 1e39 is finite in f64 and +inf as
a float.  A battery one of whose segments has no length (P + radius w == P in all three components: the reference
divides by the distance) is left out and counted.  A point one of whose pairs has a NaN t in the oracle's intersection
list is replaced by the set's first point without one (the product reports RR_E_NAN where the reference panics), and
counted.  The indirect batteries (IND_BATTERIES, 24) are the four sets with K in 1, 3, 4 and remaining in 0, 2.

Everything is computed once per scene and process (functools.lru_cache) and must not be modified by its users."""
import ctypes as C
import functools
import math

import numpy as np

import scene_fuzz as F

MIX_NODE_SEEDS = (24, 32, 40, 48, 56)  # `nodes` at 33, 64, 65, 150 and 600 nodes (seeds 0 / 8 / 16: 8, 9, 32)
# Of those 69 scenes only 7 take the G = 1 walks (groups, no general shape: build-3, build-11, area-2, area-6, mix-9,
# mix-10, mix-13); three more of the mix, so that every walk variant serves at least 10 scenes: four lights (mix-33),
# pattern trees (mix-36) and glass (mix-61) over grouped spheres
MIX_GROUP_SEEDS = (33, 36, 61)
SCENES = (list(F.PATH_SCENES) + list(F.MIX_PATH_SCENES) + [("mix", s) for s in MIX_NODE_SEEDS] +
          [("mix", s) for s in MIX_GROUP_SEEDS])
IDS = [f"{b}-{s}" for b, s in SCENES]
BUILDERS = ("build", "general", "area", "own", "mix")
SETS = ("spread", "shuffled", "outlier", "inside")
N_POINTS = 64
KS = (1, 3, 16, 64, 65)  # 64 % 3 and 64 % 65 != 0: the atomic counting path, points that straddle waves
RADII = (("1e-6 S", 1e-6), ("0.02 S", 0.02), ("0.3 S", 0.3), ("3 S", 3.0), ("1e4 S", 1e4), ("1e39", None))
HUGE_RADIUS = 1e39  # finite and > 0 (what rr_ao asks); (float)1e39 is +inf
INSIDE_ZERO, INSIDE_DOWN = 5, 6
AO_BATTERIES = ([("spread", 16, r) for r, _ in RADII] +
                [(s, k, "0.3 S") for s in SETS for k in KS if (s, k) != ("spread", 16)] +
                [(s, k, r) for s in ("shuffled", "outlier") for r in ("0.02 S", "1e39") for k in (3, 16)])
IND_BATTERIES = [(s, k, rem) for s in SETS for k in (1, 3, 4) for rem in (0, 2)]
AO_FRAME = (24, 16)   # render_ao on the scene's own camera, K in AO_FRAME_KS at 0.3 S
AO_FRAME_KS = (3, 16)
IND_FRAME = (16, 12)  # render_indirect, K = 3, remaining in IND_FRAME_REMAINING
IND_FRAME_K = 3
IND_FRAME_REMAINING = (0, 2)
COUNTS = ("rays", "shadow_rays", "shade_events")
_D = C.POINTER(C.c_double)
_CAP = 8192


def key_of(name, seed):
    return SCENES.index((name, seed))


def radius_of(label, size):
    f = dict(RADII)[label]
    return HUGE_RADIUS if f is None else f * size


class Walker:
    """the oracle's queries through buffers allocated once (tens of thousands of pairs per scene)"""

    def __init__(self, o):
        self.o, self.L, self.w = o, o.L, o.w
        self.a, self.b = np.zeros(3), np.zeros(3)
        self.pa, self.pb = self.a.ctypes.data_as(_D), self.b.ctypes.data_as(_D)
        self.t, self.u, self.v = np.zeros(_CAP), np.zeros(_CAP), np.zeros(_CAP)
        self.ob = np.zeros(_CAP, np.int32)
        self.pt, self.pu, self.pv = (x.ctypes.data_as(_D) for x in (self.t, self.u, self.v))
        self.pob = self.ob.ctypes.data_as(C.POINTER(C.c_int))
        self.rgb = np.zeros(3)
        self.prgb = self.rgb.ctypes.data_as(_D)

    def list_of(self, o, d):
        """(t, object) of Oracle.intersect(o, d): views, valid until the next call"""
        self.a[:], self.b[:] = o, d
        n = self.L.orc_intersect(self.w, self.pa, self.pb, _CAP, self.pt, self.pob, self.pu, self.pv)
        assert n <= _CAP
        return self.t[:n], self.ob[:n]

    def nan_list(self, o, d):
        return bool(np.isnan(self.list_of(o, d)[0]).any())

    def segment_ray(self, p, target):
        """the ray Scene::is_shadowed walks (scene.rs:234-245): normalize(target - p), and its length"""
        v = target - p
        dist = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + 0.0)
        with np.errstate(all="ignore"):
            return v / dist, dist

    def shadowed(self, p, target):
        self.a[:], self.b[:] = p, target
        return bool(self.L.orc_is_shadowed(self.w, self.pa, self.pb))

    def color(self, o, d, remaining):
        self.a[:], self.b[:] = o, d
        self.L.orc_color_at(self.w, self.pa, self.pb, int(remaining), self.prgb)
        return self.rgb.copy()


def closed_leaf(P, oid):
    """an object with an inside: a sphere, a cube, a torus, a closed and bounded cylinder or cone, outside any CSG node
    (a difference turns insides out)"""
    import rray_amd as R

    L = R._lib
    bid = {v: k for k, v in P.ids.items()}[oid]
    b = P.b
    p = b.parent[bid]
    while p >= 0:
        if b.kind[p] == L.CSG:
            return False
        p = b.parent[p]
    if b.kind[bid] in (L.SPHERE, L.CUBE, L.TORUS):
        return True
    if b.kind[bid] in (L.CYLINDER, L.CONE):
        lo, hi, closed = b.shape[3 * bid:3 * bid + 3]
        return bool(closed) and math.isfinite(lo) and math.isfinite(hi)
    return False


def first_hits(P, ocam):
    """The oracle's first hits (t >= 0) of every ray of `ocam` in row-major order, query_batch's rule for NaN (a ray whose
    list holds a NaN t gives no point) -> dict of arrays over the W * H samples: hit (bool), nan (bool), over, under,
    normal (n, 3), object (oracle ids, -1)."""
    import oracle

    n = ocam.hsize * ocam.vsize
    out = {"hit": np.zeros(n, bool), "nan": np.zeros(n, bool), "over": np.zeros((n, 3)), "under": np.zeros((n, 3)),
           "normal": np.zeros((n, 3)), "object": np.full(n, -1, np.int64)}
    for i in range(n):
        ro, rd = oracle.Oracle.ray_for_pixel(ocam, i % ocam.hsize, i // ocam.hsize)
        xs = P.o.intersect(ro[:3], rd[:3])
        if any(math.isnan(x[0]) for x in xs):
            out["nan"][i] = True
            continue
        h = next((k for k, x in enumerate(xs) if x[0] >= 0.0), None)
        if h is None:
            continue
        c = P.o.prepare_computations(ro[:3], rd[:3], xs, h)
        out["hit"][i] = True
        out["over"][i], out["under"][i], out["normal"][i] = c["over_point"][:3], c["under_point"][:3], c["normalv"][:3]
        out["object"][i] = xs[h][1]
    return out


@functools.lru_cache(maxsize=None)
def scene(name, seed):
    """-> (Pair, camera spec, depth, category, jitter seed, S = |from - to|, Walker): built once per process"""
    P, spec, depth, cat, js = F.build_path(name, seed)
    size = float(np.linalg.norm(np.array(spec["from_"]) - np.array(spec["to"])))
    return P, spec, depth, cat, js, size, Walker(P.o)


@functools.lru_cache(maxsize=None)
def point_sets(name, seed):
    """-> ({set: (points (64, 3), normals (64, 3))}, closed (64,) bool: the inside set's records that lie in a closed
    leaf, the two special records excluded; hits; distinct hit points)"""
    P, spec, _, _, _, size, _ = scene(name, seed)
    key = key_of(name, seed)
    rng = np.random.default_rng(80_000 + key)
    _, ocam = F.cameras(P, spec, *F.QUERY_SIZE)
    h = first_hits(P, ocam)
    at = np.flatnonzero(h["hit"])
    n = len(at)
    assert n > 0, (name, seed)
    idx = at[np.linspace(0, n - 1, N_POINTS).astype(np.int64) if n >= N_POINTS else np.arange(N_POINTS) % n]
    sets = {"spread": (h["over"][idx].copy(), h["normal"][idx].copy())}
    perm = rng.permutation(N_POINTS)
    sets["shuffled"] = (sets["spread"][0][perm].copy(), sets["spread"][1][perm].copy())
    p, nn = sets["spread"][0].copy(), sets["spread"][1].copy()
    lane = 0 if key % 2 == 0 else N_POINTS - 1
    to = np.array(spec["to"])
    p[lane] = to + F._unit(rng) * 1e5 * size
    aim = to - p[lane]
    nn[lane] = aim / np.linalg.norm(aim)
    sets["outlier"] = (p, nn)
    p, nn = h["under"][idx].copy(), -h["normal"][idx]
    closed = np.array([closed_leaf(P, int(o)) for o in h["object"][idx]])
    p[INSIDE_ZERO], nn[INSIDE_ZERO] = 0.0, 0.0
    nn[INSIDE_DOWN] = (0.0, 0.0, -1.0)
    closed[[INSIDE_ZERO, INSIDE_DOWN]] = False
    sets["inside"] = (p, nn)
    distinct = len(np.unique(h["over"][at], axis=0))
    return sets, closed, n, distinct


def ao_seed(key, bi):
    return 1_000_003 * key + 97 * bi + 11


def _replace_nan_points(P0, N0, rays_of, bad_of):
    """The NaN rule: points one of whose pairs / rays has a NaN t take the place's first point without one (the point
    keeps its place, so its hash index and with it its directions are its place's: checked again).
    -> (points, normals, per-point data of rays_of, replaced)"""
    pts, nrm = P0.copy(), N0.copy()
    data = rays_of(pts, nrm)
    bad = np.array([bad_of(pts, data, i) for i in range(len(pts))])
    replaced = int(bad.sum())
    for _ in range(8):
        if not bad.any():
            return pts, nrm, data, replaced
        good = int(np.flatnonzero(~bad)[0])
        pts[bad], nrm[bad] = pts[good], nrm[good]
        data = rays_of(pts, nrm)
        bad = np.array([b and bad_of(pts, data, i) for i, b in enumerate(bad)])
    raise AssertionError("a replaced point keeps a NaN t at every place")


@functools.lru_cache(maxsize=None)
def ao_cases(name, seed):
    """The AO batteries of one scene -> list of dict(set, K, radius_label, radius, seed, points, normals, targets
    (64, K, 3), occluded (64, K) bool, replaced, left_out); a battery left out holds no targets."""
    import rray_amd as R

    P, _, _, _, _, size, W = scene(name, seed)
    sets = point_sets(name, seed)[0]
    key = key_of(name, seed)
    out = []
    for bi, (sname, K, label) in enumerate(AO_BATTERIES):
        ao = R.Ao(K, radius_of(label, size), seed=ao_seed(key, bi))
        case = {"set": sname, "K": K, "radius_label": label, "radius": ao.radius, "seed": ao.seed, "left_out": False,
                "replaced": 0}
        P0, N0 = sets[sname]
        T0 = R.ao_targets(P0, N0, ao)
        if (T0 == P0[:, None, :]).all(axis=2).any():
            case["left_out"] = True
            out.append(case)
            continue

        def bad_of(pts, T, i):
            return any(W.nan_list(pts[i], W.segment_ray(pts[i], T[i, k])[0]) for k in range(K))

        pts, nrm, T, case["replaced"] = _replace_nan_points(P0, N0, lambda p, n: R.ao_targets(p, n, ao), bad_of)
        if (T == pts[:, None, :]).all(axis=2).any():
            case["left_out"] = True
            out.append(case)
            continue
        occ = np.array([[W.shadowed(pts[i], T[i, k]) for k in range(K)] for i in range(N_POINTS)])
        case.update(points=pts, normals=nrm, targets=T, occluded=occ)
        out.append(case)
    return out


def _counts_delta(o, before):
    st = o.stats()
    return {k: st[k] - before[k] for k in ("rays", "shadow_rays", "shade_events", "nan_sorts")}


def _trace(P, W, rays, ids, remaining, js):
    """Oracle.color_at of rays[j] for j in ids with correctly rounded powers and ray j's jitter identity (sample j,
    path 1) -> (L (len(rays), 3), the counters under the product's names, nan_sorts)"""
    L = np.zeros((len(rays), 3))
    P.o.set_pow_mode(1)
    try:
        before = P.o.stats()
        for j in ids:
            P.o.set_context(js, 0, int(j))
            L[j] = W.color(rays[j, :3], rays[j, 3:], remaining)
        d = _counts_delta(P.o, before)
    finally:
        P.o.set_pow_mode(0)
        P.o.set_context(0, 0, 0)
    return L, F.oracle_counts(d), d["nan_sorts"]


@functools.lru_cache(maxsize=None)
def indirect_cases(name, seed):
    """The indirect batteries of one scene -> list of dict(set, K, remaining, seed, points, normals, rays (64 K, 6),
    L (64 K, 3), value (64, 3), counts, hit_share, replaced)"""
    import rray_amd as R

    P, _, _, _, js, _, W = scene(name, seed)
    sets = point_sets(name, seed)[0]
    key = key_of(name, seed)
    out = []
    for bi, (sname, K, rem) in enumerate(IND_BATTERIES):
        ind = R.Indirect(K, rem, seed=ao_seed(key, 100 + bi // 2))  # remaining 0 and 2 of a (set, K): the same rays
        P0, N0 = sets[sname]

        def bad_of(pts, rays, i):
            for k in range(K):
                r = rays[i * K + k]
                if not np.isfinite(r).all() or W.nan_list(r[:3], r[3:]):
                    return True
                P.o.set_context(js, 0, i * K + k)
                before = P.o.stats()["nan_sorts"]
                W.color(r[:3], r[3:], rem)
                if P.o.stats()["nan_sorts"] != before:  # a NaN list further down the ray's tree
                    return True
            return False

        pts, nrm, rays, replaced = _replace_nan_points(P0, N0, lambda p, n: R.indirect_rays(p, n, ind), bad_of)
        L, counts, nans = _trace(P, W, rays, range(len(rays)), rem, js)
        assert nans == 0
        hits = sum(bool((W.list_of(r[:3], r[3:])[0] >= 0.0).any()) for r in rays)
        out.append({"set": sname, "K": K, "remaining": rem, "seed": ind.seed, "points": pts, "normals": nrm, "rays": rays,
                    "L": L, "value": R.indirect_resolve(L, K), "counts": counts, "hit_share": hits / len(rays),
                    "replaced": replaced})
    return out


def frame_points(h):
    """points and normals of a frame's samples for the numpy mirrors: a miss takes a placeholder, its rays are dropped"""
    hit = h["hit"]
    return (np.ascontiguousarray(np.where(hit[:, None], h["over"], [0.0, 1e6, 0.0])),
            np.ascontiguousarray(np.where(hit[:, None], h["normal"], [0.0, 1.0, 0.0])))


@functools.lru_cache(maxsize=None)
def ao_frames(name, seed):
    """render_ao's expected planes on the scene's own camera at AO_FRAME, radius 0.3 S -> (hits dict, {K: dict(seed,
    radius, ao (n,), nan (n,) bool: samples compared by nan_rays only, nan_rays)})"""
    import rray_amd as R

    P, spec, _, _, _, size, W = scene(name, seed)
    key = key_of(name, seed)
    _, ocam = F.cameras(P, spec, *AO_FRAME)
    h = first_hits(P, ocam)
    pts, nrm = frame_points(h)
    frames = {}
    for K in AO_FRAME_KS:
        ao = R.Ao(K, radius_of("0.3 S", size), seed=ao_seed(key, 200 + K))
        T = R.ao_targets(pts, nrm, ao)
        want, nan, nan_rays = np.ones(len(pts)), h["nan"].copy(), int(h["nan"].sum())
        for i in np.flatnonzero(h["hit"]):
            bad = sum(W.nan_list(pts[i], W.segment_ray(pts[i], T[i, k])[0]) for k in range(K))
            if bad:
                nan[i], nan_rays = True, nan_rays + bad
                continue
            c = sum(W.shadowed(pts[i], T[i, k]) for k in range(K))
            want[i] = float(K - c) / float(K)
        frames[K] = {"seed": ao.seed, "radius": ao.radius, "ao": want, "nan": nan, "nan_rays": nan_rays}
    return h, frames


@functools.lru_cache(maxsize=None)
def indirect_frames(name, seed):
    """render_indirect's expected planes at IND_FRAME, K = IND_FRAME_K -> (hits dict, {remaining: dict(seed, value
    (n, 3), nan (n,) bool, counts: the trace's over the hits' rays, rays (n K, 6), L)})"""
    import rray_amd as R

    P, spec, _, _, js, _, W = scene(name, seed)
    key = key_of(name, seed)
    _, ocam = F.cameras(P, spec, *IND_FRAME)
    h = first_hits(P, ocam)
    pts, nrm = frame_points(h)
    K = IND_FRAME_K
    frames = {}
    for rem in IND_FRAME_REMAINING:
        ind = R.Indirect(K, rem, seed=ao_seed(key, 300))  # the same rays at either `remaining`
        rays = R.indirect_rays(pts, nrm, ind)
        ids = (np.flatnonzero(h["hit"])[:, None] * K + np.arange(K)[None, :]).reshape(-1)
        nan = h["nan"].copy()
        for j in ids:
            if W.nan_list(rays[j, :3], rays[j, 3:]):
                nan[j // K] = True
        L, counts, nans = _trace(P, W, rays, ids, rem, js)
        value = R.indirect_resolve(L, K)
        value[~h["hit"]] = 0.0
        frames[rem] = {"seed": ind.seed, "value": value, "nan": nan, "nan_sorts": nans, "counts": counts, "rays": rays,
                       "L": L}
    return h, frames


def describe_pair(P, W, p, target):
    """the oracle's intersection list of one segment, for a failure's print-out"""
    d, dist = W.segment_ray(np.asarray(p, float), np.asarray(target, float))
    t, ob = W.list_of(p, d)
    back = {v: k for k, v in P.ids.items()}
    with np.errstate(over="ignore"):
        as_float = float(np.float32(dist))
    return (f"distance {dist!r} (as float {as_float!r}), "
            f"list [{', '.join(f'(t={x!r}, object {back.get(int(o), int(o))})' for x, o in zip(t.tolist(), ob.tolist()))}]")


def describe_ray(P, W, o, d):
    t, ob = W.list_of(o, d)
    back = {v: k for k, v in P.ids.items()}
    return f"list [{', '.join(f'(t={x!r}, object {back.get(int(o_), int(o_))})' for x, o_ in zip(t.tolist(), ob.tolist()))}]"
