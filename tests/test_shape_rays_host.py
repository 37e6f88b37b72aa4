"""Host side of the edge-ray batteries (tests/shape_rays.py): on the oracle alone, the conditions that keep
tests/test_gpu_shape_rays.py from passing vacuously — every battery hits with at least a quarter of its rays and
has no NaN ray, the edge rays leave every entry count the shape can give, each shadow battery answers both ways,
each pattern battery returns both sub-colours — and the batteries upload: the flattening holds the oracle's inverses."""
import ctypes as C
import math

import numpy as np
import pytest

import scene_fuzz as F  # noqa: E402
import shape_rays as S  # noqa: E402


def _entries(B):
    """(hit fraction over all rays, NaN rays) from the oracle's Scene::intersect"""
    hits = nan = 0
    for o, d in zip(B.o, B.d):
        xs = B.P.o.intersect(tuple(o), tuple(d))
        nan += any(math.isnan(x[0]) for x in xs)
        hits += any(x[0] >= 0.0 for x in xs)
    return hits / len(B.o), nan


def _outside_hits(B):
    """edge rays whose first oracle hit is the featured leaf at a point outside the sphere around its box (what a cull
    sphere with a near, far or segment bound would drop), and the extra shadow pairs the oracle answers True"""
    oid = B.P.ids[B.objs[0]]
    lo, hi = np.array(B.box[0]), np.array(B.box[1])
    c0, r0 = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo) * 1.05
    far = 0
    for o, d in zip(B.edge_o, B.edge_d):
        h = next((x for x in B.P.o.intersect(tuple(o), tuple(d)) if x[0] >= 0.0), None)
        if h is None or h[1] != oid or not math.isfinite(h[0]):
            far += h is not None and h[1] == oid
            continue
        lp = np.array(B.P.o.world_to_object(oid, tuple(o + h[0] * d)))[:3]
        far += bool(np.linalg.norm(lp - c0) > r0)
    extra = [B.P.o.is_shadowed(tuple(p), tuple(l)) for p, l in zip(B.shadow_p[B.n_edge:], B.shadow_l[B.n_edge:])]
    return far, int(sum(extra))


@pytest.mark.parametrize("name", S.leaf_names() + list(S.CSG_NAMES))
def test_battery_is_not_vacuous(oracle_mod, name):
    import rray_amd as R

    B = S.build(name)
    assert B.n_edge <= 700 and len(B.o) == B.fan_start + 64 * B.n_edge
    lens = np.linalg.norm(B.edge_d, axis=1)
    assert lens.min() < 1e-2 and lens.max() > 1e2  # direction lengths over five decades
    frac, nan = _entries(B)
    print(f"{name}: {B.n_edge} edge rays, {len(B.o)} rays, hit fraction {frac:.2f}")
    assert nan == 0 and B.P.o.stats()["nan_sorts"] == 0
    assert frac >= 0.25, (name, frac)
    counts = set(S.entry_counts(B))
    kind = name.split("-")[0]
    if kind in ("cone_closed", "coneshell_closed"):
        assert {1, 2, 4} <= counts, (name, counts)
    elif kind.startswith("cone_"):
        assert {1, 2} <= counts, (name, counts)
    elif kind.startswith("torus_"):  # every placement: the same object-space rays
        # a torus that closes its hole (minor radius >= 1) has no inner rim for a ray to touch once
        want = {1, 2, 3, 4} if float(kind[6:]) < 1.0 else {1, 2, 4}
        assert want <= counts, (name, counts)
    elif kind == "cylinder":
        assert {1, 2} <= counts, (name, counts)
    if kind.startswith("cone") or kind.startswith("torusfar"):
        far, far_sh = _outside_hits(B)
        print(f"{name}: {far} first hits on the leaf outside the sphere around its box, {far_sh} shadowed pairs among "
              f"the extra ones")
        assert far >= 30 and far_sh >= 20, (name, far, far_sh)
    sh = np.array([B.P.o.is_shadowed(tuple(p), tuple(l)) for p, l in zip(B.shadow_p, B.shadow_l)])
    print(f"{name}: shadowed {sh.mean():.2f} of {len(sh)} pairs")
    assert 0.2 <= sh.mean() <= 0.8, (name, float(sh.mean()))
    # both sides hold the same scene
    desc = B.P.b.desc()
    inv = np.zeros((desc.n_objects, 16))
    R._lib.check(R.lib().rr_scene_inspect(C.byref(desc), inv.ctypes.data_as(R._lib._D), None, None))
    for bid, oid in B.P.ids.items():
        assert np.array_equal(inv[bid], np.array(B.P.o.inverse_of(oid))), (name, bid)


@pytest.mark.parametrize("name", S.PATTERN_NAMES)
def test_pattern_battery_returns_both_colours(oracle_mod, name):
    P, o, d, plane, pat = S.build_pattern(name, alone=False)
    cols = np.array([P.o.color_at(tuple(a), tuple(b), 3) for a, b in zip(o, d)])
    # noise.rs works on `as i32` lattice cells of coordinates doubled per octave: past 2^31 / 2^8 the reference's own
    # colours may be non-finite; nearer the origin every colour is finite
    near = np.abs(o[:, [0, 2]]).max(axis=1) < 2.0 ** 20
    assert near.mean() >= 0.7 and np.isfinite(cols[near]).all()
    cols = cols[np.isfinite(cols).all(axis=1)]
    if name in ("stripe", "ring", "checker", "transformed"):
        seen = {tuple(c) for c in cols.tolist()}
        assert S.A_COL in seen and S.B_COL in seen, name
    else:  # mixtures: both sub-colours weigh in somewhere (red dominant / blue dominant)
        assert (cols[:, 0] > cols[:, 2]).any() and (cols[:, 2] > cols[:, 0]).any(), name
    assert len({tuple(c) for c in cols.tolist()}) >= 2


@pytest.mark.parametrize("kind", S.TEXTURED_KINDS)
def test_textured_battery_reads_several_texels(oracle_mod, kind):
    P, o, d = S.build_textured(kind, 1)  # the 2 x 3 texture
    cols = [P.o.color_at(tuple(a), tuple(b), 3) for a, b in zip(o, d)]
    assert np.isfinite(np.array(cols)).all()
    assert len(set(cols) - {(0.0, 0.0, 0.0)}) >= 3, kind
