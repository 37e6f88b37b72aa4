"""AO and indirect fans on the adversarial scenes against the oracle itself (tests/fan_cases.py holds the cases,
tests/test_fan_cases_host.py the conditions that keep them from being vacuous).

tests/test_gpu_ao.py and tests/test_gpu_indirect.py compare the fused entries with the composition of the public ray
entries over the same pairs in the same order, so both sides put the same lanes into every wave: a mistake in anything
that depends on a wave's composition (the f32 bundle cull and its origin-ball slack, tmax = (float)distance in
shadowed_dir, the segment culls) shows identically on both sides.  Here the expected values are the oracle's, over 69
scenes with groups, meshes, CSG, cones, tori, 600 nodes, scales from 1e-3 to 1e3 and far cameras.

AO: exact integers, no tolerance and no pair set aside.  For every battery rint((1 - ao) K) equals the oracle's count for
every point and ao equals (K - c) / K bit for bit; on the same pairs is_shadowed_device answers as the oracle pair by
pair, in the batch order and in a seeded shuffle of the pairs (which tells a wrong walk from a wrong count); render_ao at
24 x 16 with K = 3 and 16 equals the plane built from the oracle's first hits, a miss 1.0, shadow_rays == K hits.
Indirect: indirect_at_device on the batteries and render_indirect at 16 x 12 (K = 3, remaining 0 and 2) equal the
oracle's values (correctly rounded powers, ray j's jitter identity sample j) bit for bit: every scene's materials share
one shininess (asserted on the host).  rays, shadow_rays and shade_events equal the oracle's as
scene_fuzz.oracle_counts maps them; nan_rays is what the oracle's NaN lists say (samples with a NaN list are compared by
it only); n1n2_scans has no counterpart in the oracle: it equals the frame's hits (plus the trace's container walks in
transparent scenes) and is 0 for the points of a scene without transparency.

Two contexts run every scene: the default one, and one that uploads under RRAY_GLOBAL_CULLS=1 (api.cpp reads it when a
scene is uploaded), which reaches both LC instantiations of the kernels wherever the scene is small enough for culls in
LDS.  The frames take the in-wave kernels with the device-side list of live samples; contexts under RRAY_UNFUSED /
RRAY_NO_TREE / RRAY_NO_CHAIN refuse them (tests/test_gpu_indirect.py) and are not run here.

A failure prints the scene, the battery and the first differing point with its K targets or rays: the oracle's
intersection list of each against the GPU's answer."""
import numpy as np
import pytest
import torch  # noqa: F401  loaded before the library (see tests/test_gpu_hit.py)

import fan_cases as FC  # noqa: E402
import scene_fuzz as F  # noqa: E402
import test_gpu_ao as A  # noqa: E402  ao_dev, frame_dev
import test_gpu_indirect as I  # noqa: E402  points_dev
import test_gpu_rays as Q  # noqa: E402  same, to_dev, shadow_dev, color_dev
import test_gpu_views_aov as V  # noqa: E402  the environment switch

pytestmark = pytest.mark.gpu
SCENES = pytest.mark.parametrize("name,seed", FC.SCENES, ids=FC.IDS)
same = Q.same


@pytest.fixture(scope="module")
def R():
    import rray_amd

    if rray_amd.device_count() < 1:
        pytest.fail("no HIP device visible (GPU tests must run on the MI355X box)")
    return rray_amd


@pytest.fixture(scope="module")
def contexts(R):
    """(name, renderer, environment of its uploads)"""
    with V.environment(RRAY_GLOBAL_CULLS="1"):
        g = R.Renderer(0)
    d = R.Renderer(0)
    yield (("default", d, {}), ("global_culls", g, {"RRAY_GLOBAL_CULLS": "1"}))
    d.close()
    g.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def uploaded(contexts, P):
    for cname, r, env in contexts:
        with V.environment(**env):
            r.upload(P.b)
        yield cname, r


def report_pairs(P, W, what, c, i, got_pairs):
    """the first differing point of an AO battery: its K targets, the oracle's list and answer against the GPU's"""
    print(f"{what}: point {i} P={c['points'][i].tolist()} N={c['normals'][i].tolist()} radius {c['radius']!r}")
    for k in range(c["K"]):
        mark = "" if bool(got_pairs[i, k]) == bool(c["occluded"][i, k]) else "  <-- differs"
        print(f"  k={k} target={c['targets'][i, k].tolist()}: gpu {int(got_pairs[i, k])} oracle {int(c['occluded'][i, k])}; "
              f"{FC.describe_pair(P, W, c['points'][i], c['targets'][i, k])}{mark}")


def test_every_walk_variant_serves_scenes():
    g = [2 if t["general"] else 1 if t["groups"] else 0 for t in (F.traits(FC.scene(*s)[0]) for s in FC.SCENES)]
    print(f"G = 0 / 1 / 2: {g.count(0)} / {g.count(1)} / {g.count(2)} scenes")
    assert min(g.count(0), g.count(1), g.count(2)) >= 10


@SCENES
def test_ao_fans_equal_the_oracle(R, contexts, dev, name, seed):
    P, spec, _, cat, _, size, W = FC.scene(name, seed)
    cases = FC.ao_cases(name, seed)
    hits, frames = FC.ao_frames(name, seed)
    cam = F.cameras(P, spec, *FC.AO_FRAME)[0]
    rng = np.random.default_rng(90_000 + FC.key_of(name, seed))
    try:
        for cname, r in uploaded(contexts, P):
            for c in cases:
                what = f"{name}-{seed} ({cat}) {cname} {c['set']} K={c['K']} radius {c['radius_label']}"
                if c["left_out"]:
                    continue
                K, n = c["K"], FC.N_POINTS
                ao = R.Ao(K, c["radius"], seed=c["seed"])
                want = c["occluded"].sum(axis=1).astype(np.int64)
                # the walk: is_shadowed_device over the same pairs, in the batch order and shuffled
                pp = np.repeat(c["points"], K, axis=0)
                tt = np.ascontiguousarray(c["targets"].reshape(n * K, 3))
                perm = rng.permutation(n * K)
                in_order = Q.shadow_dev(r, Q.to_dev(pp, dev), Q.to_dev(tt, dev), n * K, dev).reshape(n, K)
                shuffled = np.empty(n * K, np.int32)
                shuffled[perm] = Q.shadow_dev(r, Q.to_dev(pp[perm], dev), Q.to_dev(tt[perm], dev), n * K, dev)
                shuffled = shuffled.reshape(n, K)
                # the count
                got = A.ao_dev(r, c["points"], c["normals"], ao, dev)
                counts = np.rint((1.0 - got) * K).astype(np.int64)
                for label, pairs in (("is_shadowed_device in batch order", in_order), ("is_shadowed_device shuffled", shuffled)):
                    bad = np.flatnonzero((pairs != c["occluded"]).any(axis=1))
                    if len(bad):
                        print(f"{what}: {label}: {int((pairs != c['occluded']).sum())} pairs of {len(bad)} points differ")
                        report_pairs(P, W, what, c, int(bad[0]), pairs)
                    assert len(bad) == 0, (what, label)
                bad = np.flatnonzero(counts != want)
                if len(bad):
                    print(f"{what}: ao_at_device: {len(bad)} points differ; point {bad[0]}: gpu count {counts[bad[0]]} oracle "
                          f"{want[bad[0]]}")
                    report_pairs(P, W, what, c, int(bad[0]), in_order)
                assert len(bad) == 0, what
                assert same(got, (K - want).astype(np.float64) / float(K)), what  # (K - c) / K bit for bit
            for K, f in frames.items():
                what = f"{name}-{seed} ({cat}) {cname} render_ao {FC.AO_FRAME} K={K}"
                ao = R.Ao(K, f["radius"], seed=f["seed"])
                if f["nan_rays"] == 0:
                    res = r.render_ao(cam, ao)
                    plane, st = res["ao"].reshape(-1), res["stats"]
                else:  # the host entry returns RR_E_NAN after writing; the device entry reports through the stats
                    plane = A.frame_dev(R, r, cam, ao, dev).reshape(-1)
                    st = r.last_stats()
                keep = ~f["nan"]
                bad = np.flatnonzero(keep & (plane != f["ao"]))
                if len(bad):
                    i = int(bad[0])
                    print(f"{what}: {len(bad)} samples differ; sample {i} ({i % cam.hsize}, {i // cam.hsize}): gpu {plane[i]!r} "
                          f"oracle {f['ao'][i]!r}, oracle hit {bool(hits['hit'][i])} over_point {hits['over'][i].tolist()} "
                          f"normalv {hits['normal'][i].tolist()}")
                    if hits["hit"][i]:
                        T = R.ao_targets(hits["over"][i:i + 1], hits["normal"][i:i + 1], ao, first=i)[0]
                        for k in range(K):
                            print(f"  k={k} target={T[k].tolist()}: oracle {int(W.shadowed(hits['over'][i], T[k]))}; "
                                  f"{FC.describe_pair(P, W, hits['over'][i], T[k])}")
                assert len(bad) == 0, what
                assert (plane[keep & ~hits["hit"]] == 1.0).all(), what
                assert st["nan_rays"] == f["nan_rays"], (what, st)
                assert st["samples"] == st["rays"] == len(plane) and st["shade_events"] == 0, (what, st)
                if f["nan_rays"] == 0:
                    assert st["shadow_rays"] == K * int(hits["hit"].sum()), (what, st)
    except AssertionError:
        print("\n".join(P.log))
        raise


def report_rays(R, P, W, r, dev, what, rays, L, K, i, remaining, js):
    """the first differing point of an indirect battery or frame: its K rays, the oracle's list and colour against what
    color_at_device answers for the whole batch's rays"""
    got = Q.color_dev(r, Q.to_dev(rays, dev), len(rays), dev, remaining=remaining, seed=js)
    for k in range(K):
        j = i * K + k
        mark = "" if np.array_equal(got[j], L[j]) else "  <-- differs"
        print(f"  {what}: ray {j} o={rays[j, :3].tolist()} d={rays[j, 3:].tolist()}: color_at_device {got[j].tolist()} oracle "
              f"{L[j].tolist()}; {FC.describe_ray(P, W, rays[j, :3], rays[j, 3:])}{mark}")


@SCENES
def test_indirect_fans_equal_the_oracle(R, contexts, dev, name, seed):
    P, spec, _, cat, js, size, W = FC.scene(name, seed)
    cases = FC.indirect_cases(name, seed)
    hits, frames = FC.indirect_frames(name, seed)
    cam = F.cameras(P, spec, *FC.IND_FRAME)[0]
    transparent = F.traits(P)["transparent"]
    n_hits = int(hits["hit"].sum())
    try:
        for cname, r in uploaded(contexts, P):
            for c in cases:
                what = f"{name}-{seed} ({cat}) {cname} {c['set']} K={c['K']} remaining {c['remaining']}"
                ind = R.Indirect(c["K"], c["remaining"], seed=c["seed"])
                got = I.points_dev(r, c["points"], c["normals"], ind, dev, seed=js)
                st = r.last_stats()
                bad = np.flatnonzero((got != c["value"]).any(axis=1))
                if len(bad):
                    i = int(bad[0])
                    print(f"{what}: {len(bad)} points differ; point {i} P={c['points'][i].tolist()} N={c['normals'][i].tolist()}: "
                          f"gpu {got[i].tolist()} oracle {c['value'][i].tolist()}")
                    report_rays(R, P, W, r, dev, what, c["rays"], c["L"], c["K"], i, c["remaining"], js)
                assert len(bad) == 0 and np.array_equal(got, c["value"]), what
                assert {k: st[k] for k in FC.COUNTS} == c["counts"], (what, st, c["counts"])
                assert st["nan_rays"] == 0 and st["samples"] == FC.N_POINTS, (what, st)
                assert st["n1n2_scans"] == 0 or transparent, (what, st)
            for rem, f in frames.items():
                what = f"{name}-{seed} ({cat}) {cname} render_indirect {FC.IND_FRAME} K={FC.IND_FRAME_K} remaining {rem}"
                ind = R.Indirect(FC.IND_FRAME_K, rem, seed=f["seed"])
                nans = int(f["nan"].sum()) + f["nan_sorts"]
                if nans == 0:
                    res = r.render_indirect(cam, ind, seed=js)
                    plane, st = res["indirect"].reshape(-1, 3), res["stats"]
                else:  # the host entry returns RR_E_NAN after writing; the device entry reports through the stats
                    plane = I.frame_dev(R, r, cam, ind, dev, seed=js).reshape(-1, 3)
                    st = r.last_stats()
                keep = ~f["nan"]
                bad = np.flatnonzero(keep & (plane != f["value"]).any(axis=1))
                if len(bad):
                    i = int(bad[0])
                    print(f"{what}: {len(bad)} samples differ; sample {i} ({i % cam.hsize}, {i // cam.hsize}): gpu "
                          f"{plane[i].tolist()} oracle {f['value'][i].tolist()}, oracle hit {bool(hits['hit'][i])} over_point "
                          f"{hits['over'][i].tolist()} normalv {hits['normal'][i].tolist()}")
                    report_rays(R, P, W, r, dev, what, f["rays"], f["L"], FC.IND_FRAME_K, i, rem, js)
                assert len(bad) == 0, what
                assert (plane[keep & ~hits["hit"]] == 0.0).all(), what
                assert st["samples"] == len(plane), (what, st)
                if nans == 0:
                    want = dict(f["counts"], rays=f["counts"]["rays"] + len(plane))  # the camera's rays and the trace's
                    assert {k: st[k] for k in FC.COUNTS} == want, (what, st, want)
                    assert st["nan_rays"] == 0, (what, st)
                    assert st["n1n2_scans"] == n_hits or (transparent and st["n1n2_scans"] >= n_hits), (what, st)
                else:
                    assert st["nan_rays"] > 0, (what, st)
    except AssertionError:
        print("\n".join(P.log))
        raise
