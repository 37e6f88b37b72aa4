"""Times the ordered ray batches (rr_ray_order_device, rr_color_at_device_ordered, rr_hit_at_device_ordered) against the
plain device entries on the same buffers, in one process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time
is the wall clock around the call plus a device synchronise, as tools/rays_time.py times color_at_device):
  colour    C2's scene, the 1920 x 1080 camera's rays under the fixed random permutation of tools/rays_time.py,
            remaining 5:
              plain              color_at_device
              ordered            color_at_device_ordered with d_perm = None (order + trace)
              ordered_given      color_at_device_ordered with a precomputed order (trace only)
              order_only         ray_order_device alone
  coherent  the same four on the rays in camera order (recorded only: what the order costs where it cannot help)
  hit       C4's scene, the 512 x 512 camera's rays, shuffled: hit_at_device against hit_at_device_ordered (d_perm None)
Before any timing the outputs are compared bit for bit: ordered = ordered_given = plain, the order is
argsort(ray_order_keys(rays), stable), the ordered records are the plain ones.
--kinds plain times the plain entries alone, which the parent build (without the ordered entries) can run too
(--package-root: the tree whose rray_amd package and library are used; the scenes are this tree's).  --parent FILE...:
JSON lines of such runs in the same session; the result records them and the issue's condition on the shuffled colour
row — the median of `ordered` below the minimum of the parent build's `plain`.
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/ray_order_time.py [--frames 20] [--warmup 3] [--kinds all|plain] [--parent a.json b.json]
                                   [--out profiles/ray_order/ray_order_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOUR = ("c2_s1024.yaml", 1920, 1080)
HIT = ("c4_teapot.yaml", 512, 512)
SHUFFLE_SEED = 20261020  # tools/rays_time.py's permutation


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="all", choices=("all", "plain"))
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("ray_order_time: no HIP device (the timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    full = args.kinds == "all"
    rend = R.Renderer(0)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "kinds": args.kinds, "rows": {}}

    def scene_of(spec):
        name, W, H = spec
        path = os.path.join(ROOT, "scenes", name)
        scene = R.YamlScene(open(path).read(), W, H, 1, obj_root=os.path.dirname(path))
        rend.upload(scene)
        return scene

    def wall(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def rounds(variants):
        ms = {k: [] for k in variants}
        for i in range(args.warmup + args.frames):
            for k, f in variants.items():
                t = wall(f)
                if i >= args.warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    def camera_rays(cam):
        n = cam.hsize * cam.vsize
        rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        rend.camera_rays_device(cam, rays.data_ptr())
        torch.cuda.synchronize()
        return rays, n

    def colour_row(rays, n, label):
        rgb = [torch.empty((n, 3), dtype=torch.float64, device=dev) for _ in range(3)]
        perm = torch.empty(n, dtype=torch.int32, device=dev)
        variants = {"plain": lambda: rend.color_at_device(n, rays.data_ptr(), rgb[0].data_ptr(), remaining=5)}
        row = {"rays": n, "remaining": 5}
        if full:
            variants.update({
                "ordered": lambda: rend.color_at_device_ordered(n, rays.data_ptr(), rgb[1].data_ptr(), remaining=5),
                "order_only": lambda: rend.ray_order_device(n, rays.data_ptr(), perm.data_ptr()),
                "ordered_given": lambda: rend.color_at_device_ordered(n, rays.data_ptr(), rgb[2].data_ptr(), perm.data_ptr(),
                                                                       remaining=5)})
        for f in variants.values():  # once, then the comparison
            wall(f)
        if full:
            want = np.argsort(R.ray_order_keys(rays.cpu().numpy()), kind="stable").astype(np.uint32)
            row["bit_equal"] = bool(torch.equal(rgb[0], rgb[1]) and torch.equal(rgb[0], rgb[2]) and
                                    np.array_equal(perm.cpu().numpy().view(np.uint32), want))
            if not row["bit_equal"]:
                raise SystemExit(f"ray_order_time: the {label} row's outputs differ")
            stats = {}
            for k in ("plain", "ordered_given"):
                wall(variants[k])
                st = rend.last_stats()
                stats[k] = {"wave_visits": list(st["wave_visits"]), "prim_tests": st["prim_tests"], "rays": st["rays"]}
            row["counters"] = stats
        row.update(rounds(variants))
        if full:
            for k in ("ordered", "ordered_given"):
                row[f"plain_over_{k}"] = row["plain"]["median_ms"] / row[k]["median_ms"]
        return row

    scene = scene_of(COLOUR)
    rays, n = camera_rays(scene.camera)
    shuffle = torch.from_numpy(np.random.default_rng(SHUFFLE_SEED).permutation(n)).to(dev)
    shuffled = rays[shuffle].contiguous()
    head = {"scene": COLOUR[0], "width": COLOUR[1], "height": COLOUR[2]}
    result["rows"]["colour"] = dict(head, **colour_row(shuffled, n, "colour"))
    result["rows"]["coherent"] = dict(head, **colour_row(rays, n, "coherent"))
    del rays, shuffled

    scene = scene_of(HIT)
    rays, n = camera_rays(scene.camera)
    shuffle = torch.from_numpy(np.random.default_rng(SHUFFLE_SEED).permutation(n)).to(dev)
    rays = rays[shuffle].contiguous()
    hits = [torch.empty((n, 192), dtype=torch.uint8, device=dev) for _ in range(2)]
    variants = {"plain": lambda: rend.hit_at_device(n, rays.data_ptr(), hits[0].data_ptr())}
    row = {"scene": HIT[0], "width": HIT[1], "height": HIT[2], "rays": n}
    if full:
        variants["ordered"] = lambda: rend.hit_at_device_ordered(n, rays.data_ptr(), hits[1].data_ptr())
        for f in variants.values():
            wall(f)
        row["bit_equal"] = bool(torch.equal(hits[0], hits[1]))
        if not row["bit_equal"]:
            raise SystemExit("ray_order_time: the ordered records differ from the plain ones")
    row.update(rounds(variants))
    if full:
        row["plain_over_ordered"] = row["plain"]["median_ms"] / row["ordered"]["median_ms"]
    result["rows"]["hit"] = row
    rend.close()

    if args.parent:
        runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent]
        plain = [r["rows"]["colour"]["plain"] for r in runs]
        result["parent"] = {"digests": sorted({r["digest"] for r in runs}), "runs": len(runs),
                            "colour_plain": plain, "coherent_plain": [r["rows"]["coherent"]["plain"] for r in runs],
                            "hit_plain": [r["rows"]["hit"]["plain"] for r in runs]}
        if full:
            parent_min = min(p["min_ms"] for p in plain)
            ordered = result["rows"]["colour"]["ordered"]["median_ms"]
            result["condition"] = {"ordered_median_ms": ordered, "parent_plain_min_ms": parent_min,
                                   "holds": bool(ordered < parent_min), "parent_min_over_ordered": parent_min / ordered}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
