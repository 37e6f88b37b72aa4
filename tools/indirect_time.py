"""Times the indirect frames (rr_render_indirect_device) against what a caller did before them, in one
process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time is
a torch event pair on the one stream everything runs on):
  c2  C2's scene at 1920 x 1080, K = 4 gathered rays per sample, remaining 1
  c5  C5's area-light scene at 1920 x 1080, K = 4
  c4  C4's teapot at 512 x 512, K = 8
        a_render_indirect  render_indirect_device
        c_torch_recipe     the hand recipe through the public entries: camera_rays_device, hit_at_device, the hits
                           sliced in torch (a boolean mask: the count visits the host), cosine-weighted directions from
                           torch.rand, color_at_device over the hits' n_hit * K materialised rays, a torch mean, a scatter
Before any timing (a) is compared bit for bit with indirect_at_device at the first hits' points (the samples that hit).
--kinds recipe times c_torch_recipe alone, which the parent build (without the indirect entries) can run too
(--package-root: the tree whose rray_amd package and library are used; the scenes are this tree's).  --parent FILE...:
JSON lines of such runs in the same session; the result records them as variant (b) and the expectation — the median of
(a) below the median of the parent build's recipe, per row.
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/indirect_time.py [--frames 20] [--warmup 3] [--kinds all|recipe] [--parent a.json]
                                  [--out profiles/indirect/indirect_time.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"c2": ("c2_s1024.yaml", 1920, 1080, 4, 1), "c5": ("c5_area_light.yaml", 1920, 1080, 4, 1),
        "c4": ("c4_teapot.yaml", 512, 512, 8, 1)}


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="all", choices=("all", "recipe"))
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("indirect_time: no HIP device (the timing needs the MI355X)")
    E = R._lib
    dev = torch.device("cuda", 0)
    full = args.kinds == "all"
    rend = R.Renderer(0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "kinds": args.kinds, "rows": {}}

    def timed(f):
        with torch.cuda.stream(stream):
            e0.record(stream)
            f()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(variants):
        ms = {k: [] for k in variants}
        for i in range(args.warmup + args.frames):
            for k, f in variants.items():
                t = timed(f)
                if i >= args.warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    def row_of(spec):
        name, W, H, K, remaining = spec
        path = os.path.join(ROOT, "scenes", name)
        scene = R.YamlScene(open(path).read(), W, H, 1, obj_root=os.path.dirname(path))
        rend.upload(scene)
        cam = scene.camera
        n = W * H
        row = {"scene": name, "width": W, "height": H, "samples": K, "remaining": remaining}
        variants = {}
        with torch.cuda.stream(stream):
            rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
            hits = torch.empty((n, 192), dtype=torch.uint8, device=dev)
            out = {k: torch.zeros((n, 3), dtype=torch.float64, device=dev) for k in "abc"}
            L = torch.empty((n * K, 3), dtype=torch.float64, device=dev)
        hd, hi = hits.view(torch.float64), hits.view(torch.int32)  # (n, 24) and (n, 48): rr_hit's words

        def first_hits():
            rend.camera_rays_device(cam, rays.data_ptr(), s)
            rend.hit_at_device(n, rays.data_ptr(), hits.data_ptr(), s)

        if full:
            ind = R.Indirect(K, remaining, seed=1)
            opts = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)

            def a():
                rend.render_indirect_device(cam, opts, ind, out["a"].data_ptr(), s)

            variants["a_render_indirect"] = a
            timed(a)
            sa = rend.last_stats()
            row["counters"] = {k: sa[k] for k in ("rays", "shadow_rays", "shade_events", "samples", "nan_rays")}
            with torch.cuda.stream(stream):  # the point query at every sample's first hit: the same identities
                first_hits()
                P, N = hd[:, 13:16].contiguous(), hd[:, 10:13].contiguous()
                rend.indirect_at_device(n, P.data_ptr(), N.data_ptr(), ind, out["b"].data_ptr(), stream=s)
                hit = hi[:, 0] >= 0
            stream.synchronize()
            row["hits"] = int(hit.sum())
            row["gathered_rays"] = row["hits"] * K
            row["max_abs_diff_to_points"] = float((out["a"][hit] - out["b"][hit]).abs().max())
            row["mean_indirect"] = float(out["a"][hit].mean())
            if not bool((out["a"][~hit] == 0).all()):
                raise SystemExit(f"indirect_time: {name}: a miss is not black")

        def c_recipe():
            first_hits()
            hit = hi[:, 0] >= 0
            P, N = hd[:, 13:16][hit], hd[:, 10:13][hit]  # the slice: n_hit visits the host
            m = P.shape[0]
            # Malley's method with torch's random numbers: a uniform disc point lifted onto the hemisphere, in a frame
            # around the normal (Duff et al.)
            rad = torch.sqrt(torch.rand((m, K), dtype=torch.float64, device=dev))
            th = torch.rand((m, K), dtype=torch.float64, device=dev) * (2.0 * math.pi)
            A, B = rad * torch.cos(th), rad * torch.sin(th)
            c = torch.sqrt(torch.clamp(1.0 - rad * rad, min=0.0))
            sg = torch.copysign(torch.ones_like(N[:, 2]), N[:, 2])
            q = -1.0 / (sg + N[:, 2])
            bb = N[:, 0] * N[:, 1] * q
            T = torch.stack([1.0 + sg * N[:, 0] * N[:, 0] * q, sg * bb, -sg * N[:, 0]], dim=1)
            Bv = torch.stack([bb, sg + N[:, 1] * N[:, 1] * q, -N[:, 1]], dim=1)
            w = A[:, :, None] * T[:, None, :] + B[:, :, None] * Bv[:, None, :] + c[:, :, None] * N[:, None, :]
            gathered = torch.cat([P[:, None, :].expand(m, K, 3), w], dim=2).reshape(m * K, 6).contiguous()
            if m:
                rend.color_at_device(m * K, gathered.data_ptr(), L.data_ptr(), remaining=remaining, stream=s)
            out["c"].zero_()
            out["c"][hit] = L[:m * K].view(m, K, 3).mean(dim=1)

        variants["c_torch_recipe"] = c_recipe
        row.update(rounds(variants))
        if full:
            row["gathered_rays_per_second"] = row["gathered_rays"] / (row["a_render_indirect"]["median_ms"] * 1e-3)
            row["mean_indirect_recipe"] = float(out["c"][hi[:, 0] >= 0].mean())
        return row

    for key, spec in ROWS.items():
        result["rows"][key] = row_of(spec)
    rend.close()

    if args.parent:
        runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent]
        result["parent"] = {"digests": sorted({r["digest"] for r in runs}), "runs": len(runs),
                            "b_torch_recipe_at_parent": {k: [r["rows"][k]["c_torch_recipe"] for r in runs] for k in ROWS}}
        if full:
            result["expectation"] = {}
            for k in ROWS:
                parent_median = statistics.median(p["median_ms"] for p in result["parent"]["b_torch_recipe_at_parent"][k])
                a = result["rows"][k]["a_render_indirect"]["median_ms"]
                result["expectation"][k] = {"a_median_ms": a, "parent_b_median_ms": parent_median,
                                            "holds": bool(a < parent_median), "parent_b_over_a": parent_median / a}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
