"""Times the lens frames (rr_render_lens_device) against what a caller did before them, in one process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time is
a torch event pair on the one stream everything runs on):
  c2  C2's scene at 1920 x 1080, S = 8 rays per pixel through a thin lens, remaining 5:
        a_render_lens     render_lens_device
        b_entries_mean    lens_rays_device + color_at_device over the whole frame's rays + a torch mean over the samples
        c_torch_recipe    README.md's hand-built thin lens, S times: camera_rays_device, torch.rand lens samples, five
                          elementwise torch passes, color_at_device; then a torch mean
        d_8x_aa1, d_aa3   for scale: eight aa 1 frames, and the one aa 3 frame (render_device)
  c5  C5's area-light scene at 1920 x 1080, S = 4, a pinhole with pixel jitter: a_render_lens and b_entries_mean
Before any timing (a) is compared bit for bit with (b)'s rays and colours summed in sample order (lens_resolve's order,
as S - 1 torch additions and a division: torch.mean's own order is not the definition's, so its equality is only
recorded).
--kinds recipe times c_torch_recipe alone, which the parent build (without the lens entries) can run too
(--package-root: the tree whose rray_amd package and library are used; the scenes are this tree's).  --parent FILE...:
JSON lines of such runs in the same session; the result records them and the expectation — the median of (a) below the
median of the parent build's (c).
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/lens_time.py [--frames 20] [--warmup 3] [--kinds all|recipe] [--parent a.json]
                              [--out profiles/lens/lens_time.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2 = ("c2_s1024.yaml", 1920, 1080)
C5 = ("c5_area_light.yaml", 1920, 1080)
THIN = dict(samples=8, pixel_jitter=False, aperture=0.05, focal_distance=8.0, seed=1)
JITTER = dict(samples=4, pixel_jitter=True, aperture=0.0, focal_distance=1.0, seed=1)


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
        raise SystemExit("lens_time: no HIP device (the timing needs the MI355X)")
    E = R._lib
    dev = torch.device("cuda", 0)
    full = args.kinds == "all"
    rend = R.Renderer(0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "kinds": args.kinds, "rows": {}}

    def scene_of(spec, aa=1):
        name, W, H = spec
        path = os.path.join(ROOT, "scenes", name)
        return R.YamlScene(open(path).read(), W, H, aa, obj_root=os.path.dirname(path))

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

    def row_of(spec, lens_kw, recipe, scale):
        scene = scene_of(spec)
        rend.upload(scene)
        cam = scene.camera
        W, H, S = cam.hsize, cam.vsize, lens_kw["samples"]
        n = W * H
        row = {"scene": spec[0], "width": W, "height": H, "lens": lens_kw, "rays": n * S, "remaining": 5}
        variants = {}
        with torch.cuda.stream(stream):
            img = {k: torch.zeros((n, 3), dtype=torch.float64, device=dev) for k in "abc"}
        if full:
            lens = R.Lens(**lens_kw)
            opts = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_NO_FRAME_TIMING, 0, 0)
            with torch.cuda.stream(stream):
                rays = torch.empty((n * S, 6), dtype=torch.float64, device=dev)
                rgb = torch.empty((n * S, 3), dtype=torch.float64, device=dev)

            def a():
                rend.render_lens_device(cam, opts, lens, img["a"].data_ptr(), s)

            def b():
                rend.lens_rays_device(cam, lens, rays.data_ptr(), 0, n, s)
                rend.color_at_device(n * S, rays.data_ptr(), rgb.data_ptr(), remaining=5, stream=s)
                torch.mean(rgb.view(n, S, 3), dim=1, out=img["b"])

            variants.update({"a_render_lens": a, "b_entries_mean": b})
            timed(a)
            timed(b)
            with torch.cuda.stream(stream):
                c = rgb.view(n, S, 3)
                acc = c[:, 0].clone()
                for k in range(1, S):
                    acc = acc + c[:, k]
                acc = acc / float(S)
                stream.synchronize()
                row["bit_equal"] = bool(torch.equal(img["a"], acc))
                row["torch_mean_bit_equal"] = bool(torch.equal(img["a"], img["b"]))
                row["max_abs_diff_from_torch_mean"] = float((img["a"] - img["b"]).abs().max())
            if not row["bit_equal"]:
                raise SystemExit(f"lens_time: {spec[0]}: render_lens_device differs from the entries' composition")
            timed(a)
            sa = rend.last_stats()
            row["counters"] = {k: sa[k] for k in ("rays", "shadow_rays", "shade_events", "samples", "nan_rays")}
        if recipe:
            # README.md's thin lens by hand: the lens plane's axes are the camera inverse's first two columns
            Minv = np.linalg.inv(np.array(list(cam.transform)).reshape(4, 4))
            with torch.cuda.stream(stream):
                ax = torch.tensor(Minv[:3, 0], dtype=torch.float64, device=dev)
                ay = torch.tensor(Minv[:3, 1], dtype=torch.float64, device=dev)
                r1 = torch.empty((n, 6), dtype=torch.float64, device=dev)
                c1 = torch.empty((S, n, 3), dtype=torch.float64, device=dev)
            fd, apt = lens_kw["focal_distance"], lens_kw["aperture"]

            def c_recipe():
                for k in range(S):
                    rend.camera_rays_device(cam, r1.data_ptr(), s)
                    rad = torch.sqrt(torch.rand(n, dtype=torch.float64, device=dev))
                    th = torch.rand(n, dtype=torch.float64, device=dev) * (2.0 * math.pi)
                    disc = (rad * torch.cos(th))[:, None] * ax + (rad * torch.sin(th))[:, None] * ay
                    focus = r1[:, :3] + fd * r1[:, 3:]
                    r1[:, :3] += apt * disc
                    r1[:, 3:] = torch.nn.functional.normalize(focus - r1[:, :3], dim=1)
                    rend.color_at_device(n, r1.data_ptr(), c1[k].data_ptr(), remaining=5, stream=s)
                torch.mean(c1, dim=0, out=img["c"])

            variants["c_torch_recipe"] = c_recipe
        if full and scale:
            o1 = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_NO_FRAME_TIMING, 0, 0)
            o3 = E.RenderOpts(3, 5, 0, 0, 0, 1, 8, E.RR_OUT_AVG | E.RR_NO_FRAME_TIMING, 0, 0)
            cam3 = scene_of(spec, 3).camera
            with torch.cuda.stream(stream):
                d1 = torch.empty((n, 3), dtype=torch.float64, device=dev)

            def d_8x():
                for _ in range(8):
                    rend.render_device(cam, o1, None, d1.data_ptr(), s)

            variants["d_8x_aa1"] = d_8x
            variants["d_aa3"] = lambda: rend.render_device(cam3, o3, None, d1.data_ptr(), s)
        row.update(rounds(variants))
        return row

    result["rows"]["c2"] = row_of(C2, THIN, True, True)
    if full:
        result["rows"]["c5"] = row_of(C5, JITTER, False, False)
    rend.close()

    if args.parent:
        runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent]
        recipe = [r["rows"]["c2"]["c_torch_recipe"] for r in runs]
        result["parent"] = {"digests": sorted({r["digest"] for r in runs}), "runs": len(runs), "c_torch_recipe": recipe}
        if full:
            parent_median = statistics.median(p["median_ms"] for p in recipe)
            a = result["rows"]["c2"]["a_render_lens"]["median_ms"]
            result["expectation"] = {"a_median_ms": a, "parent_c_median_ms": parent_median,
                                     "holds": bool(a < parent_median), "parent_c_over_a": parent_median / a}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
