"""Times the edge-avoiding denoiser (rr_denoise_device) against the same filter written in torch, in one
process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time is
a torch event pair on the one stream everything runs on; each variant's rounds stop at --limit seconds):
  lens  C5's area-light scene at 1920 x 1080: the S = 4 lens frame (pixel jitter) with its aa 1 first-hit planes, C = 3
  ao    C2's scene at 1920 x 1080: the K = 16 occlusion plane (radius 1) with its first-hit planes, C = 1
both with I = 5 levels and all four sigmas on (colour 0.5, normal 0.25, depth 0.05, albedo 0.1):
        a_denoise_device  denoise_device
        b_torch_filter    the same filter in torch: f64, 25 shifted slices per level
        levels            denoise_device at iterations 1..5 — level i's time is the difference of two neighbours — in
                          a context created under RRAY_DENOISE_LDS=0 (every level in the direct kernel) and, at
                          iterations 1 and 2, in one created under RRAY_DENOISE_LDS=2 (levels 0 and 1 in the LDS-tiled
                          kernel): the A/B of the two forms per level.  (a) runs in a default context, which takes the
                          faster form per level.
Before any timing (a) is compared with (b): the largest difference must be rounding noise (the torch form fuses nothing
but orders its sums as the definition does; it is not asked to be bit-equal).
--kinds torch times b_torch_filter alone, which the parent build (without the denoiser) can run too (--package-root: the
tree whose rray_amd package and library are used; the scenes are this tree's).  --parent FILE...: JSON lines of such
runs in the same session; the result records them and the expectation — the median of (a) below the median of the parent
build's (b), per row.  The result also sets (a) against the memory floor of its levels (a 24 C / 3 + 32 byte read and a
24 C / 3 byte write per pixel and level at --hbm-tbs) and against the frame it cleans (README's render_lens_device 1.05 ms
on C5, render_ao_device 4.40 ms on C2).
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/denoise_time.py [--frames 20] [--warmup 3] [--kinds all|torch] [--parent a.json]
                                 [--out profiles/denoise/denoise_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"lens": ("c5_area_light.yaml", 1920, 1080, 3, 1.05), "ao": ("c2_s1024.yaml", 1920, 1080, 1, 4.40)}
LEVELS = 5
SIGMAS = dict(sigma_color=0.5, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def torch_filter(F, z, nrm, ids, alb, levels, sc, sn, sz, sa):
    """rray_amd.denoise_filter in torch on device tensors: F (H, W, C) f64, z (H, W), nrm / alb (H, W, 3), ids (H, W)
    int32; guides rounded to f32 and widened.  25 shifted slices per level."""
    H, W, Cn = F.shape
    f32 = lambda v: v.to(torch.float32).to(torch.float64)  # noqa: E731
    z, nrm, alb = f32(z), f32(nrm), f32(alb)
    void = ~(z < float("inf")) | (ids < 0)
    zero = torch.zeros((), dtype=torch.float64, device=F.device)
    for i in range(levels):
        s = 1 << i
        sc2 = (sc / s) * (sc / s)
        acc = torch.zeros_like(F)
        ws = torch.zeros((H, W), dtype=torch.float64, device=F.device)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * s, dy * s
                if abs(ox) >= W or abs(oy) >= H:
                    continue
                P = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
                Q = (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox)))
                ok = ~void[P] & ~void[Q]
                w = torch.full(ok.shape, H5[dy + 2] * H5[dx + 2], dtype=torch.float64, device=F.device)
                Fq = F[Q]
                if dx or dy:
                    d = F[P] - Fq
                    dc = d[..., 0] * d[..., 0]
                    if Cn == 3:
                        dc = (dc + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    t = 1.0 + dc / sc2
                    ok &= t > 0.0
                    w = w * (1.0 / (t * t))
                    a, b = nrm[P], nrm[Q]
                    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
                    t = 1.0 - torch.clamp(1.0 - dot, min=0.0) / sn
                    ok &= t > 0.0
                    w = w * (t * t)
                    r = float(max(abs(dx), abs(dy)) * s)
                    t = 1.0 - torch.abs(z[P] - z[Q]) / ((sz * torch.abs(z[P])) * r)
                    ok &= t > 0.0
                    w = w * (t * t)
                    da = alb[P] - alb[Q]
                    da = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                    t = 1.0 - da / (sa * sa)
                    ok &= t > 0.0
                    w = w * (t * t)
                ok &= w > 0.0
                w = torch.where(ok, w, zero)
                acc[P] += torch.where(ok[..., None], w[..., None] * Fq, zero)
                ws[P] += w
        F = torch.where(void[..., None], F, acc / torch.where(void, 1.0, ws)[..., None])
    return F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="all", choices=("all", "torch"))
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--limit", type=float, default=60.0, help="seconds after which a variant's rounds stop")
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the copy bandwidth the memory floor is computed at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("denoise_time: no HIP device (the timing needs the MI355X)")
    E = R._lib
    dev = torch.device("cuda", 0)
    full = args.kinds == "all"
    rend = R.Renderer(0)
    rend_lds = rend_direct = None
    if full:
        os.environ["RRAY_DENOISE_LDS"] = "2"  # read at context creation
        rend_lds = R.Renderer(0)
        os.environ["RRAY_DENOISE_LDS"] = "0"
        rend_direct = R.Renderer(0)
        del os.environ["RRAY_DENOISE_LDS"]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "kinds": args.kinds,
              "levels": LEVELS, "sigmas": SIGMAS, "hbm_tbs": args.hbm_tbs, "rows": {}}

    def timed(f):
        with torch.cuda.stream(stream):
            e0.record(stream)
            f()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(variants):
        ms = {k: [] for k in variants}
        spent = {k: 0.0 for k in variants}
        for i in range(args.warmup + args.frames):
            for k, f in variants.items():
                if spent[k] > args.limit:  # the variant's own time limit: it keeps the rounds it has
                    continue
                t0 = time.monotonic()
                t = timed(f)
                spent[k] += time.monotonic() - t0
                if i >= args.warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    def row_of(key, spec):
        name, W, H, Cn, frame_ms = spec
        path = os.path.join(ROOT, "scenes", name)
        scene = R.YamlScene(open(path).read(), W, H, 1, obj_root=os.path.dirname(path))
        rend.upload(scene)
        cam = scene.camera
        n = W * H
        row = {"scene": name, "width": W, "height": H, "channels": Cn, "frame_ms_readme": frame_ms}
        opts = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, 0, 0, 0)
        with torch.cuda.stream(stream):
            img = torch.zeros((H, W, Cn), dtype=torch.float64, device=dev)
            depth = torch.zeros((H, W), dtype=torch.float64, device=dev)
            normal = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
            albedo = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
            obj = torch.zeros((H, W), dtype=torch.int32, device=dev)
            out = {k: torch.zeros((H, W, Cn), dtype=torch.float64, device=dev) for k in "ab"}
            if key == "lens":
                rend.render_lens_device(cam, opts, R.Lens(4, pixel_jitter=True, seed=1), img.data_ptr(), s)
            else:
                rend.render_ao_device(cam, opts, R.Ao(16, 1.0, seed=1), img.data_ptr(), s)
            rend.render_aov_device(cam, opts, ("depth", "normal", "object", "albedo"), depth.data_ptr(), normal.data_ptr(),
                                   obj.data_ptr(), albedo.data_ptr(), s)
        stream.synchronize()
        row["hit_share"] = float((obj >= 0).double().mean())
        variants = {}

        def b():
            out["b"] = torch_filter(img, depth, normal, obj, albedo, LEVELS, SIGMAS["sigma_color"], SIGMAS["sigma_normal"],
                                    SIGMAS["sigma_depth"], SIGMAS["sigma_albedo"])

        if full:
            def run(levels, dst, r=rend):
                r.denoise_device(R.Denoise(levels, **SIGMAS), W, H, Cn, img.data_ptr(), dst.data_ptr(),
                                    d_depth=depth.data_ptr(), d_normal=normal.data_ptr(), d_object=obj.data_ptr(),
                                    d_albedo=albedo.data_ptr(), stream=s)

            def a():
                run(LEVELS, out["a"])

            variants["a_denoise_device"] = a
            timed(a)
            timed(b)
            stream.synchronize()
            live = obj >= 0
            diff = float((out["a"] - out["b"])[live].abs().max())
            row["max_abs_a_minus_b"] = diff
            row["bit_equal_a_b"] = bool(torch.equal(out["a"], out["b"]))
            if not diff <= 1e-9:
                raise SystemExit(f"denoise_time: {key}: denoise_device differs from the torch filter by {diff}")
            before = float((img - out["a"])[live].abs().mean())
            row["mean_abs_change"] = before
            scratch = torch.zeros_like(out["a"])
            for lv in range(1, LEVELS + 1):
                variants[f"levels_1_to_{lv}"] = (lambda lv=lv: run(lv, scratch, rend_direct))
            for lv in (1, 2):
                variants[f"lds_levels_1_to_{lv}"] = (lambda lv=lv: run(lv, scratch, rend_lds))
            run(2, scratch, rend_lds)
            run(2, out["b"], rend_direct)
            stream.synchronize()
            row["lds_bit_equal_direct"] = bool(torch.equal(scratch, out["b"]))
        variants["b_torch_filter"] = b
        row.update(rounds(variants))
        if full:
            a_ms = row["a_denoise_device"]["median_ms"]
            cum = [row[f"levels_1_to_{lv}"]["median_ms"] for lv in range(1, LEVELS + 1)]
            row["level_ms"] = [cum[0]] + [cum[i] - cum[i - 1] for i in range(1, LEVELS)]  # level 0 includes the pack kernel
            lds = [row[f"lds_levels_1_to_{lv}"]["median_ms"] for lv in (1, 2)]
            row["lds_level_ms"] = [lds[0], lds[1] - lds[0]]
            per_level = n * (2 * 8 * Cn + 32)
            floor_ms = LEVELS * per_level / (args.hbm_tbs * 1e12) * 1e3
            row["bytes_per_level"] = per_level
            row["memory_floor_ms"] = floor_ms
            row["a_over_floor"] = a_ms / floor_ms
            row["a_over_frame"] = a_ms / frame_ms
            row["pixels_per_second_per_level"] = n * LEVELS / (a_ms * 1e-3)
        return row

    for key, spec in ROWS.items():
        result["rows"][key] = row_of(key, spec)
    rend.close()
    if rend_lds:
        rend_lds.close()
        rend_direct.close()

    if args.parent:
        runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent]
        result["parent"] = {"digests": sorted({r["digest"] for r in runs}), "runs": len(runs),
                            "b_torch_filter": {k: [r["rows"][k]["b_torch_filter"] for r in runs] for k in ROWS}}
        if full:
            result["expectation"] = {}
            for k in ROWS:
                parent_median = statistics.median(p["median_ms"] for p in result["parent"]["b_torch_filter"][k])
                a = result["rows"][k]["a_denoise_device"]["median_ms"]
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
