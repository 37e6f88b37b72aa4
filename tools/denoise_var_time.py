"""Times variance-guided denoising (rr_variance_device, rr_denoise_var_device) against the plain
denoiser it is judged by and against the same filter written in torch, in one process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time is
a torch event pair on the one stream everything runs on; each variant's rounds stop at --limit seconds):
  indirect  C5's area-light scene at 1920 x 1080: the K = 4 indirect plane, C = 3
  ao        C2's scene at 1920 x 1080: the K = 16 occlusion plane (radius 1), C = 1
each with its aa 1 first-hit planes and after one rr_temporal_device step with moments (every hit has a history of 1),
I = 5 levels and the guide sigmas normal 0.25, depth 0.05, albedo 0.1:
        a_variance_history   variance_device with the moments and counts, min_history 1: the temporal branch everywhere
        b_variance_spatial   variance_device without them: the 7 x 7 window everywhere
        c_denoise_var        denoise_var_device (sigma_color 4, epsilon 1e-12, var_out given) under (b)'s plane: after one
                             frame every moment equals in * in and (a)'s plane is all zeros
        d_denoise_plain      denoise_device with the same levels and guide sigmas (sigma_color 0.5)
        e_torch_var_filter   (c)'s filter in torch: f64, 9 + 25 shifted slices per level
Before any timing (c) is compared with (e): the largest difference must be rounding noise.
--kinds plain times d_denoise_plain alone, which the parent build (without this feature) can run too (--package-root: the
tree whose rray_amd package and library are used; the scenes are this tree's).  --parent FILE...: JSON lines of such runs
in the same session; the result records them beside this build's (d) and gives (c) over the parent's (d).  No ratio is
fixed in advance.  The result also sets (a), (b) and (c) against their memory floors at --hbm-tbs: per pixel (a) reads
8 C + 8 C + 4 + 32 bytes and writes 8, (b) reads 8 C + 32 and writes 8, (c) reads 8 C + 8 + 32 and writes 8 C + 8 per
level; each call also packs the records once (the planes in, 32 bytes out), which the floors leave out.
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/denoise_var_time.py [--frames 20] [--warmup 3] [--kinds all|plain] [--parent a.json]
                                     [--out profiles/denoise_var/denoise_var_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"indirect": ("c5_area_light.yaml", 1920, 1080, 3), "ao": ("c2_s1024.yaml", 1920, 1080, 1)}
LEVELS = 5
GUIDES = dict(sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1)
PLAIN_SIGMA_COLOR, VAR_SIGMA_COLOR, EPSILON = 0.5, 4.0, 1e-12
H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
G3 = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def _shifted(H, W, ox, oy):
    return ((slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox))),
            (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox))))


def torch_var_filter(F, V, z, nrm, ids, alb, levels, sc, eps, sn, sz, sa):
    """rray_amd.denoise_var_filter in torch on device tensors: F (H, W, C) f64, V (H, W), z (H, W), nrm / alb (H, W, 3),
    ids (H, W) int32; guides rounded to f32 and widened -> (F', V')."""
    H, W, Cn = F.shape
    f32 = lambda v: v.to(torch.float32).to(torch.float64)  # noqa: E731
    z, nrm, alb = f32(z), f32(nrm), f32(alb)
    void = ~(z < float("inf")) | (ids < 0)
    zero = torch.zeros((), dtype=torch.float64, device=F.device)
    sc2 = sc * sc
    for i in range(levels):
        s = 1 << i
        ga = torch.zeros((H, W), dtype=torch.float64, device=F.device)
        gs = torch.zeros_like(ga)
        for ey in range(-1, 2):
            for ex in range(-1, 2):
                P, Q = _shifted(H, W, ex, ey)
                ok = ~void[P] & ~void[Q]
                gw = G3[ey + 1] * G3[ex + 1]
                ga[P] += torch.where(ok, gw * V[Q], zero)
                gs[P] += ok.to(torch.float64) * gw
        den = sc2 * (ga / gs) + eps
        acc = torch.zeros_like(F)
        va = torch.zeros_like(ga)
        ws = torch.zeros_like(ga)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * s, dy * s
                if abs(ox) >= W or abs(oy) >= H:
                    continue
                P, Q = _shifted(H, W, ox, oy)
                ok = ~void[P] & ~void[Q]
                w = torch.full(ok.shape, H5[dy + 2] * H5[dx + 2], dtype=torch.float64, device=F.device)
                Fq = F[Q]
                if dx or dy:
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
                    d = F[P] - Fq
                    dc = d[..., 0] * d[..., 0]
                    if Cn == 3:
                        dc = (dc + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    t = 1.0 + dc / den[P]
                    ok &= t > 0.0
                    w = w * (1.0 / (t * t))
                ok &= w > 0.0
                w = torch.where(ok, w, zero)
                acc[P] += torch.where(ok[..., None], w[..., None] * Fq, zero)
                va[P] += torch.where(ok, (w * w) * V[Q], zero)
                ws[P] += w
        safe = torch.where(void, 1.0, ws)
        F = torch.where(void[..., None], F, acc / safe[..., None])
        V = torch.where(void, V, va / (safe * safe))
    return F, V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="all", choices=("all", "plain"))
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--limit", type=float, default=60.0, help="seconds after which a variant's rounds stop")
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the copy bandwidth the memory floors are computed at")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("denoise_var_time: no HIP device (the timing needs the MI355X)")
    E = R._lib
    dev = torch.device("cuda", 0)
    full = args.kinds == "all"
    rend = R.Renderer(0)
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "kinds": args.kinds, "levels": LEVELS,
              "guides": GUIDES, "plain_sigma_color": PLAIN_SIGMA_COLOR, "var_sigma_color": VAR_SIGMA_COLOR,
              "epsilon": EPSILON, "hbm_tbs": args.hbm_tbs, "rows": {}}

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
        name, W, H, Cn = spec
        path = os.path.join(ROOT, "scenes", name)
        scene = R.YamlScene(open(path).read(), W, H, 1, obj_root=os.path.dirname(path))
        rend.upload(scene)
        cam = scene.camera
        n = W * H
        row = {"scene": name, "width": W, "height": H, "channels": Cn}
        opts = E.RenderOpts(1, 5, 0, 0, 0, 1, 8, 0, 0, 0)
        f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
        with torch.cuda.stream(stream):
            raw, img, m2 = f64(H, W, Cn), f64(H, W, Cn), f64(H, W, Cn)
            depth, normal, albedo = f64(H, W), f64(H, W, 3), f64(H, W, 3)
            obj = torch.zeros((H, W), dtype=torch.int32, device=dev)
            count, zero_n = torch.zeros_like(obj), torch.zeros_like(obj)
            zero_img = f64(H, W, Cn)
            var = {k: f64(H, W) for k in "ab"}
            out = {k: f64(H, W, Cn) for k in "cde"}
            vout = {k: f64(H, W) for k in "ce"}
            if key == "indirect":
                rend.render_indirect_device(cam, opts, R.Indirect(4, 1, seed=1), raw.data_ptr(), s)
            else:
                rend.render_ao_device(cam, opts, R.Ao(16, 1.0, seed=1), raw.data_ptr(), s)
            rend.render_aov_device(cam, opts, ("depth", "normal", "object", "albedo"), depth.data_ptr(), normal.data_ptr(),
                                   obj.data_ptr(), albedo.data_ptr(), s)
            planes = dict(depth=depth.data_ptr(), normal=normal.data_ptr(), object=obj.data_ptr())
            rend.temporal_device(R.Temporal(), W, H, Cn, cam, cam, dict(image=raw.data_ptr(), **planes),
                                 dict(image=zero_img.data_ptr(), count=zero_n.data_ptr(), m2=zero_img.data_ptr(), **planes),
                                 img.data_ptr(), count.data_ptr(), m2.data_ptr(), stream=s)
        stream.synchronize()
        row["hit_share"] = float((obj >= 0).double().mean())
        guides = dict(d_depth=depth.data_ptr(), d_normal=normal.data_ptr(), d_object=obj.data_ptr(), d_albedo=albedo.data_ptr())
        variants = {}

        def d():
            rend.denoise_device(R.Denoise(LEVELS, sigma_color=PLAIN_SIGMA_COLOR, **GUIDES), W, H, Cn, img.data_ptr(),
                                out["d"].data_ptr(), stream=s, **guides)

        if full:
            vr = R.Variance(min_history=1, **GUIDES)
            dv = R.DenoiseVar(LEVELS, sigma_color=VAR_SIGMA_COLOR, epsilon=EPSILON, **GUIDES)

            def a():
                rend.variance_device(vr, W, H, Cn, img.data_ptr(), var["a"].data_ptr(), d_m2=m2.data_ptr(),
                                     d_count=count.data_ptr(), stream=s, **guides)

            def b():
                rend.variance_device(vr, W, H, Cn, img.data_ptr(), var["b"].data_ptr(), stream=s, **guides)

            def c():
                rend.denoise_var_device(dv, W, H, Cn, img.data_ptr(), var["b"].data_ptr(), out["c"].data_ptr(),
                                        vout["c"].data_ptr(), stream=s, **guides)

            def e():
                out["e"], vout["e"] = torch_var_filter(img, var["b"], depth, normal, obj, albedo, LEVELS, VAR_SIGMA_COLOR,
                                                       EPSILON, GUIDES["sigma_normal"], GUIDES["sigma_depth"],
                                                       GUIDES["sigma_albedo"])

            for f in (a, b, c, e):
                timed(f)
            stream.synchronize()
            live = obj >= 0
            # after one frame every moment equals in * in, so (a)'s plane is all zeros: (c) and (e) run under (b)'s, the
            # plane a first frame really has
            row["a_plane_max"] = float(var["a"].max())
            row["b_plane_mean"] = float(var["b"][live].mean())
            diff = float((out["c"] - out["e"])[live].abs().max())
            vdiff = float((vout["c"] - vout["e"])[live].abs().max())
            row["max_abs_c_minus_e"], row["max_abs_var_c_minus_e"] = diff, vdiff
            if not (diff <= 1e-9 and vdiff <= 1e-9):
                raise SystemExit(f"denoise_var_time: {key}: denoise_var_device differs from the torch filter by {diff}, {vdiff}")
            row["mean_abs_change"] = float((img - out["c"])[live].abs().mean())
            variants.update(a_variance_history=a, b_variance_spatial=b, c_denoise_var=c)
        variants["d_denoise_plain"] = d
        if full:
            variants["e_torch_var_filter"] = e
        row.update(rounds(variants))
        if full:
            ms = {k[0]: row[k]["median_ms"] for k in variants}
            tb = args.hbm_tbs * 1e12
            floors = {"a": n * (16 * Cn + 4 + 32 + 8) / tb * 1e3, "b": n * (8 * Cn + 32 + 8) / tb * 1e3,
                      "c": LEVELS * n * (16 * Cn + 16 + 32) / tb * 1e3}
            row["memory_floor_ms"] = floors
            row["over_floor"] = {k: ms[k] / floors[k] for k in floors}
            row["c_over_d"] = ms["c"] / ms["d"]
            row["e_over_c"] = ms["e"] / ms["c"]
        return row

    for key, spec in ROWS.items():
        result["rows"][key] = row_of(key, spec)
    rend.close()

    if args.parent:
        runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in args.parent]
        result["parent"] = {"digests": sorted({r["digest"] for r in runs}), "runs": len(runs),
                            "d_denoise_plain": {k: [r["rows"][k]["d_denoise_plain"] for r in runs] for k in ROWS}}
        if full:
            result["c_over_parent_d"] = {}
            for k in ROWS:
                parent_median = statistics.median(p["median_ms"] for p in result["parent"]["d_denoise_plain"][k])
                c = result["rows"][k]["c_denoise_var"]["median_ms"]
                result["c_over_parent_d"][k] = {"c_median_ms": c, "parent_d_median_ms": parent_median, "ratio": c / parent_median}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
