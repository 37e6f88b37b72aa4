"""Times temporal accumulation (rr_temporal_device) against the same filter written in torch, in one
process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup; each time is
a torch event pair on the one stream everything runs on, behind a 1 GiB read-modify-write that leaves the caches cold,
so that no variant profits from what its predecessor in the round left there; each variant's rounds stop at --limit
seconds), both at
1920 x 1080 under a small camera move, with the Temporal() defaults and a history of one frame:
  indirect  C5's area-light scene: the K = 4 indirect plane, C = 3, moments on
  ao        C2's scene: the K = 16 occlusion plane (radius 1), C = 1
        a_temporal_device  temporal_device in a default context (the 32 x 8 tile)
        a_rows             temporal_device in a context created under RRAY_TEMPORAL_ROWS=1 (the row-major lane map): the
                           A/B of the two maps
        b_torch_filter     the same filter in torch in f64: project, four index gathers, the tests, the blend.  It needs
                           nothing from the library
        frame              the frame's own render (render_indirect_device / render_ao_device), for scale
Before any timing, at 64 x 36 on the same scenes and cameras, temporal_device must equal rr_temporal_reference bit for
bit, and at full size (a) is compared with (b): the largest difference must be rounding noise (the torch form is not
asked to be bit-equal).
The result sets (a) against the frame it accumulates and against the memory floor: the bytes of every plane read or
written once, at the HBM peak (--hbm-peak-tbs, 8.0 TB/s) and at the measured copy bandwidth (--hbm-tbs, 6.29 TB/s).
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/temporal_time.py [--frames 30] [--warmup 3] [--out profiles/temporal/temporal_time.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {"indirect": ("c5_area_light.yaml", 3, True), "ao": ("c2_s1024.yaml", 1, False)}
W_FULL, H_FULL = 1920, 1080


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def moved(R, cam, W, H):
    """the camera turned a little about its y axis and shifted"""
    a = 0.01
    rot = np.array([[math.cos(a), 0, math.sin(a), 0.03], [0, 1, 0, -0.01], [-math.sin(a), 0, math.cos(a), 0.005], [0, 0, 0, 1]])
    M = rot @ np.array(list(cam.transform), np.float64).reshape(4, 4)
    return R.camera(W, H, cam.field_of_view, [float(v) for v in M.reshape(-1)])


def torch_filter(tp, cam, pcam, img, depth, normal, ids, pimg, pdepth, pnormal, pids, pcnt, pm2):
    """rray_amd.temporal_filter for moving cameras in torch on device tensors (H, W[, C]) -> (out, n, m2)"""
    H, W, Cn = img.shape
    dev = img.device
    f64 = dict(dtype=torch.float64, device=dev)
    M = np.linalg.inv(np.array(list(cam.transform)).reshape(4, 4))
    Mp = np.linalg.inv(np.array(list(pcam.transform)).reshape(4, 4))
    T = np.array(list(pcam.transform)).reshape(4, 4)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")

    def dirs(m, c, x, y):
        wx = c.half_width - (x.to(torch.float64) + 0.5) * c.pixel_size
        wy = c.half_height - (y.to(torch.float64) + 0.5) * c.pixel_size
        d = [(m[r, 0] * wx + m[r, 1] * wy) - m[r, 2] for r in range(3)]  # f - o: the translation cancels
        mag = torch.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return [v / mag for v in d]

    void = ~(depth < float("inf")) | (ids < 0)
    pvoid = ~(pdepth < float("inf")) | (pids < 0)
    d = dirs(M, cam, xs, ys)
    P = [M[r, 3] + depth * d[r] for r in range(3)]
    c = [((T[r, 0] * P[0] + T[r, 1] * P[1]) + T[r, 2] * P[2]) + T[r, 3] for r in range(3)]
    cand = ~void & (c[2] < 0.0)
    fx = (pcam.half_width - c[0] / -c[2]) / pcam.pixel_size - 0.5
    fy = (pcam.half_height - c[1] / -c[2]) / pcam.pixel_size - 0.5
    cand &= (fx > -1.0) & (fx < W) & (fy > -1.0) & (fy < H)
    fx0, fy0 = torch.floor(fx), torch.floor(fy)
    ax, ay = fx - fx0, fy - fy0
    x0 = torch.where(cand, fx0, torch.zeros((), **f64)).to(torch.int64)
    y0 = torch.where(cand, fy0, torch.zeros((), **f64)).to(torch.int64)
    e = [P[r] - Mp[r, 3] for r in range(3)]
    te = torch.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    acc, accm2 = torch.zeros_like(img), torch.zeros_like(img)
    ws = torch.zeros((H, W), **f64)
    nmin = torch.full((H, W), 2**31 - 1, dtype=torch.int64, device=dev)
    zero = torch.zeros((), **f64)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            w = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
            ok = cand & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = qx.clamp(0, W - 1), qy.clamp(0, H - 1)
            q = qy * W + qx
            nq = pcnt.reshape(-1)[q].to(torch.int64)
            ok &= ~pvoid.reshape(-1)[q] & (nq >= 1)
            if tp.object:
                ok &= pids.reshape(-1)[q] == ids
            nqv = pnormal.reshape(-1, 3)[q]
            dot = (normal[..., 0] * nqv[..., 0] + normal[..., 1] * nqv[..., 1]) + normal[..., 2] * nqv[..., 2]
            ok &= (1.0 - dot) <= tp.sigma_normal
            dq = dirs(Mp, pcam, qx, qy)
            zq = pdepth.reshape(-1)[q]
            Q = [Mp[r, 3] + zq * dq[r] for r in range(3)]
            g = (normal[..., 0] * (Q[0] - P[0]) + normal[..., 1] * (Q[1] - P[1])) + normal[..., 2] * (Q[2] - P[2])
            ok &= (torch.abs(g) <= tp.sigma_plane * te) & (w > 0.0)
            w = torch.where(ok, w, zero)
            acc += w[..., None] * torch.where(ok[..., None], pimg.reshape(-1, Cn)[q], zero)
            if pm2 is not None:
                accm2 += w[..., None] * torch.where(ok[..., None], pm2.reshape(-1, Cn)[q], zero)
            ws += w
            nmin = torch.where(ok, torch.minimum(nmin, nq), nmin)
    keep = ws > 0.0
    n = torch.where(keep, torch.clamp(nmin + 1, max=tp.max_history), torch.ones_like(nmin)).to(torch.int32)
    a = torch.clamp(1.0 / n.to(torch.float64), min=tp.alpha)[..., None]
    safe = torch.where(keep, ws, torch.ones((), **f64))[..., None]
    h = acc / safe
    out = torch.where(keep[..., None], h + (img - h) * a, img)
    m2 = None
    if pm2 is not None:
        hm2 = accm2 / safe
        m2 = torch.where(keep[..., None], hm2 + (img * img - hm2) * a, img * img)
    return out, n, m2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=float, default=45.0, help="seconds after which a variant's rounds stop")
    ap.add_argument("--hbm-peak-tbs", type=float, default=8.0, help="the HBM peak the memory floor is computed at")
    ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the measured copy bandwidth, for a second floor")
    ap.add_argument("--width", type=int, default=W_FULL)
    ap.add_argument("--height", type=int, default=H_FULL)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("temporal_time: no HIP device (the timing needs the MI355X)")
    E = R._lib
    dev = torch.device("cuda", 0)
    rend = R.Renderer(0)
    os.environ["RRAY_TEMPORAL_ROWS"] = "1"  # read at context creation
    rend_rows = R.Renderer(0)
    del os.environ["RRAY_TEMPORAL_ROWS"]
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tp = R.Temporal()
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "temporal": repr(tp),
              "hbm_peak_tbs": args.hbm_peak_tbs, "hbm_tbs": args.hbm_tbs, "rows": {}}

    flush = torch.zeros(1 << 27, dtype=torch.float64, device=dev)  # 1 GiB: four times the 256 MiB Infinity Cache

    def timed(f):
        with torch.cuda.stream(stream):
            flush.add_(1.0)  # every timed call starts with cold caches, whatever ran before it
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

    def image(r, key, cam, seed):
        opts = E.RenderOpts(1, 0, seed, 0, 0, 1, 8, 0, 0, 0)
        if key == "indirect":
            return lambda d_out: r.render_indirect_device(cam, opts, R.Indirect(4, 1, seed=seed), d_out, s)
        return lambda d_out: r.render_ao_device(cam, opts, R.Ao(16, 1.0, seed=seed), d_out, s)

    def frames(key, scene_text, root, W, H, Cn, moments):
        """device tensors of the two frames: the previous one accumulated once (counts of 1), the current one raw"""
        scene = R.YamlScene(scene_text, W, H, 1, obj_root=root)
        rend.upload(scene)
        cams = (scene.camera, moved(R, scene.camera, W, H))
        opts = E.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)
        f64 = dict(dtype=torch.float64, device=dev)
        out = []
        with torch.cuda.stream(stream):
            for k, cam in enumerate(cams):
                t = dict(image=torch.zeros((H, W, Cn), **f64), depth=torch.zeros((H, W), **f64),
                         normal=torch.zeros((H, W, 3), **f64), object=torch.zeros((H, W), dtype=torch.int32, device=dev))
                image(rend, key, cam, 1 + k)(t["image"].data_ptr())
                rend.render_aov_device(cam, opts, ("depth", "normal", "object"), t["depth"].data_ptr(), t["normal"].data_ptr(),
                                       t["object"].data_ptr(), None, s)
                out.append(t)
            prev = out[0]
            first = dict(prev, image=torch.zeros_like(prev["image"]), count=torch.zeros((H, W), dtype=torch.int32, device=dev),
                         m2=torch.zeros_like(prev["image"]) if moments else None)
            none = dict(prev, image=torch.zeros_like(prev["image"]), count=torch.zeros((H, W), dtype=torch.int32, device=dev),
                        m2=torch.zeros_like(prev["image"]) if moments else None)
            ptr = lambda f: {k: (None if v is None else v.data_ptr()) for k, v in f.items()}  # noqa: E731
            rend.temporal_device(tp, W, H, Cn, cams[0], cams[0], ptr(prev), ptr(none), first["image"].data_ptr(),
                                 first["count"].data_ptr(), first["m2"].data_ptr() if moments else None, stream=s)
        stream.synchronize()
        return cams, out[1], first

    def row_of(key, spec):
        name, Cn, moments = spec
        path = os.path.join(ROOT, "scenes", name)
        text, root = open(path).read(), os.path.dirname(path)
        ptr = lambda f: {k: (None if v is None else v.data_ptr()) for k, v in f.items()}  # noqa: E731
        # 1. the device entry equals the host reference, at 64 x 36
        cams, cur, hist = frames(key, text, root, 64, 36, Cn, moments)
        host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        want = R.temporal_reference(host(cur["image"]), tp, cams[1], cams[0], host(cur["depth"]), normal=host(cur["normal"]),
                                    object=host(cur["object"]), moments=moments,
                                    prev={"out": host(hist["image"]), "n": host(hist["count"]), "m2": host(hist["m2"]),
                                          "depth": host(hist["depth"]), "normal": host(hist["normal"]),
                                          "object": host(hist["object"])})
        small_equal = {}
        for label, r in (("tile", rend), ("rows", rend_rows)):
            o = (torch.zeros((36, 64, Cn), dtype=torch.float64, device=dev), torch.zeros((36, 64), dtype=torch.int32, device=dev),
                 torch.zeros((36, 64, Cn), dtype=torch.float64, device=dev) if moments else None)
            r.temporal_device(tp, 64, 36, Cn, cams[1], cams[0], ptr(cur), ptr(hist), o[0].data_ptr(), o[1].data_ptr(),
                              o[2].data_ptr() if moments else None, stream=s)
            stream.synchronize()
            same = np.array_equal(host(o[0]).reshape(want["out"].shape), want["out"], equal_nan=True) and \
                np.array_equal(host(o[1]), want["n"]) and (not moments or np.array_equal(host(o[2]).reshape(want["m2"].shape),
                                                                                          want["m2"], equal_nan=True))
            small_equal[label] = bool(same)
            if not same:
                raise SystemExit(f"temporal_time: {key}: temporal_device ({label}) differs from rr_temporal_reference at 64 x 36")
        # 2. the timed frames
        W, H = args.width, args.height
        n = W * H
        cams, cur, hist = frames(key, text, root, W, H, Cn, moments)
        row = {"scene": name, "width": W, "height": H, "channels": Cn, "moments": moments, "equal_reference_64x36": small_equal,
               "hit_share": float((cur["object"] >= 0).double().mean())}
        f64 = dict(dtype=torch.float64, device=dev)
        outs = {k: (torch.zeros((H, W, Cn), **f64), torch.zeros((H, W), dtype=torch.int32, device=dev),
                    torch.zeros((H, W, Cn), **f64) if moments else None) for k in ("a", "rows")}
        res_b = {}

        def run(r, o):
            r.temporal_device(tp, W, H, Cn, cams[1], cams[0], ptr(cur), ptr(hist), o[0].data_ptr(), o[1].data_ptr(),
                              o[2].data_ptr() if moments else None, stream=s)

        def b():
            res_b["o"] = torch_filter(tp, cams[1], cams[0], cur["image"], cur["depth"], cur["normal"], cur["object"],
                                      hist["image"], hist["depth"], hist["normal"], hist["object"], hist["count"], hist["m2"])

        scratch = torch.zeros((H, W, Cn), **f64)
        render = image(rend, key, cams[1], 2)
        variants = {"a_temporal_device": lambda: run(rend, outs["a"]), "a_rows": lambda: run(rend_rows, outs["rows"]),
                    "b_torch_filter": b, "frame": lambda: render(scratch.data_ptr())}
        timed(variants["a_temporal_device"])
        timed(variants["a_rows"])
        timed(b)
        stream.synchronize()
        live = cur["object"] >= 0
        row["reuse_share"] = float((outs["a"][1] > 1)[live].double().mean())
        row["rows_bit_equal_tile"] = bool(all(x is None or torch.equal(x, y) for x, y in zip(outs["a"], outs["rows"])))
        diff = float((outs["a"][0] - res_b["o"][0])[live].abs().max())
        row["max_abs_a_minus_b"] = diff
        row["n_equal_a_b"] = float((outs["a"][1] == res_b["o"][1]).double().mean())
        if not diff <= 1e-9 or not row["rows_bit_equal_tile"]:
            raise SystemExit(f"temporal_time: {key}: temporal_device differs from the torch filter by {diff}")
        row.update(rounds(variants))
        a_ms = row["a_temporal_device"]["median_ms"]  # the default context
        # every plane read or written once: image, depth, normal, object of both frames; count and m2 of the history;
        # out, n and m2 written
        per_pixel = 2 * (8 * Cn + 8 + 24 + 4) + 4 + 8 * Cn + 4 + (16 * Cn if moments else 0)
        row["bytes_per_pixel"] = per_pixel
        for label, tbs in (("memory_floor_peak_ms", args.hbm_peak_tbs), ("memory_floor_copy_ms", args.hbm_tbs)):
            row[label] = n * per_pixel / (tbs * 1e12) * 1e3
        row["a_ms"] = a_ms
        row["a_over_floor_peak"] = a_ms / row["memory_floor_peak_ms"]
        row["a_over_floor_copy"] = a_ms / row["memory_floor_copy_ms"]
        row["achieved_tbs"] = n * per_pixel / (a_ms * 1e-3) / 1e12
        row["a_over_frame"] = a_ms / row["frame"]["median_ms"]
        row["b_over_a"] = row["b_torch_filter"]["median_ms"] / a_ms
        row["expectation_a_below_b"] = bool(row["a_temporal_device"]["median_ms"] < row["b_torch_filter"]["median_ms"])
        return row

    for key, spec in ROWS.items():
        result["rows"][key] = row_of(key, spec)
    rend.close()
    rend_rows.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
