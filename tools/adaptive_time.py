"""Frame times of adaptive anti-aliasing (rr_render_adaptive_device) next to the full frame and the aa 1 frame of the
same build, in one process.

For C3 (scenes/c3_s1024_reflect.yaml, 3840x2160 aa 3), C4 (scenes/c4_teapot.yaml, 1920x1080 aa 2) and C5
(scenes/c5_area_light.yaml, 1920x1080 aa 2), all at max_depth 5, it reports the HIP-event kernel_ms
(rr_stats.kernel_ms) of
  * the full frame (rr_render_device at the config's aa into the f64 averaged image: the benchmark's frame),
  * the aa 1 frame of the same view (the adaptive frame's probe alone),
  * the adaptive frame at thresholds -1 (every pixel listed: prices the list path against the tile path), 0.02, 0.05,
    0.1 and +inf (no pixel listed: prices the mask and the scan),
each after a warm-up, over --frames frames, the kinds alternating frame by frame so that they share whatever else the
machine is doing: median, minimum and maximum.  Per threshold also the refined fraction and, against the full frame,
max |delta| and the number of pixels whose u8 colour (rr_quantize) differs.  Everything renders into device buffers;
nothing is copied back inside the timed frames.  Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/adaptive_time.py [--frames 20] [--warmup 3] [--configs C3,C4,C5] [--out file.json]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C3": ("c3_s1024_reflect.yaml", 3840, 2160, 3), "C4": ("c4_teapot.yaml", 1920, 1080, 2),
           "C5": ("c5_area_light.yaml", 1920, 1080, 2)}
THRESHOLDS = (-1.0, 0.02, 0.05, 0.1, math.inf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="C3,C4,C5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 20:
        ap.error("--frames must be at least 20")
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("adaptive_time: no HIP device (the timing needs the MI355X)")
    hip = ctypes.CDLL("libamdhip64.so.7")

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) != 0:
            raise SystemExit(f"adaptive_time: hipMalloc({nbytes}) failed")
        return p

    def to_host(arr, dptr):
        if hip.hipMemcpy(arr.ctypes.data_as(ctypes.c_void_p), dptr, ctypes.c_size_t(arr.nbytes), 2) != 0:
            raise SystemExit("adaptive_time: hipMemcpy failed")
        return arr

    rend = R.Renderer(0)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "max_depth": 5, "configs": {}}
    for name in args.configs.split(","):
        scene_file, W, H, aa = CONFIGS[name]
        path = os.path.join(ROOT, "scenes", scene_file)
        scene = R.YamlScene(open(path).read(), W, H, aa, obj_root=os.path.dirname(path))
        rend.upload(scene)
        cam = scene.camera
        cam1 = R.camera(W, H, cam.field_of_view, list(cam.transform))
        kinds = ["full", "aa1"] + [f"adaptive_{t}" for t in THRESHOLDS]
        bufs = {k: dmalloc(W * H * 24) for k in kinds}
        d_n = dmalloc(8)
        full_opts = R._lib.RenderOpts(aa, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG, 0, 0)
        aa1_opts = R._lib.RenderOpts(1, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG, 0, 0)
        ad_opts = R._lib.RenderOpts(aa, 5, 0, 0, 0, 1, 8, 0, 0, 0)

        def run(kind):
            if kind == "full":
                rend.render_device(cam, full_opts, None, bufs[kind].value, None)
            elif kind == "aa1":
                rend.render_device(cam1, aa1_opts, None, bufs[kind].value, None)
            else:
                rend.render_adaptive_device(cam, ad_opts, float(kind.split("_")[1]), bufs[kind].value, None, d_n.value)

        ms = {k: [] for k in kinds}
        stats = {}
        for i in range(args.warmup + args.frames):
            for k in kinds:
                run(k)
                st = rend.last_stats()  # waits for the frame; kernel_ms is its HIP event pair
                if i >= args.warmup:
                    ms[k].append(st["kernel_ms"])
                stats[k] = st
        full = to_host(np.zeros((H, W, 3)), bufs["full"])
        full_q = R.quantize(full)
        cfg = {"scene": scene_file, "width": W, "height": H, "aa": aa}
        for k in kinds:
            v = ms[k]
            row = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rays": stats[k]["rays"],
                   "samples": stats[k]["samples"]}
            if k != "full":
                img = to_host(np.zeros((H, W, 3)), bufs[k])
                with np.errstate(invalid="ignore"):
                    row["max_abs_delta_vs_full"] = float(np.nanmax(np.abs(img - full)))
                row["u8_pixels_differing"] = int((R.quantize(img) != full_q).any(axis=2).sum())
            if k.startswith("adaptive_"):
                row["refined_fraction"] = (stats[k]["samples"] - W * H) / (aa * aa) / (W * H)
                row["over_full"] = row["median_ms"] / statistics.median(ms["full"])
            cfg[k] = row
        for p in list(bufs.values()) + [d_n]:
            hip.hipFree(p)
        result["configs"][name] = cfg
    rend.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
