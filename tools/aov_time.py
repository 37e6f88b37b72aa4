"""Frame times of the first-hit (AOV) frames next to the colour frame of the same build, in one process.

For C2 (scenes/c2_s1024.yaml, 1920x1080 aa 1) and C4 (scenes/c4_teapot.yaml, 1920x1080 aa 2) it reports the HIP-event
kernel_ms (rr_stats.kernel_ms) of
  * the AOV frame with all four planes (depth, normal, object, albedo),
  * the AOV frame with depth + object only,
  * the colour frame (rr_render_device into the f64 averaged image, max_depth 5: the benchmark's frame),
each after a warm-up, over --frames frames, alternating the three kinds frame by frame so that they share whatever
else the machine is doing: median, minimum and maximum.  Everything renders into device buffers; nothing is copied
back inside the timed frames.  Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/aov_time.py [--frames 30] [--warmup 5] [--out file.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"C2": ("c2_s1024.yaml", 1920, 1080, 1), "C4": ("c4_teapot.yaml", 1920, 1080, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 20:
        ap.error("--frames must be at least 20")
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("aov_time: no HIP device (the timing needs the MI355X)")
    hip = ctypes.CDLL("libamdhip64.so.7")

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) != 0:
            raise SystemExit(f"aov_time: hipMalloc({nbytes}) failed")
        return p

    rend = R.Renderer(0)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "configs": {}}
    for name, (scene_file, W, H, aa) in CONFIGS.items():
        path = os.path.join(ROOT, "scenes", scene_file)
        scene = R.YamlScene(open(path).read(), W, H, aa, obj_root=os.path.dirname(path))
        rend.upload(scene)
        cam = scene.camera
        n = cam.hsize * cam.vsize
        bufs = {"avg": dmalloc(W * H * 24), "depth": dmalloc(n * 8), "normal": dmalloc(n * 24), "object": dmalloc(n * 4),
                "albedo": dmalloc(n * 24)}
        colour_opts = R._lib.RenderOpts(aa, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_AVG, 0, 0)
        aov_opts = R._lib.RenderOpts(aa, 0, 0, 0, 0, 1, 8, 0, 0, 0)
        ptr = {k: v.value for k, v in bufs.items()}

        def colour():
            rend.render_device(cam, colour_opts, None, ptr["avg"], None)

        def aov_all():
            rend.render_aov_device(cam, aov_opts, ("depth", "normal", "object", "albedo"), ptr["depth"], ptr["normal"],
                                   ptr["object"], ptr["albedo"])

        def aov_depth_object():
            rend.render_aov_device(cam, aov_opts, ("depth", "object"), ptr["depth"], None, ptr["object"], None)

        kinds = {"colour": colour, "aov_all": aov_all, "aov_depth_object": aov_depth_object}
        ms = {k: [] for k in kinds}
        rays = {}
        for i in range(args.warmup + args.frames):
            for k, fn in kinds.items():
                fn()
                st = rend.last_stats()  # waits for the frame; kernel_ms is its HIP event pair
                if i >= args.warmup:
                    ms[k].append(st["kernel_ms"])
                rays[k] = st["rays"]
        for p in bufs.values():
            hip.hipFree(p)
        cfg = {"scene": scene_file, "width": W, "height": H, "aa": aa, "samples": n}
        for k, v in ms.items():
            cfg[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "rays": rays[k]}
        cfg["aov_all_over_colour"] = cfg["aov_all"]["median_ms"] / cfg["colour"]["median_ms"]
        cfg["aov_depth_object_over_colour"] = cfg["aov_depth_object"]["median_ms"] / cfg["colour"]["median_ms"]
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
