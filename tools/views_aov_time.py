"""Times the first-hit planes of a batch of views (rr_render_views_aov_device) against a loop of rr_render_aov_device
calls over the same cameras, in one process.

Per configuration — a scene, N views of W x H samples — the N cameras sit on a ring around the scene (the scene's own
camera, the world turned about its y axis by k / N of a full turn) and two kinds of run alternate:
  * batch  one rr_render_views_aov_device call into stacked planes of N views;
  * loop   N rr_render_aov_device calls, one per camera, into the N slices of a second set of planes.
Both ask for all four planes (depth, normal, object, albedo) on one stream of the tool's own, and one HIP event pair
encloses the whole batch or all N calls of the loop, so the loop's per-call host work counts where the device waits for
it.  After --warmup rounds, --frames rounds: median, minimum and maximum in milliseconds.  The two sets of planes are
compared once (bit for bit).  --kinds loop times the loop alone, which a build without the batch entry points can run
too (--package-root: the tree whose rray_amd package and library are used; the scenes are this tree's).  Prints one
JSON line.  Needs the MI355X: there is no CPU path.

    python tools/views_aov_time.py [--frames 20] [--warmup 3] [--configs C2,C4,C2L] [--kinds batch,loop] [--out f.json]
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

# name: (scene, views, W, H), aa 1
CONFIGS = {"C2": ("c2_s1024.yaml", 64, 128, 128), "C4": ("c4_teapot.yaml", 64, 128, 128),
           "C2L": ("c2_s1024.yaml", 4, 1920, 1080)}
# plane: (bytes per sample, numpy dtype, trailing shape)
PLANES = {"depth": (8, np.float64, ()), "normal": (24, np.float64, (3,)), "object": (4, np.int32, ()),
          "albedo": (24, np.float64, (3,))}
ORDER = ("depth", "normal", "object", "albedo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="C2,C4,C2L")
    ap.add_argument("--kinds", default="batch,loop")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 20:
        ap.error("--frames must be at least 20")
    kinds = args.kinds.split(",")
    if not set(kinds) <= {"batch", "loop"}:
        ap.error("--kinds: batch, loop or both")
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("views_aov_time: no HIP device (the timing needs the MI355X)")
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipFree.argtypes = [ctypes.c_void_p]

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"views_aov_time: {what} failed ({rc})")

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        ok(hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)), f"hipMalloc({nbytes})")
        return p

    def to_host(arr, dptr):
        ok(hip.hipMemcpy(arr.ctypes.data_as(ctypes.c_void_p), dptr, ctypes.c_size_t(arr.nbytes), 2), "hipMemcpy")
        return arr

    stream, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ok(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")

    rend = R.Renderer(0)
    result = {"digest": lib_digest, "frames": args.frames, "warmup": args.warmup, "planes": list(ORDER), "kinds": kinds,
              "configs": {}}
    for name in args.configs.split(","):
        scene_file, n, W, H = CONFIGS[name]
        path = os.path.join(ROOT, "scenes", scene_file)
        scene = R.YamlScene(open(path).read(), W, H, 1, obj_root=os.path.dirname(path))
        rend.upload(scene)
        base = np.array(list(scene.camera.transform)).reshape(4, 4)
        cams = []
        for k in range(n):
            a = 2.0 * math.pi * k / n
            turn = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]])
            cams.append(R.camera(W, H, scene.camera.field_of_view, [float(v) for v in (base @ turn).reshape(-1)]))
        samples = W * H
        bufs = {k: {p: dmalloc(n * samples * PLANES[p][0]) for p in ORDER} for k in kinds}
        opts = R._lib.RenderOpts(1, 0, 0, 0, 0, 1, 8, 0, 0, 0)

        def run(kind):
            b = bufs[kind]
            ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
            if kind == "batch":
                rend.render_views_aov_device(cams, opts, ORDER, *(b[p].value for p in ORDER), stream.value)
            else:
                for k, cam in enumerate(cams):
                    rend.render_aov_device(cam, opts, ORDER, *(b[p].value + k * samples * PLANES[p][0] for p in ORDER),
                                           stream.value)
            ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
            ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = ctypes.c_float(0.0)
            ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
            return float(ms.value)

        ms = {k: [] for k in kinds}
        for i in range(args.warmup + args.frames):
            for k in kinds:
                t = run(k)
                if i >= args.warmup:
                    ms[k].append(t)
        cfg = {"scene": scene_file, "views": n, "width": W, "height": H, "aa": 1}
        for k in kinds:
            cfg[k] = {"median_ms": statistics.median(ms[k]), "min_ms": min(ms[k]), "max_ms": max(ms[k])}
        if len(kinds) == 2:
            equal = True
            for p in ORDER:
                a, b = (to_host(np.zeros((n, H, W) + PLANES[p][2], PLANES[p][1]), bufs[k][p]) for k in kinds)
                equal = equal and bool(np.array_equal(a, b, equal_nan=p != "object"))
            cfg["bit_equal"] = equal
            cfg["loop_over_batch"] = cfg["loop"]["median_ms"] / cfg["batch"]["median_ms"]
        for b in bufs.values():
            for p in b.values():
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
