"""Times the device-resident ray queries (rr_color_at_device, rr_hit_at_device, rr_camera_rays_device) against the
host-buffer entries and against the frame the same rays make, in one process.

Rows (every variant of a row runs once per round, the variants alternating; --frames rounds after --warmup):
  colour   C2's scene, the 1920 x 1080 camera's rays, remaining 5:
             a  host color_at from numpy arrays                            wall clock around the call (it blocks)
             b  color_at_device from a resident tensor                     wall clock around the call + a device synchronise
             c  camera_rays_device + color_at_device                       one HIP event pair on the tool's stream
             d  render_device with RR_OUT_CANVAS (the frame of those rays) one HIP event pair on the tool's stream
  permuted the same rays under one fixed random permutation, color_at_device as b (recorded only: what incoherent
           waves cost)
  hit      C4's scene, the 512 x 512 camera's rays: hit_at host against hit_at_device, both by the wall clock (+ a
           device synchronise for the device entry)
Before any timing the outputs of every row are compared bit for bit (a = b = c = d, the permuted colours are b's
permuted, the device records are the host's).  --kinds host times a and the host hit_at alone, which a build without
the device entries can run too (--package-root: the tree whose rray_amd package and library are used; the scenes are
this tree's; the rays then come from the frame's arithmetic in numpy via the host entry's own camera: see host_rays).
Prints one JSON line.  Needs the MI355X: there is no CPU path.

    python tools/rays_time.py [--frames 20] [--warmup 3] [--kinds all|host] [--out profiles/rays/rays_time.json]
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


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def host_rays(cam):
    """Camera::ray_for_pixel (camera.rs:75-93) for every sample in numpy, for a build without rr_camera_rays_device.
    Used for timing the host entries only (the values need not be the device's bit for bit: an affine camera)."""
    T = np.linalg.inv(np.array(list(cam.transform), np.float64).reshape(4, 4))
    px, py = np.meshgrid(np.arange(cam.hsize), np.arange(cam.vsize))
    wx = cam.half_width - (px.reshape(-1) + 0.5) * cam.pixel_size
    wy = cam.half_height - (py.reshape(-1) + 0.5) * cam.pixel_size
    p = np.stack([wx, wy, -np.ones_like(wx), np.ones_like(wx)], 1) @ T.T
    o = np.tile(T[:3, 3], (len(wx), 1))
    d = p[:, :3] - o
    return np.ascontiguousarray(o), np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="all", choices=("all", "host"))
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.frames < 20:
        ap.error("--frames must be at least 20")
    sys.path.insert(0, os.path.abspath(args.package_root))
    import rray_amd as R

    lib_digest, _ = R._lib.check_provenance()
    if R.device_count() < 1:
        raise SystemExit("rays_time: no HIP device (the timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    device = args.kinds == "all"
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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

    def events(f):
        torch.cuda.synchronize()
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def rounds(variants):
        ms = {k: [] for k in variants}
        for i in range(args.warmup + args.frames):
            for k, f in variants.items():
                t = f()
                if i >= args.warmup:
                    ms[k].append(t)
        return {k: summary(v) for k, v in ms.items()}

    # ---- colour rows ----
    scene = scene_of(COLOUR)
    cam = scene.camera
    n = cam.hsize * cam.vsize
    row = {"scene": COLOUR[0], "width": COLOUR[1], "height": COLOUR[2], "rays": n, "remaining": 5}
    if device:
        rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
        rays_c = torch.empty_like(rays)
        rgb_b, rgb_c, rgb_d = (torch.empty((n, 3), dtype=torch.float64, device=dev) for _ in range(3))
        torch.cuda.synchronize()
        rend.camera_rays_device(cam, rays.data_ptr())
        torch.cuda.synchronize()
        host = rays.cpu().numpy()
        o, d = np.ascontiguousarray(host[:, :3]), np.ascontiguousarray(host[:, 3:])
    else:
        o, d = host_rays(cam)
    opts = R._lib.RenderOpts(1, 5, 0, 0, 0, 1, 8, R._lib.RR_OUT_CANVAS, 0, 0)
    out_a = {}

    def run_a():
        out_a["rgb"] = rend.color_at(o, d, remaining=5)

    def run_b():
        rend.color_at_device(n, rays.data_ptr(), rgb_b.data_ptr(), remaining=5)

    def run_c():
        rend.camera_rays_device(cam, rays_c.data_ptr(), s)
        rend.color_at_device(n, rays_c.data_ptr(), rgb_c.data_ptr(), remaining=5, stream=s)

    def run_d():
        rend.render_device(cam, opts, rgb_d.data_ptr(), None, s)

    variants = {"a_host_color_at": lambda: wall(run_a)}
    if device:
        variants.update({"b_color_at_device": lambda: wall(run_b), "c_camera_rays_then_color_at_device": lambda: events(run_c),
                         "d_render_device_canvas": lambda: events(run_d)})
        for f in variants.values():  # once, then the comparison
            f()
        b, c, dd = rgb_b.cpu().numpy(), rgb_c.cpu().numpy(), rgb_d.cpu().numpy()
        row["bit_equal"] = bool(np.array_equal(out_a["rgb"], b, equal_nan=True) and np.array_equal(b, c, equal_nan=True) and
                                np.array_equal(c, dd, equal_nan=True) and torch.equal(rays, rays_c))
        if not row["bit_equal"]:
            raise SystemExit("rays_time: the colour row's outputs differ")
    row.update(rounds(variants))
    if device:
        row["host_over_device"] = row["a_host_color_at"]["median_ms"] / row["b_color_at_device"]["median_ms"]
        row["rays_over_frame"] = (row["c_camera_rays_then_color_at_device"]["median_ms"] /
                                  row["d_render_device_canvas"]["median_ms"])
    result["rows"]["colour"] = row

    if device:  # the same rays, shuffled once
        perm = torch.from_numpy(np.random.default_rng(20261020).permutation(n)).to(dev)
        rays_p = rays[perm].contiguous()
        rgb_p = torch.empty_like(rgb_b)

        def run_p():
            rend.color_at_device(n, rays_p.data_ptr(), rgb_p.data_ptr(), remaining=5)

        wall(run_p)
        prow = {"rays": n, "bit_equal": bool(torch.equal(rgb_p, rgb_b[perm]))}
        if not prow["bit_equal"]:
            raise SystemExit("rays_time: the permuted colours are not the permuted colours")
        prow.update(rounds({"b_color_at_device_permuted": lambda: wall(run_p), "b_color_at_device": lambda: wall(run_b)}))
        prow["permuted_over_coherent"] = prow["b_color_at_device_permuted"]["median_ms"] / prow["b_color_at_device"]["median_ms"]
        result["rows"]["permuted"] = prow
        del rays_p, rgb_p, rays_c, rgb_c, rgb_d

    # ---- hit row ----
    scene = scene_of(HIT)
    cam = scene.camera
    n = cam.hsize * cam.vsize
    row = {"scene": HIT[0], "width": HIT[1], "height": HIT[2], "rays": n}
    if device:
        hrays = torch.empty((n, 6), dtype=torch.float64, device=dev)
        hits = torch.empty((n, 192), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        rend.camera_rays_device(cam, hrays.data_ptr())
        torch.cuda.synchronize()
        host = hrays.cpu().numpy()
        o, d = np.ascontiguousarray(host[:, :3]), np.ascontiguousarray(host[:, 3:])
    else:
        o, d = host_rays(cam)
    out_h = {}

    def run_hit_host():
        out_h["hits"] = rend.hit_at(o, d)

    def run_hit_dev():
        rend.hit_at_device(n, hrays.data_ptr(), hits.data_ptr())

    variants = {"host_hit_at": lambda: wall(run_hit_host)}
    if device:
        variants["hit_at_device"] = lambda: wall(run_hit_dev)
        for f in variants.values():
            f()
        got = hits.cpu().numpy().reshape(-1).view(R._lib.hit_dtype())
        row["bit_equal"] = all(bool(np.array_equal(got[k], out_h["hits"][k], equal_nan=got[k].dtype.kind == "f"))
                               for k in got.dtype.names)
        if not row["bit_equal"]:
            raise SystemExit("rays_time: the device records differ from the host's")
    row.update(rounds(variants))
    if device:
        row["host_over_device"] = row["host_hit_at"]["median_ms"] / row["hit_at_device"]["median_ms"]
    result["rows"]["hit"] = row
    rend.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
