"""Frames and parameter sets shared by the host and GPU tests of variance-guided denoising (test_denoise_var_host.py,
test_gpu_denoise_var.py): the same frames, channel counts, level counts, guide-term combinations and history planes on
both sides, each built once per process.  The guides and base images are denoise_cases.frame's (void rows and islands by
depth, by object and by both, a NaN depth, a depth of exactly 0.0, a zero normal, an object seam)."""
import functools
import math

import numpy as np

import denoise_cases as D

same_bits = D.same_bits
# (W, H): one pixel; smaller than every window; smaller than the 7 x 7 window on one axis; a row and a column longer
# than a wave's run of 32; one pixel past a 32 x 8 tile on both axes; several tiles with partial ones at both edges
FRAMES = ((1, 1), (3, 2), (7, 5), (65, 1), (1, 65), (33, 9), (70, 37))
CHANNELS = (1, 3)
ITERATIONS = (1, 2, 6)  # 6: holes of 32 pixels exceed every frame on at least one axis
MIN_HISTORY = 4
# name -> (guide keywords, the planes that are passed): each guide term alone, none, all with and without RR_DN_OBJECT
GUIDES = {
    "none": (dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0), ("depth", "object")),
    "object": (dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.0, object=True), ("object",)),
    "normal": (dict(sigma_normal=0.25, sigma_depth=0.0, sigma_albedo=0.0), ("normal", "depth")),
    "depth": (dict(sigma_normal=0.0, sigma_depth=0.05, sigma_albedo=0.0), ("depth",)),
    "albedo": (dict(sigma_normal=0.0, sigma_depth=0.0, sigma_albedo=0.1), ("albedo", "object")),
    "all": (dict(sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1, object=True), ("depth", "normal", "object", "albedo")),
    "all_no_object": (dict(sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1), ("depth", "normal", "object", "albedo")),
}
# the history given to rr_variance: none; counts mixing 0, MIN_HISTORY - 1, MIN_HISTORY and large values pixel by pixel
# (both branches in every wave); the same counts with min_history = 0 (every pixel temporal, a count of 0 divides by 0)
HISTORIES = ("absent", "mixed", "zero")
# the colour term of rr_denoise_var: on at the default sigma, off
COLOURS = {"colour": 4.0, "plain": 0.0}


@functools.lru_cache(maxsize=None)
def frame(W, H):
    """denoise_cases.frame(W, H) and, per channel count C: img<C> (the base image with one NaN colour where the frame
    has room), m2_<C> and count (a history whose moments lie above, on and below in * in), var (a variance plane with
    exact zeros (a whole block of them in the largest frame), denormals, one NaN and one +inf where the frame has room)."""
    f = dict(D.frame(W, H))
    rng = np.random.default_rng(77000 + 100 * W + H)
    room = W * H >= 35
    for Cn in CHANNELS:
        img = np.array(f[f"img{Cn}"])
        if room:
            img[(H - 1) // 2, (W - 1) // 3] = math.nan  # every channel of one pixel
        f[f"img{Cn}"] = img
        spread = 0.04 * rng.random(img.shape) - 0.005  # mostly above in * in, some below: the clamp
        m2 = img * img + spread
        m2[rng.random(img.shape) < 0.1] = 0.0
        exact = rng.random((H, W)) < 0.15
        m2[exact] = (img * img)[exact]  # a pixel whose m2 == in * in has V == 0.0 exactly
        f[f"m2_{Cn}"] = m2
    f["count"] = rng.choice(np.array([0, MIN_HISTORY - 1, MIN_HISTORY, 9, 1 << 20], np.int32), size=(H, W)).astype(np.int32)
    var = 0.09 * rng.random((H, W)) ** 2
    var[rng.random((H, W)) < 0.2] = 0.0
    if W >= 60 and H >= 30:
        var[8:16, 40:60] = 0.0  # a noise-free block: inside it the prefiltered variance is 0 and den is epsilon
    if room:
        flat = var.reshape(-1)
        flat[3], flat[4], flat[W * H // 2], flat[W * H - 2] = 5e-324, 1e-310, math.nan, math.inf
    f["var"] = var
    for v in f.values():
        v.setflags(write=False)
    return f


def variance_cases():
    """(W, H, C, guides name, history name) of the whole product"""
    return [(W, H, C, g, h) for (W, H) in FRAMES for C in CHANNELS for g in GUIDES for h in HISTORIES]


def variance_arguments(R, W, H, C, guides, history):
    """(image, Variance, keyword arguments) of one case"""
    f = frame(W, H)
    kw, given = GUIDES[guides]
    args = {k: f[k] for k in given}
    if history != "absent":
        args.update(m2=f[f"m2_{C}"], count=f["count"])
    return f[f"img{C}"], R.Variance(min_history=0 if history == "zero" else MIN_HISTORY, **kw), args


@functools.lru_cache(maxsize=None)
def variance_expected(W, H, C, guides, history):
    """variance_estimate of the case, computed once per process and never written to"""
    import rray_amd as R

    img, vr, args = variance_arguments(R, W, H, C, guides, history)
    out = R.variance_estimate(img, vr, **args)
    out.setflags(write=False)
    return out


def filter_cases():
    """(W, H, C, iterations, guides name, colour name) of the whole product"""
    return [(W, H, C, I, g, c) for (W, H) in FRAMES for C in CHANNELS for I in ITERATIONS for g in GUIDES for c in COLOURS]


def filter_arguments(R, W, H, C, iterations, guides, colour):
    """(image, variance plane, DenoiseVar, planes dict) of one case"""
    f = frame(W, H)
    kw, given = GUIDES[guides]
    return f[f"img{C}"], f["var"], R.DenoiseVar(iterations, sigma_color=COLOURS[colour], **kw), {k: f[k] for k in given}


@functools.lru_cache(maxsize=None)
def filter_expected(W, H, C, iterations, guides, colour):
    """(image, variance plane) of denoise_var_filter of the case, computed once per process and never written to"""
    import rray_amd as R

    img, var, dv, planes = filter_arguments(R, W, H, C, iterations, guides, colour)
    out, vout = R.denoise_var_filter(img, var, dv, return_var=True, **planes)
    out.setflags(write=False)
    vout.setflags(write=False)
    return out, vout
