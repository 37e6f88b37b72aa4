"""Edge-ray batteries for every leaf kind, CSG and the pattern kinds (tests/test_gpu_shape_rays.py on the GPU,
tests/test_shape_rays_host.py for the conditions that keep those tests from passing vacuously).

A battery is one small scene built on both sides (scene_fuzz.Pair) plus rays written in the object's own space and
mapped to world space with its forward matrix, aimed where leaf_intersect (device_core.inc) branches on EPSILON or on
a strict bound: the cone's |a| < EPS and |a|,|b| < EPS paths and its single-entry return (cone.rs:75-135), the
`mn < y < mx` bounds and cap rims of cones and cylinders, the cube's check_axis with |d| around EPS or 0 * inf
(cube.rs:49-61), torus double roots (torus.rs:37-95), sphere tangents, planes with |d.y| around EPS, triangle edges,
vertices and det around EPS.  Direction lengths run from 1e-3 to 1e3 (the reference never normalises a ray).

Each kind is placed at top level with the identity transform ("ident"), under a non-uniform scale, rotation, shear
and translation ("xform") and inside a sheared group ("group").  Every battery sends its edge rays shuffled (the
waves' bundles are invalid: every node is tested) and then each edge ray again as a fan of 64 rays with 8 x 8 offsets
of 1e-7 rad starting at a multiple of 64 (a valid bundle: the f32 culls and lane tests run at the silhouette).
"""
import functools
import math

import numpy as np

import scene_fuzz as F

EPS = 0.00001  # main.rs:10
LENGTHS = (1.0, 1e-3, 1e3, 0.37, 17.0, 1e-2, 250.0)
MAT = (0.1, 0.9, 0.9, F.SHININESS, 0.3, 0.0, 1.0)
GLASS = (0.1, 0.5, 0.9, F.SHININESS, 0.2, 0.9, 1.5)
PLACEMENTS = ("ident", "xform", "group")
TORUS_RADII = (1e-3, 0.25, 0.99, 1.0, 1.5)
CONES = {"closed": (-1.0, 0.5, True), "open": (-1.0, 0.5, False), "onesided": (-math.inf, 0.5, False)}
FAN_STEP = 1e-7
SHELL_R = 2.0  # the "coneshell" battery's sphere around the cone: found before the cone, after its far entries


class Rays:
    """object-space rays; add() cycles the direction length unless keep (rays whose |d| is part of the edge)"""

    def __init__(self):
        self.o, self.d, self.k = [], [], 0
        self.sh = []  # extra object-space shadow pairs (point, light)

    def add(self, o, d, keep=False):
        o, d = np.array(o, float), np.array(d, float)
        if not keep:
            d = d * LENGTHS[self.k % len(LENGTHS)]
            self.k += 1
        assert np.isfinite(d).all() and np.any(d != 0.0)
        self.o.append(o)
        self.d.append(d)

    def to(self, o, target, keep=False):
        """from o through target (t = 1 before the length cycling)"""
        self.add(o, np.array(target, float) - np.array(o, float), keep)

    def toward(self, rng, n, radius=1.0, centre=(0.0, 0.0, 0.0)):
        """n seeded rays from outside aimed into a ball: the generic hits next to the edges"""
        for _ in range(n):
            o = np.array(centre) + F._unit(rng) * radius * rng.uniform(2.0, 6.0)
            self.to(o, np.array(centre) + rng.uniform(-1, 1, 3) * radius * 0.7)


ANGLES = (0.0, 0.5, math.pi / 2, 2.0, math.pi, 4.0, 5.5)
ORIGINS = ((0.0, 3.0, -4.0), (3.0, -2.5, 1.0), (-2.0, 0.25, 3.0), (0.3, -4.0, 0.2), (0.1, 4.0, -0.3))


def cone_rays(mn, mx, rng):
    R = Rays()
    lo = mn if math.isfinite(mn) else -2.0
    for d in ((0, 1, 0), (1, 1, 0), (1, 0, 0), (0.3, -1, 0.2), (1, 2, 3), (0, -1, 1), (1e-6, 1, 0)):  # through the apex
        d = np.array(d, float)
        R.add(-2.0 * d, d)
        R.add(1.5 * d, -d)
    for ph in ANGLES:  # parallel to the slant: a == 0 up to rounding
        s = np.array([math.cos(ph), 1.0, math.sin(ph)])
        for o in ((0, 0, -2), (0.5, -0.3, 0.1), (-1.0, -0.5, 0.2), (0.2, 0.4, 0.0), (2, 2, 0)):
            R.add(o, s, keep=True)
            R.add(o, -s * 0.7, keep=True)
    for m in (0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0):  # a within +-(EPS/2 .. 2 EPS)
        for sg in (1.0, -1.0):
            a = sg * m * EPS
            for o in ((-1.0, -0.5, 0.2), (0, 0, -2), (0.4, -0.8, 0.0), (-3, -0.2, 0.1)):
                R.add(o, (1.0, math.sqrt(1.0 - a), 0.0), keep=True)
                R.add(o, (1.0, -math.sqrt(1.0 - a), 0.0), keep=True)
    for ph in ANGLES:  # along a surface line: a ~ b ~ 0 (caps only)
        for sy in (1.0, -1.0):
            p = np.array([math.cos(ph), sy, math.sin(ph)])
            R.add(p * 2.0, -p, keep=True)
            R.add(p * 0.25, p * 0.5, keep=True)
            R.add(p * 0.7 + [1e-7, 0, 0], -p, keep=True)  # b just off zero
    for rr in (0.0, 0.1, 0.25, 0.5, 0.5 + 1e-12, 1.0, 1.0 - 1e-12, 1.0 + 1e-12, 2.0):  # axis-parallel
        for ph in (0.0, 2.0):
            x, z = rr * math.cos(ph), rr * math.sin(ph)
            R.add((x, -3.0, z), (0, 1, 0))
            R.add((x, 3.0, z), (0, -1, 0))
            R.add((x, -0.2, z), (0, 1, 0))
    for ph in ANGLES:  # cap rims and side hits at y == minimum / maximum
        for y in (lo, mx):
            q = (abs(y) * math.cos(ph), y, abs(y) * math.sin(ph))
            for o in ORIGINS[:3]:
                R.to(o, q)
            R.to((0.0, y - 0.5, 0.0), q)  # from inside the other nappe / below the cap
    for y in (lo, mx, 0.0, lo + 1e-12, mx - 1e-12):  # horizontal rays in the bound planes (d.y == 0: no caps)
        R.add((-3, y, 0), (1, 0, 0))
        R.add((-3, y, 0.2), (1, 0, 0.01))
    R.toward(rng, 60, 0.8, (0.0, -0.4, 0.0))
    # Hits outside the cone's box: a ray parallel to a generator s meets the infinite cone once, at q; from
    # o = q - T s the |a| < EPS path reports t = T / 2 (cone.rs:96-103), the midpoint, whenever its y lies inside the
    # bounds, however far from the cone that is.  Shadow pairs with the light just beyond and just before that point
    # (between it and any sphere around the cone), and pairs that look away from the cone.
    for ph, ps, qy, yb in ((0.5, 2.6, 3.0, -0.3), (2.0, 5.0, 4.0, 0.2), (4.0, 0.9, -5.0, -0.8), (5.5, 3.0, 6.0, 0.4),
                           (1.0, 4.2, -3.0, -0.5), (3.0, 0.2, 8.0, 0.1)):
        for sc in (1.0, 1e-3, 1e3):
            sg = 1.0 if qy > 0 else -1.0
            sdir = np.array([math.cos(ph), sg, math.sin(ph)])  # towards q along the generator's direction
            q = np.array([abs(qy) * math.cos(ps), qy, abs(qy) * math.sin(ps)])
            T = 2.0 * abs(qy - yb)
            o = q - T * sdir
            R.add(o, sdir * sc, keep=True)
            R.add(o + [0.0, 0.0, 1e-9], sdir * sc, keep=True)
            if sc == 1.0:
                for f in (0.45, 0.49, 0.51, 0.55, 0.7):
                    R.sh.append((o, o + f * T * sdir))
                    R.sh.append((o + f * T * sdir, o))
    for k, (o, d, t, enter) in enumerate(spurious_cone(mn, mx, 40) + spurious_cone(mn, mx, 20, shell=True, seed=12)):
        o, d = np.array(o), np.array(d)
        R.add(o, d * (1.0, 1e-3, 1e3)[k % 3], keep=True)
        R.sh.append((o, o + d * 0.5 * (t + enter)))  # a light between the entry and the sphere: shadowed
        R.sh.append((o, o + d * 0.9 * t))            # a light before the entry
        R.sh.append((o + d * 0.5 * (t + enter), o))  # and from the far side
    return R


@functools.lru_cache(maxsize=None)
def spurious_cone(mn, mx, n, shell=False, seed=11):
    """n object-space rays, found by a seeded search, parallel to a generator within rounding, whose line passes the
    cone's box and whose |a| < EPS entry t = -c / (2 b) > 0 (cone.rs:96-103) lies before the sphere around that box
    begins — and, with shell, outside the sphere of radius SHELL_R around the box's centre too, which the ray then
    enters first.  -> ((origin, direction, t of the entry, t where the box's sphere begins), ...)"""
    rng = np.random.default_rng(seed)
    lo = mn if math.isfinite(mn) else -2.0
    bmin, bmax = np.array([-1.0, lo, -1.0]), np.array([1.0, mx, 1.0])
    c0, r0 = 0.5 * (bmin + bmax), 0.5 * np.linalg.norm(bmax - bmin) * 1.01
    out = []
    for _ in range(400000):
        if len(out) == n:
            break
        ph = rng.uniform(0, 2 * math.pi)
        d = np.array([math.cos(ph), float(rng.choice([-1.0, 1.0])), math.sin(ph)])
        o = c0 + F._unit(rng) * rng.uniform(2.5, 6.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (bmin - o) / d, (bmax - o) / d
        if np.minimum(t1, t2).max() > np.maximum(t1, t2).min():
            continue  # the line misses the box
        b = 2.0 * o[0] * d[0] - 2.0 * o[1] * d[1] + 2.0 * o[2] * d[2]
        c = o[0] * o[0] - o[1] * o[1] + o[2] * o[2]
        if abs(b) < 1e-3:
            continue
        t = -c / (2.0 * b)
        y = o[1] + t * d[1]
        v = c0 - o
        p, dd = v @ d, d @ d
        disc = p * p - dd * (v @ v - r0 * r0)
        if not (t > 0.05 and lo < y < mx and disc > 0):
            continue
        enter = (p - math.sqrt(disc)) / dd
        if not t < enter - 0.2:
            continue
        if shell and not np.linalg.norm(o + t * d - c0) > SHELL_R + 0.1:
            continue
        out.append((tuple(o), tuple(d), t, enter))
    assert len(out) == n, (len(out), n)
    return tuple(out)


def cylinder_rays(mn, mx, rng):
    R = Rays()
    for dx in (0.0, 1e-6, 1e-5, 3e-3, 4e-3):  # axis-parallel: a = dx^2 against EPS
        for rr in (0.0, 0.5, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, 1.5):
            R.add((rr, mn - 2.0, 0.0), (dx, 1, 0), keep=True)
            R.add((0.0, mx + 2.0, rr), (dx, -1, 0), keep=True)
            R.add((rr * 0.6, 0.5 * (mn + mx), rr * 0.8), (dx, 1, 0))
    for ph in ANGLES:  # cap rims, hits at y == min and y == max
        for y in (mn, mx):
            q = (math.cos(ph), y, math.sin(ph))
            for o in ORIGINS:
                R.to(o, q)
            R.to((0.0, 0.5 * (mn + mx), 0.0), q)
    for y in (mn, mx, mn + 1e-12, mx - 1e-12, 0.3):  # horizontal rays in the bound planes
        R.add((-3, y, 0), (1, 0, 0))
        R.add((-3, y, 0.5), (1, 0, 0.01))
    for e in (0.0, 1e-15, -1e-15, 1e-9, -1e-9):  # side tangents: the discriminant about 0
        R.add((1.0 + e, 0.2, -3.0), (0, 0.1, 1))
        R.add((-3.0, mn - 1.0, 1.0 + e), (1, 0.5, 0))
        R.add((math.sqrt(0.5) * 2 + e, 0.0, 0.0), (-1, 0.2, 1))
    R.toward(rng, 25, 1.0, (0.0, 0.5 * (mn + mx), 0.0))
    return R


def cube_rays(rng):
    R = Rays()
    corners = [(x, y, z) for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]
    for c in corners:  # corners
        for o in ORIGINS[:3]:
            R.to(o, c)
        R.to((0.1, 0.2, -0.3), c)
    for s in (-0.5, 0.0, 0.7):  # edges
        for a, b in ((1.0, 1.0), (-1.0, 1.0), (1.0, -1.0)):
            for q in ((a, b, s), (a, s, b), (s, a, b)):
                R.to(ORIGINS[0], q)
                R.to(ORIGINS[1], q)
    for ax in range(3):  # axis-parallel rays lying in a face plane: 0 * inf in check_axis
        for f in (1.0, -1.0):
            for other in (0.3, 1.0, -1.0, 1.5):
                o, d = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                o[ax], o[(ax + 1) % 3], o[(ax + 2) % 3] = f, other, -3.0
                d[(ax + 2) % 3] = 1.0
                R.add(o, d)
    for m in (0.9, 0.95, 0.999999, 1.0, 1.000001, 1.05, 1.1):  # a direction component within +-10 % of EPS
        for sg in (1.0, -1.0):
            R.add((0.5, -0.2, -3.0), (sg * m * EPS, 0.3, 1.0), keep=True)
            R.add((1.0, -3.0, 0.4), (sg * m * EPS, 1.0, sg * m * EPS), keep=True)
            R.add((-3.0, 0.99, 1.0), (1.0, sg * m * EPS, 0.0), keep=True)
    for o in ((1.0, 0.2, 0.3), (0.0, 0.0, 0.0), (-1.0, -1.0, 0.0), (0.2, 1.0, -0.4), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0)):
        for d in ((1, 0, 0), (-1, 0.2, 0.1), (0, 1, 0), (0.3, -0.5, 1), (0, 0, -1)):  # origin on a face or inside
            R.add(o, d)
    R.toward(rng, 20, 1.0)
    return R


def torus_far_rays(r, rng):
    """origins 1e5 tube sizes away: the quartic's coefficients cancel to noise and find_roots_quartic returns roots
    anywhere along the line (torus.rs:37-95).  Rays towards the torus and rays looking away from it along lines through
    its box, with shadow pairs on both sides of the origin."""
    R = Rays()
    for _ in range(110):
        u = F._unit(rng)
        dist = float(rng.choice([3e4, 1e5, 3e5])) * r
        th = rng.uniform(0, 2 * math.pi)  # at the tube, or (one in five) anywhere around the box
        aim = np.array([math.cos(th), math.sin(th), 0.0]) + rng.uniform(-0.5, 0.5, 3) * r if rng.random() < 0.8 else \
            rng.uniform(-1, 1, 3) * [1.0 + r, 1.0 + r, r] * 3.0
        o = aim + u * dist
        d = (aim - o) / dist
        R.add(o, d, keep=True)        # towards the torus
        R.add(o, -d, keep=True)       # away from it, the line still through the box
        R.add(o, d * 1e3, keep=True)
        R.add(o, -d * 1e-3, keep=True)
        R.sh.append((o, o + d * dist * 2.0))
        R.sh.append((o, o - d * dist))
        R.sh.append((o, o + d * dist * 0.5))
        R.sh.append((aim - u * 3.0, o))
        R.sh.append((aim - u * 3.0, aim + u * 3.0))
    R.toward(rng, 140, 1.0)  # near rays, so that the battery still hits with a quarter of its rays
    return R


def torus_rays(r, rng):
    """the torus lies in the xy plane, its axis is z (torus.rs:23-31)"""
    R = Rays()
    for rho in (0.0, 1.0 - r, 1.0, 1.0 + r, 1.0 + 0.5 * r):  # axis rays
        for ph in (0.0, 0.5, 2.0, 4.0):
            x, y = rho * math.cos(ph), rho * math.sin(ph)
            R.add((x, y, -3.0), (0, 0, 1))
            R.add((x, y, 2.0 * r + 1.0), (0, 0, -1))
    for ph in ANGLES:  # in-plane rays through the centre
        c, s = math.cos(ph), math.sin(ph)
        R.add((-3 * c, -3 * s, 0.0), (c, s, 0))
        R.add((0.0, 0.0, 0.0), (c, s, 0))
        R.add((-3 * c, -3 * s, 0.5 * r), (c, s, 0))
    for e in (0.0, 1e-15, -1e-15, 1e-9, -1e-9):  # tangents to the outer rim, the inner rim and the top
        R.add((1.0 + r + e, -3.0, 0.0), (0, 1, 0))
        R.add((1.0 - r + e, -3.0, 0.0), (0, 1, 0))
        R.add((-3.0, 1.0 + r + e, 0.0), (1, 0, 0))
        R.add((1.0, -3.0, r + e), (0, 1, 0))
        R.add((-3.0, 0.0, r + e), (1, 0, 0))
        R.add((-3.0, 0.0, -r - e), (1, 0, 0.0))
        R.add((1.0 + r + e, 0.0, -3.0), (0, 0, 1))
    for o in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.3 * r), (math.sqrt(0.5), math.sqrt(0.5), -0.5 * r), (1.0 + 0.5 * r, 0, 0)):
        for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0.3, 0.2), (0.2, -1, 0.1), (-0.3, 0.1, -1)):  # inside the tube
            R.add(o, d)
    for _ in range(45):  # generic rays at the tube
        ph = rng.uniform(0, 2 * math.pi)
        q = np.array([math.cos(ph), math.sin(ph), 0.0]) + rng.uniform(-0.6, 0.6, 3) * r
        R.to(F._unit(rng) * rng.uniform(2.5, 6.0) * (1 + r), q)
    return R


def sphere_rays(rng):
    R = Rays()
    for e in (0.0, 1e-15, -1e-15, 1e-12, -1e-12, 1e-9, -1e-9):  # tangents: the discriminant about 0
        R.add((1.0 + e, -3.0, 0.0), (0, 1, 0))
        R.add((-3.0, 0.0, -1.0 - e), (1, 0, 0))
        R.add((math.sqrt(0.5) + e, -3.0, math.sqrt(0.5)), (0, 1, 0))
        R.add((3.0, 3.0, 1.0 + e), (-1, -1, 0))
        R.add((0.6 + e, 0.8, -2.0), (0, 0, 1))
    for o in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0.5, 0.5, 0.5)):  # inside and on the surface
        for d in ((0, 0, 1), (1, 0, 0), (0, -1, 0), (0.3, 0.2, -1)):
            R.add(o, d)
    R.toward(rng, 40, 1.0)
    return R


def plane_rays(rng):
    R = Rays()
    for m in (0.5, 0.9, 0.99, 0.999999, 1.0, 1.000001, 1.01, 1.1, 2.0, 10.0):  # |d.y| around EPS
        for sg in (1.0, -1.0):
            for o in ((0.0, 1.0, 0.0), (0.0, -1e-3, 0.0), (0.0, 0.0, 0.0), (5.0, 1e-4, -2.0), (1.0, -2.0, 1.0)):
                R.add(o, (1.0, sg * m * EPS, 0.3), keep=True)
    for o in ((0, 1, 0), (0, -1, 0), (0, 0, 0), (3, 1e-9, 2)):
        for d in ((0, -1, 0), (0, 1, 0), (1, -1, 1), (1, 0, 0), (0.2, -1e-3, 1)):
            R.add(o, d)
    R.toward(rng, 40, 1.0)
    return R


TRI = ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))  # p1, p2, p3; the second triangle shares p2-p3
TRI2 = ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.2, -1.0, 0.3))
TRI_N = ((0.0, 1.0, -1.0), (-1.0, 0.0, -1.0), (1.0, 0.0, -1.0))


def triangle_rays(rng):
    R = Rays()
    p1, p2, p3 = (np.array(p) for p in TRI)
    targets = [p1, p2, p3]
    for s in (0.0, 0.25, 0.5, 1.0 / 3.0, 0.9, 1.0):
        targets += [p1 + s * (p2 - p1), p1 + s * (p3 - p1), p2 + s * (p3 - p2)]  # v = 0, u = 0, u + v = 1 / shared edge
    for q in targets:
        for o in ((0.0, 0.5, -3.0), (2.0, 1.0, -2.0), (-0.5, -1.0, 4.0)):
            R.to(o, q)
        R.add(q + [0, 0, -2.0], (0, 0, 1))
    for m in (0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0):  # det around EPS: e1 x e2 = (0, 0, 2), det = -2 d.z
        for sg in (1.0, -1.0):
            dz = sg * m * EPS / 2.0
            R.add((-2.0, 0.4, -2.0 * dz), (1.0, 0.0, dz), keep=True)
            R.add((0.1, 3.0, -3.0 * dz), (0.0, -1.0, dz), keep=True)
            R.add((-2.0, -0.5, -2.0 * dz), (1.0, 0.0, dz), keep=True)  # the second triangle's plane is tilted
    R.toward(rng, 40, 0.6, (0.0, 0.2, 0.0))
    return R


def _xform(M, rng):
    return F._mul(M, M.scale(*[float(x) for x in rng.uniform(0.4, 2.5, 3)]), F._rot(M, rng),
                  M.shear(*[float(x) for x in rng.uniform(-0.6, 0.6, 6)]),
                  M.translate(*[float(x) for x in rng.uniform(-2, 2, 3)]))


def _np4(m):
    return np.array(m, float).reshape(4, 4)


class Battery:
    """P: the scene on both sides; o, d: (N, 3) world rays (shuffled edge rays padded to a multiple of 64, then the
    fans); n_edge: edge rays; shadow_p, shadow_l: point / light pairs; objs: builder ids of the featured leaves."""


def _finish(B, P, fwd, R, rng, centre_w, extent):
    """object-space rays -> world space, the shuffled block, the fans, the shadow pairs"""
    o = np.array(R.o) @ fwd[:3, :3].T + fwd[:3, 3]
    d = np.array(R.d) @ fwd[:3, :3].T
    B.P, B.n_edge = P, len(o)
    B.edge_o, B.edge_d = o, d
    perm = rng.permutation(len(o))
    pad = (-len(o)) % 64
    idx = np.concatenate([perm, perm[:pad]])
    fo, fd = [], []
    for i in range(len(o)):
        di = d[i]
        n = np.linalg.norm(di)
        e1 = np.cross(di, [1.0, 0.0, 0.0] if abs(di[0]) < 0.9 * n else [0.0, 1.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(di, e1) / n
        j, k = np.meshgrid(np.arange(8) - 3.5, np.arange(8) - 3.5)
        off = (j.reshape(-1, 1) * e1 + k.reshape(-1, 1) * e2) * (FAN_STEP * n)
        fo.append(np.repeat(o[i][None], 64, 0))
        fd.append(di + off)
    B.o = np.concatenate([o[idx]] + fo)
    B.d = np.concatenate([d[idx]] + fd)
    B.fan_start = len(idx)
    assert B.fan_start % 64 == 0 and np.isfinite(B.o).all() and np.isfinite(B.d).all()
    # shadow pairs from the same geometry: the edge rays' segments (long ones cross the shape, short ones stop before
    # it; rim rays graze), surface points (t = 1 targets) towards outside lights, and outside points towards lights
    # on the surface
    sp, sl = [], []
    for i in range(len(o)):
        n = np.linalg.norm(d[i])
        reach = np.linalg.norm(o[i] - centre_w) + 2.0 * extent
        kind = i % 4
        if kind == 0:
            sp.append(o[i]), sl.append(o[i] + d[i] * (reach / n))  # through the shape
        elif kind == 1:
            sp.append(o[i]), sl.append(o[i] + d[i] * (0.2 * max(np.linalg.norm(o[i] - centre_w) - extent, 0.1) / n))
        elif kind == 2:
            sp.append(o[i] + d[i] * 1.5), sl.append(o[i] - d[i] * (reach / n))  # back through the t = 1 target
        else:
            sp.append(o[i] - d[i] * (0.5 * reach / n)), sl.append(o[i] + d[i])  # a light on the t = 1 target
    for a, b in R.sh:
        sp.append(np.array(a, float) @ fwd[:3, :3].T + fwd[:3, 3])
        sl.append(np.array(b, float) @ fwd[:3, :3].T + fwd[:3, 3])
    B.shadow_p, B.shadow_l = np.array(sp), np.array(sl)
    return B


def leaf_names():
    names = [f"{k}-{p}" for k in ("sphere", "plane", "triangle", "smooth_triangle", "cube", "cylinder") for p in PLACEMENTS]
    names += [f"cone_closed-{p}" for p in PLACEMENTS] + ["cone_open-ident", "cone_onesided-xform", "cone_open-group"]
    names += [f"torus_{r}-ident" for r in TORUS_RADII] + ["torus_0.25-xform", "torus_0.25-group", "torus_0.99-xform"]
    names += ["coneshell_closed-igroup", "torusfar_0.25-ident", "torusfar_0.25-group"]
    return names


CSG_NAMES = ("csg_coincident", "csg_nested", "csg_full", "csg_glass")


def build(name):
    """-> Battery for one of leaf_names() / CSG_NAMES"""
    import zlib

    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in CSG_NAMES:
        return _build_csg(name, rng)
    kind, place = name.split("-")
    P = F.Pair()
    M = P.M
    B = Battery()
    B.name = name
    P.light((-8.0, 9.0, -7.0))
    tr = M.identity() if place in ("ident", "igroup") else _xform(M, rng)
    parent, fwd = -1, _np4(tr)
    if place == "igroup":  # an identity group: its box is the leaf's
        parent = P.obj("group", M.identity())
    if place == "group":
        g = F._mul(M, M.scale(1.3, 0.7, 1.1), M.shear(0.5, -0.3, 0.2, 0.4, -0.6, 0.1), M.rotate("y", 0.4),
                   M.translate(0.5, -0.4, 0.8))
        parent = P.obj("group", g)
        fwd = _np4(g) @ fwd
    col = (0.8, 0.5, 0.3)
    extent = 1.5
    if kind == "sphere":
        B.objs = [P.obj("sphere", tr, MAT, col, parent)]
        R = sphere_rays(rng)
    elif kind == "plane":
        B.objs = [P.obj("plane", tr, MAT, col, parent)]
        R = plane_rays(rng)
    elif kind in ("triangle", "smooth_triangle"):
        nr = None if kind == "triangle" else [tuple(float(x) for x in np.array(n) / np.linalg.norm(n)) for n in TRI_N]
        B.objs = [P.triangle(*TRI, MAT, col, parent=parent, normals=nr, tr=None if place == "ident" else tr),
                  P.triangle(*TRI2, MAT, (0.2, 0.6, 0.9), parent=parent, normals=nr, tr=None if place == "ident" else tr)]
        R = triangle_rays(rng)
    elif kind == "cube":
        B.objs = [P.obj("cube", tr, MAT, col, parent)]
        R = cube_rays(rng)
        extent = 2.0
    elif kind == "cylinder":
        B.objs = [P.cylinder(tr, MAT, col, -1.0, 2.0, True, parent)]
        R = cylinder_rays(-1.0, 2.0, rng)
        extent = 2.5
    elif kind.startswith("cone_"):
        mn, mx, closed = CONES[kind[5:]]
        B.objs = [P.cone(tr, MAT, col, mn, mx, closed, parent)]
        B.box = ((-1.0, mn if math.isfinite(mn) else -2.0, -1.0), (1.0, mx, 1.0))
        R = cone_rays(mn, mx, rng)
    elif kind.startswith("coneshell_"):  # a sphere around the cone, between its far entries and its box
        mn, mx, closed = CONES[kind[10:]]
        B.objs = [P.cone(tr, MAT, col, mn, mx, closed, parent)]
        B.box = ((-1.0, mn, -1.0), (1.0, mx, 1.0))
        R = cone_rays(mn, mx, rng)
        P.obj("sphere", F._mul(M, M.scale(SHELL_R, SHELL_R, SHELL_R), M.translate(0.0, 0.5 * ((mn if math.isfinite(mn) else -2.0) + mx), 0.0)),
              MAT, (0.4, 0.4, 0.4), parent)  # a sibling, in the group's space
    elif kind.startswith("torus_"):
        r = float(kind[6:])
        B.objs = [P.torus(tr, MAT, col, r, parent)]
        R = torus_rays(r, rng)
        extent = 1.0 + r
    elif kind.startswith("torusfar_"):
        r = float(kind[9:])
        B.objs = [P.torus(tr, MAT, col, r, parent)]
        B.box = ((-1.0 - r, -1.0 - r, -r), (1.0 + r, 1.0 + r, r))
        R = torus_far_rays(r, rng)
        extent = 1.0 + r
    else:
        raise ValueError(name)
    centre = fwd[:3, 3]
    scale = float(np.linalg.norm(fwd[:3, :3], 2))
    return _finish(B, P, fwd, R, rng, centre, extent * scale)


def _build_csg(name, rng):
    P = F.Pair()
    M = P.M
    B = Battery()
    B.name = name
    P.light((-8.0, 9.0, -7.0))
    I = M.identity()
    R = Rays()
    B.objs = []

    def leaf(kind, tr, parent, m7=MAT):
        col = F._color(rng)
        if kind == "cylinder":
            i = P.cylinder(tr, m7, col, -1.0, 1.0, True, parent)
        elif kind == "cone":
            i = P.cone(tr, m7, col, -1.0, 0.0, True, parent)
        elif kind == "torus":
            i = P.torus(tr, m7, col, 0.25, parent)
        else:
            i = P.obj(kind, tr, m7, col, parent)
        B.objs.append(i)
        return i

    if name == "csg_coincident":  # equal t from the left and the right child: the stable left ++ right order decides
        x = -6.0
        for op in ("union", "intersection", "difference"):
            for kinds, shift in ((("cube", "cube"), 2.0), (("cube", "cube"), 1.0), (("sphere", "sphere"), 0.0),
                                 (("cube", "cylinder"), 0.0)):
                c = P.csg(op, M.translate(x, 0.0, 0.0))
                leaf(kinds[0], I, c)
                leaf(kinds[1], M.translate(shift, 0.0, 0.0), c)
                for o, d in (((-3, 0.2, 0.3), (1, 0, 0)), ((5, 0.2, 0.3), (-1, 0, 0)), ((0.5, 0.2, 0.3), (1, 0, 0)),
                             ((1.0, 0.2, 0.3), (1, 0, 0)), ((0.3, -3, 0.2), (0, 1, 0)), ((1.0, -3, 0.2), (0, 1, 0)),
                             ((0.2, 0.3, -3), (0, 0, 1)), ((1.5, 0.0, -3), (0, 0, 1)), ((-3, 1.0, 0.0), (1, 0, 0)),
                             ((0.0, 0.0, 0.0), (0.3, 0.2, 1)), ((1.5, 0.1, 0.1), (-1, 0.1, 0.2))):
                    R.add(np.array(o, float) + [x, 0, 0], d)
                x += 4.5
        centre, extent = np.zeros(3), 30.0
    elif name == "csg_nested":  # depth 3 inside a sheared group, a group as a child, cone / cylinder / torus children
        g = P.obj("group", F._mul(M, M.shear(0.3, 0.0, -0.2, 0.0, 0.1, 0.4), M.rotate("y", 0.3)))
        c1 = P.csg("union", M.translate(0.0, 0.2, 0.0), g)
        c2 = P.csg("difference", I, c1)
        c3 = P.csg("intersection", I, c2)
        leaf("sphere", M.scale(1.3, 1.3, 1.3), c3)
        leaf("cube", I, c3)
        leaf("cylinder", F._mul(M, M.scale(0.5, 2.0, 0.5)), c2)
        gg = P.obj("group", M.translate(1.2, 0.0, 0.0), parent=c1)
        leaf("torus", M.rotate("x", 0.5), gg)
        leaf("cone", F._mul(M, M.scale(0.8, 1.5, 0.8), M.translate(0.0, 1.0, 0.5)), gg)
        for o, d in (((0, 0, 0), (0, 1, 0)), ((0, 0.2, 0), (1, 0, 0)), ((0.6, 0.3, 0.6), (0, 0, -1)), ((1.2, 0, 0), (0, 0, 1)),
                     ((0, -4, 0), (0, 1, 0)), ((0.25, -4, 0.25), (0, 1, 0)), ((-4, 0.2, 0.0), (1, 0, 0))):
            R.add(o, d)
        R.toward(rng, 160, 1.6, (0.5, 0.2, 0.0))
        centre, extent = np.zeros(3), 3.0
    elif name == "csg_full":  # eight four-entry leaves under one CSG: exactly RR_MAX_CSG_ENTRIES possible entries
        kinds = ("cone", "cylinder", "torus", "cone", "cylinder", "torus", "cone", "cylinder")
        top = P.csg("union", I)
        k = 0
        for a in range(2):
            mid = P.csg("union" if a == 0 else "difference", I, top)
            for b in range(2):
                low = P.csg(("union", "intersection")[b] if a == 0 else "union", I, mid)
                for c in range(2):
                    leaf(kinds[k], F._mul(M, M.scale(1.0, 1.0 + 0.1 * k, 1.0), M.rotate("x", 0.3 * k),
                                          M.translate(0.15 * (k - 3.5), 0.0, 0.1 * (k % 3))), low)
                    k += 1
        for o, d in (((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (1, 0, 0)), ((-4, 0, 0), (1, 0, 0)), ((-4, 0.1, 0.05), (1, 0, 0)),
                     ((0, -4, 0), (0, 1, 0)), ((0.9, 0, -4), (0, 0, 1))):
            R.add(o, d)
        R.toward(rng, 170, 1.3)
        centre, extent = np.zeros(3), 3.0
    else:  # csg_glass: a glass CSG next to (and overlapping) a glass sphere, for n1 and n2
        c = P.csg("difference", I)
        leaf("cube", I, c, GLASS)
        leaf("sphere", F._mul(M, M.scale(1.2, 1.2, 1.2), M.translate(0.5, 0.5, -0.5)), c, (0.1, 0.5, 0.9, F.SHININESS, 0.0, 0.8, 2.0))
        leaf("sphere", M.translate(1.4, 0.0, 0.0), -1, (0.1, 0.5, 0.9, F.SHININESS, 0.1, 1.0, 1.33))
        P.obj("plane", M.translate(0.0, -1.5, 0.0), MAT, (0.5, 0.5, 0.5))
        for o in ((0, 0, 0), (-0.5, -0.5, 0.5), (1.0, 0, 0), (1.2, 0.1, 0.0), (0.7, 0.0, 0.3), (2.0, 0.0, 0.0)):
            for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0.2, 0.1, 1), (0.5, -0.3, -1)):
                R.add(o, d)
        R.toward(rng, 150, 1.5, (0.6, 0.0, 0.0))
        centre, extent = np.zeros(3), 3.0
    return _finish(B, P, np.eye(4), R, rng, centre, extent)


def entry_counts(B):
    """how many entries each edge ray's local_intersect leaves in the oracle's list, per featured leaf"""
    counts = []
    for o, d in zip(B.edge_o, B.edge_d):
        xs = B.P.o.intersect(tuple(o), tuple(d))
        for i in B.objs:
            counts.append(sum(1 for x in xs if x[1] == B.P.ids[i]))
    return counts


# ---------------------------------------------------------------------------------------------------------------
# Pattern points: rays straight down onto a plane that carries each pattern kind (ambient 1, diffuse and specular 0:
# the colour is the pattern's), at the points where stripe / checker / ring / gradient / noise branch.
FLAT = (1.0, 0.0, 0.0, F.SHININESS, 0.0, 0.0, 1.0)
A_COL, B_COL = (0.9, 0.2, 0.1), (0.1, 0.3, 0.8)
PATTERN_NAMES = ("stripe", "gradient", "ring", "checker", "blend", "perturbed", "noise", "nested", "octaves",
                 "transformed")


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, math.inf if k > 0 else -math.inf)
    return float(x)


def pattern_points():
    xs = []
    for n in (0, 1, 2, 3, -1, -2, -3, -5, 7, 1024, -1023):
        for k in (-2, -1, 0, 1, 2):
            xs.append(_ulps(float(n), k))
    xs += [-0.0, 0.5, -0.5, 1.5, -1.5, 1e9, -1e9, 1e9 + 1.0, 2.0 ** 31, 2.0 ** 31 + 1.0, -(2.0 ** 31) - 2.0, 3e9, -3e9,
           2.0 ** 32 + 1.0, 1e12, -1e12 - 1.0]
    pts = [(x, 0.0) for x in xs] + [(0.0, x) for x in xs] + [(x, -x) for x in xs[::3]] + [(x, 2.0) for x in xs[::4]]
    for r in (1, 2, 3, 5):  # integer radii for ring: 3-4-5 style points and axis points
        pts += [(float(r), 0.0), (0.0, -float(r)), (0.6 * r, 0.8 * r), (-0.8 * r, 0.6 * r)]
    return pts


def build_pattern(name, alone):
    """-> (Pair, origins, directions, builder id of the plane, its pattern Pat).  alone: the plane is the only
    top-level object (the scalar uniform-hit path); otherwise spheres and a group stand beside it."""
    P = F.Pair()
    M = P.M
    P.light((-10.0, 10.0, -10.0))
    a, b = P.pat("solid", A_COL), P.pat("solid", B_COL)
    if name in ("stripe", "gradient", "ring", "checker"):
        pat = P.pat(name, a=a, b=b)
    elif name == "blend":
        pat = P.pat("blend", a=P.pat("stripe", a=a, b=b), b=P.pat("stripe", a=a, b=b, transform=M.rotate("y", math.pi / 2)),
                    scale=0.3)
    elif name == "perturbed":
        pat = P.pat("perturbed", a=P.pat("checker", a=a, b=b), scale=0.2, octaves=3, persistence=0.5)
    elif name == "noise":
        pat = P.pat("noise", a=a, b=b, scale=1.0, octaves=2, persistence=2.0)
    elif name == "nested":  # a blend of a perturbed checker and a noise, each with its own transform
        pc = P.pat("perturbed", a=P.pat("checker", a=a, b=b, transform=M.scale(0.5, 0.5, 0.5)), scale=0.35, octaves=4,
                   persistence=0.3, transform=F._mul(M, M.rotate("y", 0.3), M.translate(0.1, 0.0, -0.2)))
        nz = P.pat("noise", a=P.pat("ring", a=a, b=b), b=P.pat("gradient", a=b, b=a), scale=1.5, octaves=5, persistence=1.0,
                   transform=M.scale(0.7, 1.0, 1.3))
        pat = P.pat("blend", a=pc, b=nz, scale=0.6, transform=M.shear(0.2, 0.0, 0.0, 0.0, 0.1, 0.0))
    elif name == "octaves":  # octaves 1 to 8 and persistence 0.3, 1, 2 as stripes of noise selected by a checker tree
        mixes = []
        for oc in range(1, 9):
            nz = P.pat("noise", a=a, b=b, scale=1.0, octaves=oc, persistence=(0.3, 1.0, 2.0)[oc % 3])
            pt = P.pat("perturbed", a=P.pat("stripe", a=a, b=b), scale=0.4, octaves=oc, persistence=(2.0, 0.3, 1.0)[oc % 3])
            mixes.append(P.pat("blend", a=nz, b=pt, scale=0.5))
        while len(mixes) > 1:  # a balanced tree of blends: seven levels with the leaves, under RR_MAX_PATTERN_DEPTH
            mixes = [P.pat("blend", a=mixes[k], b=mixes[k + 1], scale=0.5) for k in range(0, len(mixes), 2)]
        pat = mixes[0]
    elif name == "transformed":
        pat = P.pat("checker", a=P.pat("stripe", a=a, b=b, transform=M.scale(0.25, 1.0, 1.0)),
                    b=P.pat("gradient", a=a, b=b, transform=M.rotate("y", 1.0)),
                    transform=F._mul(M, M.scale(0.5, 0.5, 0.5), M.translate(0.25, 0.0, 0.0)))
    else:
        raise ValueError(name)
    plane = P.obj("plane", M.identity(), FLAT, pat)
    if not alone:
        P.obj("sphere", M.translate(0.3, 4.0, 0.2), FLAT, (0.2, 0.9, 0.2))  # above the rays' origins
        g = P.obj("group", M.translate(-3.0, 6.0, 1.0))
        P.obj("sphere", M.scale(0.5, 0.5, 0.5), FLAT, (0.2, 0.2, 0.9), g)
    pts = pattern_points()
    if name in ("perturbed", "noise", "nested", "octaves"):
        pts = pts + [(x + 0.37, z - 0.21) for x, z in pts[::2]]  # off the lattice, where the noise is not zero
    o = np.array([(x, 1.0, z) for x, z in pts])
    d = np.tile([0.0, -1.0, 0.0], (len(o), 1))
    return P, o, d, plane, pat


# textures of 1 x 1, 2 x 3 and 5 x 1 texels on every shape kind, hit where u and v reach 0 and 1
def textures():
    rng = np.random.default_rng(77)
    return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for w, h in ((1, 1), (2, 3), (5, 1))]


def build_textured(kind, tex_index):
    """-> (Pair, origins, directions): one textured shape at the origin and rays at its uv edges.  The directions are
    normalised: the eye vector's length goes through the specular power (inf * 0 would turn every colour into NaN)."""
    P = F.Pair()
    M = P.M
    P.light((-10.0, 10.0, -10.0))
    pat = P.pat("texture", a=P.tex(textures()[tex_index]))
    R = Rays()
    I = M.identity()
    rng = np.random.default_rng(5)
    if kind == "sphere":
        P.obj("sphere", I, FLAT, pat)
        for q in ((0, 1, 0), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (-1, 0, 1e-17), (-1, 0, -1e-17), (0, 0, 1), (0, 0, -1)):
            R.to(np.array(q, float) * 3.0, q)  # poles, the seam (theta = +-pi) and its neighbours
            R.to(np.array(q, float) * 3.0 + [0.0, 0.0, 1e-9], q)
        R.toward(rng, 30)
    elif kind == "plane":
        P.obj("plane", I, FLAT, pat)
        for x, z in pattern_points()[:80]:
            R.add((x, 1.0, z), (0, -1, 0))
    elif kind == "cube":
        P.obj("cube", I, FLAT, pat)
        for a in (-1.0, 1.0):
            for b in (-1.0, 1.0):
                for s in (-1.0, -0.3, 0.0, 0.5, 1.0):  # edges and corners, where two faces tie
                    for q in ((a, b, s), (a, s, b), (s, a, b)):
                        R.to((a * 3.0, b * 2.5 + 0.1, s + 2.0), q)
        R.toward(rng, 20)
    elif kind in ("cylinder", "cone"):
        if kind == "cylinder":
            P.cylinder(I, FLAT, pat, 0.0, 1.0, True)
            lo, hi, rad = 0.0, 1.0, (1.0, 1.0)
        else:
            P.cone(I, FLAT, pat, -1.0, -0.25, True)
            lo, hi, rad = -1.0, -0.25, (1.0, 0.25)
        for ph in ANGLES + (math.pi - 1e-16, -math.pi):
            for y, r in ((lo, rad[0]), (hi, rad[1])):  # the cap and side boundary
                q = (r * math.cos(ph), y, r * math.sin(ph))
                R.to((3 * math.cos(ph), y + 0.5, 3 * math.sin(ph)), q)
                R.to((0.1, y + (2.0 if y == hi else -2.0), 0.1), q)
                R.add((q[0] * 0.5, y + (2.0 if y == hi else -2.0), q[2] * 0.5), (0, -1 if y == hi else 1, 0))
        R.toward(rng, 20, 0.5, (0.0, 0.5 * (lo + hi), 0.0))
    elif kind == "triangle":
        P.triangle(*TRI, FLAT, pat)
        p1, p2, p3 = (np.array(p) for p in TRI)
        for q in (p1, p2, p3, 0.5 * (p1 + p2), 0.5 * (p1 + p3), 0.5 * (p2 + p3), (p1 + p2 + p3) / 3.0):
            R.add(q + [0, 0, -2.0], (0, 0, 1))
            R.to((0.3, 0.2, -3.0), q)
    elif kind == "torus":
        P.torus(I, FLAT, pat, 0.25)
        for ph in ANGLES + (math.pi - 1e-16, -math.pi):
            for q in ((1.25 * math.cos(ph), 1.25 * math.sin(ph), 0.0), (0.75 * math.cos(ph), 0.75 * math.sin(ph), 0.0),
                      (math.cos(ph), math.sin(ph), 0.25), (math.cos(ph), math.sin(ph), -0.25)):
                R.to((2.5 * math.cos(ph), 2.5 * math.sin(ph), 3.0 * (1 if q[2] >= 0 else -1)), q)
    else:
        raise ValueError(kind)
    d = np.array(R.d)
    return P, np.array(R.o), d / np.linalg.norm(d, axis=1)[:, None]


TEXTURED_KINDS = ("sphere", "plane", "cube", "cylinder", "cone", "triangle", "torus")
