"""Seeded adversarial scenes for the exact-cull fuzz (tests/test_gpu_fuzz.py, tests/test_fuzz_host.py).

Every scene is built twice from the same numbers: through the product's SceneBuilder (C ABI descriptor)
and through the oracle (the CPU restatement of the reference, test infrastructure).  The kernels cull
nodes with conservative f32 tests (bundle cones, lane line tests, the far-origin shift, inflated cull
spheres; DESIGN.md §3.5, device_core.inc, flatten.cpp make_cull) whose slacks are hand-derived; the
reference tests every primitive for every ray (scene.rs:97-106).  These scenes go where the benchmark
configs never do:

  scales    spheres from 1e-3 to 1e4 units, huge ones far away, a floor
  far_cam   the camera 1e3-1e5 units outside the scene's bounding sphere, narrow field of view (the
            far-origin shift of the bundles, device_core.inc make_bundle)
  tiny_far  objects of 1e-3 units 1e3-1e5 away, the camera aimed at them with a tiny field of view
            (near-parallel bundles, cull radii at the edge of f32 resolution)
  groups    nested groups with non-uniform scale and shear holding spheres, triangles and smooth
            triangles (ancestor chains, group AABBs, transformed cull spheres)
  grazing   planes tilted a few milli-radians off the view direction, camera just above a floor
  lights    lights inside / next to surfaces, reflective everywhere, glass (the n1/n2 walk's two-sided
            culls), recursion depth 5
  many      600-900 spheres of mixed scale (culls too large for LDS: the global-memory cull kernels)
  general   cubes and cylinders inside sheared groups (the G = 2 kernels)

build_area, build_own, build_general and build_area_mix (area lights across every kernel variant, light mix and level)
follow the same pattern with families of their own.

Shininess is 200 everywhere so the specular power takes the correctly rounded path:
any difference from the oracle is then a walk / cull error, never a last-ulp `pow`.
"""
import math

import numpy as np

CATEGORIES = ["scales", "far_cam", "tiny_far", "groups", "grazing", "lights", "many", "general"]
SHININESS = 200.0


class Pat(tuple):
    """(builder pattern id, oracle pattern id) of one pattern tree node; accepted wherever a colour is."""


class Pair:
    """One scene on both sides: product SceneBuilder + oracle.Oracle, identical inputs."""

    def __init__(self):
        import oracle
        import rray_amd as R

        self.b = R.SceneBuilder()
        self.o = oracle.Oracle()
        self.M = oracle.Oracle.mat
        self.ids = {}  # builder id -> oracle id
        self.log = []  # printable description (failing seeds print it)

    def _mat(self, m7, color):
        if isinstance(color, Pat):  # a pattern tree built with pat(): (builder id, oracle id)
            return color
        pb = self.b.pattern("solid", color=color)
        po = self.o.pattern("solid", color=color)
        return pb, po

    def obj(self, kind, tr, m7=None, color=(0.8, 0.5, 0.3), parent=-1):
        po_parent = self.ids[parent] if parent >= 0 else -1
        if kind == "group":
            bid = self.b.group(transform=tr, parent=parent)
            oid = self.o.add("group", po_parent, tr)
        else:
            pb, po = self._mat(m7, color)
            if kind == "sphere":
                bid = self.b.sphere(transform=tr, material=m7, pattern=pb, parent=parent)
            elif kind == "plane":
                bid = self.b.plane(transform=tr, material=m7, pattern=pb, parent=parent)
            elif kind == "cube":
                bid = self.b.cube(transform=tr, material=m7, pattern=pb, parent=parent)
            else:
                raise ValueError(kind)
            oid = self.o.add(kind, po_parent, tr, m7, po)
        self.ids[bid] = oid
        self.log.append(f"{kind} id={bid} parent={parent} tr={np.round(tr, 6).tolist()} mat={m7}")
        return bid

    def cylinder(self, tr, m7, color, minimum, maximum, closed, parent=-1):
        pb, po = self._mat(m7, color)
        bid = self.b.cylinder(minimum, maximum, closed, transform=tr, material=m7, pattern=pb, parent=parent)
        oid = self.o.add("cylinder", self.ids[parent] if parent >= 0 else -1, tr, m7, po)
        self.o.set_shape_params(oid, minimum, maximum, closed)
        self.ids[bid] = oid
        self.log.append(f"cylinder id={bid} parent={parent} [{minimum},{maximum}] closed={closed} "
                        f"tr={np.round(tr, 6).tolist()} mat={m7}")
        return bid

    def cone(self, tr, m7, color, minimum, maximum, closed, parent=-1):
        pb, po = self._mat(m7, color)
        bid = self.b.cone(minimum, maximum, closed, transform=tr, material=m7, pattern=pb, parent=parent)
        oid = self.o.add("cone", self.ids[parent] if parent >= 0 else -1, tr, m7, po)
        self.o.set_shape_params(oid, minimum, maximum, closed)
        self.ids[bid] = oid
        self.log.append(f"cone id={bid} parent={parent} [{minimum},{maximum}] closed={closed} "
                        f"tr={np.round(tr, 6).tolist()} mat={m7}")
        return bid

    def torus(self, tr, m7, color, minor_radius, parent=-1):
        pb, po = self._mat(m7, color)
        bid = self.b.torus(minor_radius, transform=tr, material=m7, pattern=pb, parent=parent)
        oid = self.o.add("torus", self.ids[parent] if parent >= 0 else -1, tr, m7, po)
        self.o.set_shape_params(oid, minor_radius, math.inf, False)  # scene_builder_yaml.rs:350-353
        self.ids[bid] = oid
        self.log.append(f"torus id={bid} parent={parent} r={minor_radius} tr={np.round(tr, 6).tolist()} mat={m7}")
        return bid

    def csg(self, op, tr, parent=-1):
        """A CSG node; its left then its right child are the next two objects added with parent=<this id>."""
        bid = self.b.csg(op, transform=tr, parent=parent)
        oid = self.o.add_csg(op, self.ids[parent] if parent >= 0 else -1, tr)
        self.ids[bid] = oid
        self.log.append(f"csg {op} id={bid} parent={parent} tr={np.round(tr, 6).tolist()}")
        return bid

    def pat(self, kind, color=(0.0, 0.0, 0.0), a=None, b=None, scale=0.5, transform=None, octaves=1, persistence=1.0):
        """One pattern tree node on both sides; a and b are Pat pairs (for "texture", a is a tex() pair)."""
        tr = transform if transform is not None else self.M.identity()
        a, b = a or (-1, -1), b or (-1, -1)
        pb = self.b.pattern(kind, color=color, a=a[0], b=b[0], scale=scale, transform=tr, octaves=octaves,
                            persistence=persistence)
        po = self.o.pattern(kind, color=color, a=a[1], b=b[1], scale=scale, transform=tr)
        if kind in ("perturbed", "noise"):
            self.o.set_noise(po, octaves, persistence)
        self.log.append(f"pattern {kind} ids=({pb},{po}) color={color} a={tuple(a)} b={tuple(b)} scale={scale} "
                        f"octaves={octaves} persistence={persistence} tr={np.round(tr, 6).tolist()}")
        return Pat((pb, po))

    def tex(self, rgba):
        """An RGBA8 image (height, width, 4) on both sides -> (builder index, oracle index)."""
        return Pat((self.b.texture(rgba), self.o.add_texture(rgba)))

    def triangle(self, p1, p2, p3, m7, color, parent=-1, normals=None, tr=None):
        pb, po = self._mat(m7, color)
        op = self.ids[parent] if parent >= 0 else -1
        if normals is None:
            bid = self.b.triangle(p1, p2, p3, transform=tr, material=m7, pattern=pb, parent=parent)
            oid = self.o.add_triangle(p1, p2, p3, op)
        else:
            bid = self.b.smooth_triangle(p1, p2, p3, *normals, transform=tr, material=m7, pattern=pb, parent=parent)
            oid = self.o.add_smooth_triangle(p1, p2, p3, *normals, parent=op)
        if tr is not None:
            self.o.set_transform(oid, tr)
        self.o.set_material(oid, m7, po)
        self.ids[bid] = oid
        self.log.append(f"{'smooth_' if normals else ''}triangle id={bid} parent={parent} "
                        f"p={np.round([p1, p2, p3], 6).tolist()} mat={m7}")
        return bid

    def light(self, pos, color=(1.0, 1.0, 1.0)):
        pos = tuple(float(x) for x in pos)
        self.b.point_light(pos, color)
        self.o.point_light(pos, color)
        self.log.append(f"point light {pos}")

    def area_light(self, corner, u, v, level, color=(1.0, 1.0, 1.0)):
        corner, u, v = (tuple(float(x) for x in a) for a in (corner, u, v))
        self.b.area_light(corner, u, v, color, int(level))
        self.o.area_light(corner, u, v, color, int(level))
        self.log.append(f"area light corner={corner} u={u} v={v} level={level}")


def _mul(M, *ts):
    """ts applied first to last (the YAML transform list order, scene_builder_yaml.rs:218-224)."""
    m = M.identity()
    for t in ts:
        m = M.multiply(t, m)
    return m


def _material(rng, reflective_p=0.3, glass_p=0.0):
    refl = float(rng.choice([0.0, 0.3, 0.5, 0.9])) if rng.random() < reflective_p else 0.0
    transp, ri = (0.0, 1.0)
    if rng.random() < glass_p:
        transp, ri = float(rng.choice([0.5, 0.9, 1.0])), float(rng.choice([1.33, 1.5, 2.4]))
    return (float(rng.uniform(0.05, 0.3)), float(rng.uniform(0.3, 0.9)), float(rng.uniform(0.0, 0.9)), SHININESS,
            refl, transp, ri)


def _color(rng):
    return tuple(float(round(x, 3)) for x in rng.uniform(0.05, 1.0, 3))


def _rot(M, rng):
    return _mul(M, M.rotate("x", float(rng.uniform(-math.pi, math.pi))), M.rotate("y", float(rng.uniform(-math.pi, math.pi))),
                M.rotate("z", float(rng.uniform(-math.pi, math.pi))))


def _logu(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def build(seed):
    """-> (Pair, camera spec dict(from_, to, up, fov), max_depth, category)."""
    rng = np.random.default_rng(10_000 + seed)
    cat = CATEGORIES[seed % len(CATEGORIES)]
    P = Pair()
    M = P.M
    depth = 5
    frm, to, fov = (0.0, 3.0, -30.0), (0.0, 0.0, 0.0), 1.0

    def sphere_at(c, s, m7=None, parent=-1, aniso=False):
        sc = (s * rng.uniform(0.2, 5.0), s, s * rng.uniform(0.2, 5.0)) if aniso else (s, s, s)
        tr = _mul(M, M.scale(*sc), _rot(M, rng), M.translate(*[float(x) for x in c])) if aniso else \
            _mul(M, M.scale(*sc), M.translate(*[float(x) for x in c]))
        return P.obj("sphere", tr, m7 or _material(rng), _color(rng), parent)

    if cat == "scales":
        P.obj("plane", M.translate(0.0, -2.0, 0.0), _material(rng), _color(rng))
        for _ in range(int(rng.integers(40, 160))):
            s = _logu(rng, 1e-3, 10.0)
            sphere_at(rng.uniform(-15, 15, 3) * [1, 0.3, 1] + [0, 2, 0], s, aniso=rng.random() < 0.3)
        for _ in range(int(rng.integers(2, 6))):  # huge and far: 1e2-1e4 units at 1e3-1e5
            d = _logu(rng, 1e3, 1e5)
            s = min(_logu(rng, 1e2, 1e4), 0.5 * d)
            dirv = _unit(rng) * [1, 0.3, 1] + [0, 0.1, 1.0]
            sphere_at(dirv / np.linalg.norm(dirv) * d, s)
        P.light(rng.uniform(-20, 20, 3) + [0, 25, -10])
        frm, fov = (float(rng.uniform(-5, 5)), float(rng.uniform(1, 8)), -30.0), float(rng.uniform(0.6, 1.3))
    elif cat == "far_cam":
        for _ in range(int(rng.integers(30, 120))):
            sphere_at(rng.uniform(-5, 5, 3), _logu(rng, 0.05, 2.0), aniso=rng.random() < 0.2)
        if rng.random() < 0.5:
            P.obj("plane", M.translate(0.0, -5.5, 0.0), _material(rng), _color(rng))
        d = _logu(rng, 1e3, 1e5)
        v = _unit(rng) * d
        frm, to = tuple(float(x) for x in v), tuple(float(x) for x in rng.uniform(-1, 1, 3))
        fov = float(2.0 * math.atan(9.0 / d))
        P.light(rng.uniform(-30, 30, 3) + [0, 40, 0])
        if rng.random() < 0.5:
            P.light(np.array(frm) * 0.5 + rng.uniform(-3, 3, 3))
    elif cat == "tiny_far":
        d = _logu(rng, 1e3, 1e5)
        s = _logu(rng, 1e-3, 1e-2)
        dirv = _unit(rng)
        target = dirv * d
        for _ in range(int(rng.integers(20, 60))):
            sphere_at(target + rng.uniform(-8, 8, 3) * s, s * rng.uniform(0.3, 2.0), aniso=rng.random() < 0.3)
        for _ in range(int(rng.integers(0, 6))):  # triangles of the same scale next to them
            c = target + rng.uniform(-6, 6, 3) * s
            P.triangle(*(tuple(float(x) for x in c + rng.uniform(-2, 2, 3) * s) for _ in range(3)), _material(rng),
                       _color(rng))
        frm, to = (0.0, 0.0, 0.0), tuple(float(x) for x in target)
        fov = float(2.0 * math.atan(12.0 * s / d))
        P.light(target + _unit(rng) * s * 30)
        P.light(_unit(rng) * d * 2)
    elif cat == "groups":
        P.obj("plane", M.translate(0.0, -3.0, 0.0), _material(rng), _color(rng))

        def fill(parent, level):
            for _ in range(int(rng.integers(2, 5))):
                r = rng.random()
                if level < 3 and r < 0.35:
                    tr = _mul(M, M.scale(*rng.uniform(0.1, 4.0, 3)),
                              M.shear(*[float(x) for x in rng.uniform(-1.5, 1.5, 6) * (rng.random() < 0.6)]),
                              _rot(M, rng), M.translate(*[float(x) for x in rng.uniform(-3, 3, 3)]))
                    g = P.obj("group", tr, parent=parent)
                    fill(g, level + 1)
                elif r < 0.7:
                    sphere_at(rng.uniform(-2, 2, 3), _logu(rng, 0.01, 1.0), parent=parent, aniso=rng.random() < 0.5)
                else:
                    c = rng.uniform(-2, 2, 3)
                    s = _logu(rng, 0.01, 1.5)
                    pts = [tuple(float(x) for x in c + rng.uniform(-1, 1, 3) * s) for _ in range(3)]
                    nrm = None
                    if rng.random() < 0.5:
                        nrm = [tuple(float(x) for x in _unit(rng)) for _ in range(3)]
                    for _ in range(int(rng.integers(1, 4))):
                        P.triangle(*pts, _material(rng), _color(rng), parent=parent, normals=nrm)
                        pts = [pts[1], pts[2], tuple(float(x) for x in c + rng.uniform(-1, 1, 3) * s)]

        for _ in range(int(rng.integers(2, 5))):
            tr = _mul(M, M.scale(*rng.uniform(0.2, 3.0, 3)), M.shear(*[float(x) for x in rng.uniform(-1, 1, 6)]),
                      _rot(M, rng), M.translate(*[float(x) for x in rng.uniform(-6, 6, 3)]))
            fill(P.obj("group", tr), 1)
        P.light(rng.uniform(-20, 20, 3) + [0, 25, -10])
        frm, fov = (float(rng.uniform(-6, 6)), float(rng.uniform(2, 10)), -25.0), float(rng.uniform(0.6, 1.2))
    elif cat == "grazing":
        h = _logu(rng, 1e-3, 0.5)
        for _ in range(int(rng.integers(1, 4))):
            tilt = float(rng.uniform(-5e-3, 5e-3))
            tr = _mul(M, M.rotate("x", tilt), M.rotate("z", float(rng.uniform(-5e-3, 5e-3))),
                      M.translate(0.0, float(rng.uniform(-0.05, 0.05)), 0.0))
            P.obj("plane", tr, _material(rng, reflective_p=0.6), _color(rng))
        for _ in range(int(rng.integers(10, 60))):
            s = _logu(rng, 0.01, 2.0)
            sphere_at((rng.uniform(-30, 30), s * rng.uniform(-0.5, 1.5), rng.uniform(1, 400)), s)
        frm, to = (0.0, h, -5.0), (float(rng.uniform(-1, 1)), h * float(rng.uniform(0.0, 1.0)), 200.0)
        fov = float(rng.uniform(0.2, 1.0))
        P.light((float(rng.uniform(-30, 30)), float(_logu(rng, 0.01, 30.0)), float(rng.uniform(-10, 100))))
    elif cat == "lights":
        P.obj("plane", M.identity(), _material(rng, reflective_p=0.8), _color(rng))
        centers = []
        for _ in range(int(rng.integers(6, 25))):
            s = _logu(rng, 0.1, 2.0)
            c = np.array([rng.uniform(-6, 6), s, rng.uniform(-2, 10)])
            centers.append((c, s))
            sphere_at(c, s, m7=_material(rng, reflective_p=0.8, glass_p=0.3))
        for _ in range(int(rng.integers(1, 3))):  # inside a sphere, or just off its surface
            c, s = centers[int(rng.integers(len(centers)))]
            off = s * (rng.uniform(0.0, 0.8) if rng.random() < 0.4 else 1.0 + _logu(rng, 1e-6, 1e-2))
            P.light(c + _unit(rng) * off)
        if rng.random() < 0.5:
            P.light((float(rng.uniform(-5, 5)), float(_logu(rng, 1e-5, 1e-2)), float(rng.uniform(0, 8))))  # near the floor
        frm, fov = (float(rng.uniform(-4, 4)), float(rng.uniform(1, 6)), -12.0), float(rng.uniform(0.7, 1.3))
    elif cat == "many":
        P.obj("plane", M.translate(0.0, -1.0, 0.0), _material(rng), _color(rng))
        for _ in range(int(rng.integers(600, 900))):
            sphere_at(rng.uniform(-20, 20, 3) * [1, 0.4, 1] + [0, 3, 10], _logu(rng, 5e-3, 1.5))
        P.light(rng.uniform(-20, 20, 3) + [0, 30, -10])
        frm, fov = (float(rng.uniform(-5, 5)), float(rng.uniform(2, 12)), -20.0), float(rng.uniform(0.7, 1.3))
        to = (0.0, 2.0, 10.0)
    elif cat == "general":
        P.obj("plane", M.translate(0.0, -2.0, 0.0), _material(rng), _color(rng))
        for _ in range(int(rng.integers(2, 5))):
            tr = _mul(M, M.scale(*rng.uniform(0.3, 3.0, 3)), M.shear(*[float(x) for x in rng.uniform(-1, 1, 6)]),
                      _rot(M, rng), M.translate(*[float(x) for x in rng.uniform(-5, 5, 3)]))
            g = P.obj("group", tr)
            for _ in range(int(rng.integers(2, 6))):
                s = _logu(rng, 0.02, 1.0)
                t = _mul(M, M.scale(*(s * rng.uniform(0.3, 3.0, 3))), _rot(M, rng),
                         M.translate(*[float(x) for x in rng.uniform(-2, 2, 3)]))
                if rng.random() < 0.5:
                    P.obj("cube", t, _material(rng), _color(rng), parent=g)
                else:
                    lo = float(rng.uniform(-2, 0))
                    P.cylinder(t, _material(rng), _color(rng), lo, lo + float(rng.uniform(0.1, 3)), bool(rng.random() < 0.5),
                               parent=g)
            for _ in range(int(rng.integers(0, 4))):
                sphere_at(rng.uniform(-2, 2, 3), _logu(rng, 0.01, 1.0), parent=g)
        P.light(rng.uniform(-20, 20, 3) + [0, 25, -10])
        frm, fov = (float(rng.uniform(-6, 6)), float(rng.uniform(2, 10)), -25.0), float(rng.uniform(0.6, 1.2))
    up = (0.0, 1.0, 0.0)
    fwd = np.array(to) - np.array(frm)
    if abs(fwd[1]) > 0.99 * np.linalg.norm(fwd):
        up = (1.0, 0.0, 0.0)
    P.log.append(f"camera from={frm} to={to} up={up} fov={fov} depth={depth}")
    return P, {"from_": tuple(float(x) for x in frm), "to": tuple(float(x) for x in to), "up": up, "fov": fov}, depth, cat


def build_area(seed):
    """Area-light scenes for the light-hull pre-test (render_levels.inc area_may_shadow): occluders placed just
    inside and just outside the capsule around the segment from a floor point to the light's centre, tilted and
    light-side planes, skewed / tiny / huge light parallelograms, groups and cubes.  -> (Pair, camera spec, depth,
    category)."""
    rng = np.random.default_rng(20_000 + seed)
    P = Pair()
    M = P.M
    kind = seed % 4
    # the light: a parallelogram above the scene (sometimes skewed, tiny or huge), a few cells per side
    size = [0.3, 1.5, 6.0, 1e-3][int(rng.integers(4))]
    corner = np.array([rng.uniform(-6, 6), rng.uniform(4, 9), rng.uniform(-8, 2)])
    u = np.array([1.0, 0.0, 0.0]) * size
    v = (np.array([0.0, 1.0, 0.0]) if rng.random() < 0.5 else _unit(rng)) * size * rng.uniform(0.3, 1.5)
    if rng.random() < 0.4:
        u = _unit(rng) * size
    level = int(rng.integers(1, 5))
    P.area_light(corner, u, v, level)
    qc = corner + 0.5 * u + 0.5 * v
    qr = 0.5 * max(np.linalg.norm(u + v), np.linalg.norm(u - v))
    # the floor, tilted at times; a second plane near the light's side at times
    tilt = float(rng.uniform(-0.3, 0.3)) if rng.random() < 0.4 else 0.0
    P.obj("plane", _mul(M, M.rotate("z", tilt)), _material(rng, reflective_p=0.5), _color(rng))
    if kind == 1:  # a wall the light's hull straddles or just misses
        P.obj("plane", _mul(M, M.rotate("x", math.pi / 2), M.translate(0.0, 0.0, float(corner[2] + rng.uniform(-0.5, 0.5)))),
              _material(rng), _color(rng))
    parent = -1
    if kind == 2:
        parent = P.obj("group", _mul(M, M.scale(*rng.uniform(0.5, 2.0, 3)), M.translate(*rng.uniform(-1, 1, 3))))
    for _ in range(int(rng.integers(2, 9))):
        # a floor point in view, the segment to the light centre, an occluder at distance ~ r + qr from it
        fp = np.array([rng.uniform(-3, 3), 0.0, rng.uniform(-1, 5)])
        t = rng.uniform(0.1, 0.9)
        a = fp + t * (qc - fp)
        r = _logu(rng, 0.05, 1.0)
        off = (r + qr * t) * (1.0 + float(rng.choice([-1e-3, 1e-6, 1e-3, 0.05, -0.05])))
        c = a + _unit(rng) * off
        if kind == 3 and rng.random() < 0.5:
            tr = _mul(M, M.scale(r, r, r), _rot(M, rng), M.translate(*[float(x) for x in c]))
            P.obj("cube", tr, _material(rng, reflective_p=0.5), _color(rng), parent=parent)
        else:
            P.obj("sphere", _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in c])),
                  _material(rng, reflective_p=0.5), _color(rng), parent)
    if rng.random() < 0.3:
        P.light(qc + rng.uniform(-2, 2, 3))
    frm = (float(rng.uniform(-2, 2)), float(rng.uniform(1.5, 4)), -6.0)
    to = (0.0, 0.5, 2.0)
    fov = float(rng.uniform(0.8, 1.2))
    P.log.append(f"camera from={frm} to={to} fov={fov} depth=3")
    return P, {"from_": frm, "to": to, "up": (0.0, 1.0, 0.0), "fov": fov}, 3, f"area{kind}"


def build_own(seed):
    """Scenes for the own-object skip (shadow and reflected rays skip the object they leave): lights on
    or next to the tangent planes of the spheres the camera sees (light . normal ~ 0), lights inside spheres, the camera
    inside a sphere (inside hits: no skip), anisotropic and sheared spheres, tilted and scaled planes, spheres from 1e-3
    to 1e3 units, far cameras with narrow fields of view (the hit-distance limit of flatten.cpp mark_own_safe), mirrors
    viewed at grazing angles, an area light straddling a sphere's tangent planes.  -> (Pair, camera spec, depth,
    category)."""
    rng = np.random.default_rng(30_000 + seed)
    P = Pair()
    M = P.M
    kind = seed % 6
    cat = ["tangent_light", "light_inside", "camera_inside", "aniso_planes", "far_small", "area_straddle"][kind]
    depth = 4
    frm, to, fov = (0.0, 2.0, -8.0), (0.0, 0.5, 0.0), 1.0
    centres = []
    for _ in range(int(rng.integers(3, 9))):
        r = _logu(rng, 0.2, 1.5)
        c = np.array([rng.uniform(-3, 3), r * rng.uniform(0.5, 1.5), rng.uniform(-2, 3)])
        if kind == 3 and rng.random() < 0.6:
            tr = _mul(M, M.scale(r * rng.uniform(0.2, 3.0), r, r * rng.uniform(0.2, 3.0)), _rot(M, rng),
                      M.shear(*[float(x) for x in rng.uniform(-0.5, 0.5, 6)]), M.translate(*[float(x) for x in c]))
        else:
            tr = _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in c]))
        P.obj("sphere", tr, _material(rng, reflective_p=0.6), _color(rng))
        centres.append((c, r))
    tilt = float(rng.uniform(-0.2, 0.2)) if kind == 3 else 0.0
    sc = float(rng.choice([1.0, 1e-3, 50.0])) if kind == 3 else 1.0
    P.obj("plane", _mul(M, M.scale(sc, sc, sc), M.rotate("z", tilt)), _material(rng, reflective_p=0.6), _color(rng))
    c, r = centres[0]
    if kind == 0:  # lights on the tangent planes of points the camera sees: light . normal ~ 0 at those points
        for _ in range(2):
            n = _unit(rng)
            n[2] = -abs(n[2])  # facing the camera
            n /= np.linalg.norm(n)
            t = np.cross(n, _unit(rng))
            t /= np.linalg.norm(t)
            P.light(c + r * n + t * rng.uniform(2, 10) + n * float(rng.choice([0.0, 1e-9, -1e-9, 1e-6])))
    elif kind == 1:  # a light inside a sphere, another just above a surface
        P.light(c + _unit(rng) * r * 0.5)
        n = _unit(rng)
        P.light(c + n * r * (1.0 + 1e-7))
    elif kind == 2:  # the camera inside a big sphere (glass-free: inside hits shade the inner wall)
        P.obj("sphere", _mul(M, M.scale(30.0, 30.0, 30.0)), _material(rng, reflective_p=0.6), _color(rng))
        P.light(rng.uniform(-5, 5, 3) + [0, 8, 0])
    elif kind == 3:
        P.light(rng.uniform(-10, 10, 3) + [0, 12, -6])
    elif kind == 4:  # spheres from 1e-3 to 1e3 units, seen from 10^2..10^4.5 units away with a narrow field of view
        s = _logu(rng, 1e-3, 1e3)
        for _ in range(4):
            P.obj("sphere", _mul(M, M.scale(s, s, s), M.translate(*[float(x) for x in rng.uniform(-3, 3, 3) * s])),
                  _material(rng, reflective_p=0.6), _color(rng))
        P.light(rng.uniform(-10, 10, 3) * s + [0, 12 * s, 0])
        dist = _logu(rng, 1e2, 3e4) * max(s, 1.0)
        frm = tuple(float(x) for x in _unit(rng) * dist)
        to = (0.0, 0.0, 0.0)
        fov = float(8.0 * s / dist)
    else:  # an area light whose parallelogram straddles the tangent planes of the first sphere's visible points
        n = np.array([0.0, 0.3, -1.0])
        n /= np.linalg.norm(n)
        q = c + r * n
        u = np.cross(n, [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        P.area_light(q + n * float(rng.uniform(-0.5, 0.5)) - u * 2.0 + np.array([0.0, 1.5, 0.0]), u * 4.0,
                     np.array([0.0, 1.0, 0.0]) * float(rng.uniform(0.5, 2.0)), int(rng.integers(2, 5)))
        depth = 3
    if kind in (0, 1, 3) and rng.random() < 0.5:  # grazing view of a mirror: the camera near a sphere's silhouette
        frm = tuple(float(x) for x in c + np.array([r * 1.02, 0.0, -6.0]))
        to = tuple(float(x) for x in c + np.array([r, 0.0, 0.0]))
        fov = 0.3
    if kind == 2:
        frm, to, fov = (0.0, 1.0, -5.0), (0.0, 0.5, 2.0), 1.2
    P.log.append(f"camera from={frm} to={to} fov={fov} depth={depth}")
    return P, {"from_": tuple(float(x) for x in frm), "to": tuple(float(x) for x in to), "up": (0.0, 1.0, 0.0),
               "fov": float(fov)}, depth, cat


GENERAL = ["cones", "tori", "csg", "patterns", "textures", "mixed"]
GENERAL_SEEDS = range(48)


def _pattern_tree(P, rng, level=0):
    """a random pattern tree with its own transforms: stripe / gradient / ring / checker / blend / perturbed / noise over
    solids, nested up to three levels"""
    M = P.M
    if level >= 3 or (level > 0 and rng.random() < 0.4):
        return P.pat("solid", _color(rng))
    kind = str(rng.choice(["stripe", "gradient", "ring", "checker", "blend", "perturbed", "noise"]))
    tr = _mul(M, M.scale(*[_logu(rng, 0.2, 2.0) for _ in range(3)]), _rot(M, rng),
              M.translate(*[float(x) for x in rng.uniform(-1, 1, 3)])) if rng.random() < 0.7 else None
    a = _pattern_tree(P, rng, level + 1)
    if kind == "perturbed":
        return P.pat(kind, a=a, scale=float(rng.uniform(0.05, 0.6)), transform=tr, octaves=int(rng.integers(1, 9)),
                     persistence=float(rng.choice([0.3, 0.5, 1.0, 2.0])))
    b = _pattern_tree(P, rng, level + 1)
    if kind == "noise":
        return P.pat(kind, a=a, b=b, scale=float(rng.uniform(0.5, 3.0)), transform=tr, octaves=int(rng.integers(1, 9)),
                     persistence=float(rng.choice([0.3, 0.5, 1.0, 2.0])))
    return P.pat(kind, a=a, b=b, scale=float(rng.uniform(0.0, 1.0)), transform=tr)


def build_general(seed, light=None, family=None, rng_base=40_000):
    """Scenes for the general kernels (the G = 2 variant: EntriesT<4>, csg_eval, quartic.inc, pattern_tree, texture_at),
    families by seed % 6:

      cones     closed, open and one-sided cones, non-uniformly scaled, half of them in sheared groups
      tori      tori of minor radius 0.05-1.5 at scales 1e-3 to 1e3, seen from 12 to 1e5 scene sizes away
      csg       nested CSG trees (depth <= 3, groups as children, cone / cylinder / torus children, at most
                RR_MAX_CSG_ENTRIES possible entries), glass among the leaves, a glass sphere beside them
      patterns  random pattern trees with their own transforms on every shape kind and on the floor
      textures  numpy textures of 1-6 x 1-6 texels on every shape kind
      mixed     everything inside sheared groups, reflective and glass materials, recursion depth 5

    -> (Pair, camera spec, max_depth, family); Pair.featured holds the builder ids of the family's featured leaves.

    build_area_mix's `general` family passes light(P, rng, s), which adds the scene's lights in place of the one point
    light (s: the scene's scale), the family by name and its own seed base; the seeded scenes of this builder itself
    are untouched by those arguments."""
    rng = np.random.default_rng(rng_base + seed)
    cat = family or GENERAL[seed % len(GENERAL)]
    P = Pair()
    M = P.M
    P.featured = set()
    depth = 5 if cat in ("mixed", "csg") else 3
    s = 1.0  # scene scale
    frm, to, fov = (float(rng.uniform(-6, 6)), float(rng.uniform(2, 8)), -14.0), (0.0, 0.0, 0.0), float(rng.uniform(0.7, 1.0))

    def place(size=(0.4, 1.6), spread=4.0):
        return _mul(M, M.scale(*[s * _logu(rng, *size) for _ in range(3)]), _rot(M, rng),
                    M.translate(*[float(x) for x in rng.uniform(-spread, spread, 3) * [s, 0.5 * s, s]]))

    def sheared_group(parent=-1):
        return P.obj("group", _mul(M, M.scale(*rng.uniform(0.6, 1.6, 3)), M.shear(*[float(x) for x in rng.uniform(-0.6, 0.6, 6)]),
                                   _rot(M, rng), M.translate(*[float(x) for x in rng.uniform(-1.5, 1.5, 3) * s])), parent=parent)

    def leaf(kind, tr, m7, col, parent=-1):
        if kind == "cone":
            lo = float(rng.uniform(-2, 0))
            onesided = rng.random() < 0.2
            i = P.cone(tr, m7, col, -math.inf if onesided else lo, lo + float(rng.uniform(0.2, 2.5)),
                       bool(rng.random() < 0.6) and not onesided, parent)
        elif kind == "cylinder":
            lo = float(rng.uniform(-2, 0))
            i = P.cylinder(tr, m7, col, lo, lo + float(rng.uniform(0.2, 3)), bool(rng.random() < 0.6), parent)
        elif kind == "torus":
            i = P.torus(tr, m7, col, float(rng.choice([0.05, 0.25, 0.5, 0.9, 1.0, 1.5])), parent)
        elif kind == "triangle":
            pts = [tuple(float(x) for x in rng.uniform(-1, 1, 3)) for _ in range(3)]
            nrm = [tuple(float(x) for x in _unit(rng)) for _ in range(3)] if rng.random() < 0.5 else None
            i = P.triangle(*pts, m7, col, parent=parent, normals=nrm, tr=tr)
        else:
            i = P.obj(kind, tr, m7, col, parent)
        return i

    def csg_tree(parent, level, tr, glass_p):
        c = P.csg(str(rng.choice(["union", "intersection", "difference"])), tr, parent)
        for _ in range(2):
            r = rng.random()
            small = _mul(M, M.scale(*rng.uniform(0.6, 1.3, 3)), _rot(M, rng), M.translate(*[float(x) for x in rng.uniform(-0.6, 0.6, 3)]))
            if level < 3 and r < 0.35:
                csg_tree(c, level + 1, small, glass_p)
            elif level < 3 and r < 0.45:
                g = P.obj("group", small, parent=c)
                for _ in range(2):
                    P.featured.add(leaf(str(rng.choice(["sphere", "cube", "cone"])), place((0.5, 1.2), 0.5),
                                        _material(rng, 0.3, glass_p), _color(rng), g))
            else:
                P.featured.add(leaf(str(rng.choice(["sphere", "cube", "cylinder", "cone", "torus"])), small,
                                    _material(rng, 0.3, glass_p), _color(rng), c))
        return c

    if cat == "tori":
        s = _logu(rng, 1e-3, 1e3)
        for _ in range(int(rng.integers(4, 9))):
            P.featured.add(leaf("torus", place((0.8, 2.5), 3.0), _material(rng), _color(rng)))
        dist = s * float(rng.choice([12.0, 1e3, 1e5]))
        frm = tuple(float(x) for x in _unit(rng) * [1, 0.5, 1] * dist + [0, 0.4 * dist, 0])
        fov = float(2.0 * math.atan(7.0 * s / np.linalg.norm(frm)))
    elif cat == "cones":
        for _ in range(int(rng.integers(6, 14))):
            parent = sheared_group() if rng.random() < 0.5 else -1
            P.featured.add(leaf("cone", place(), _material(rng), _color(rng), parent))
    elif cat == "csg":
        for _ in range(int(rng.integers(3, 6))):
            parent = sheared_group() if rng.random() < 0.3 else -1
            csg_tree(parent, 1, place((0.8, 1.8), 3.5), 0.35)
        P.obj("sphere", place((0.8, 1.5), 2.0), (0.1, 0.4, 0.9, SHININESS, 0.1, 0.9, 1.5), _color(rng))
    elif cat == "patterns":
        for k in ("sphere", "cube", "cylinder", "cone", "torus", "triangle", "sphere", "cube")[:int(rng.integers(5, 9))]:
            P.featured.add(leaf(k, place((0.7, 2.0)), _material(rng), _pattern_tree(P, rng)))
    elif cat == "textures":
        for k in ("sphere", "cube", "cylinder", "cone", "torus", "triangle", "sphere", "cube")[:int(rng.integers(5, 9))]:
            img = rng.integers(0, 256, (int(rng.integers(1, 7)), int(rng.integers(1, 7)), 4), dtype=np.uint8)
            pat = P.pat("texture", a=P.tex(img), transform=M.scale(*rng.uniform(0.5, 2, 3)) if rng.random() < 0.5 else None)
            P.featured.add(leaf(k, place((0.7, 2.0)), _material(rng), pat))
    else:  # mixed
        for _ in range(int(rng.integers(2, 5))):
            g = sheared_group()
            for _ in range(int(rng.integers(2, 5))):
                r = rng.random()
                if r < 0.25:
                    csg_tree(g, 2, place((0.6, 1.4), 2.0), 0.3)
                else:
                    k = str(rng.choice(["sphere", "cube", "cylinder", "cone", "torus", "triangle"]))
                    col = _pattern_tree(P, rng) if rng.random() < 0.4 else _color(rng)
                    P.featured.add(leaf(k, place((0.5, 1.5), 2.0), _material(rng, 0.5, 0.3), col, g))
    floor_col = _pattern_tree(P, rng) if cat in ("patterns", "mixed") else _color(rng)
    floor = P.obj("plane", M.translate(0.0, -3.0 * s, 0.0), _material(rng, 0.4 if cat == "mixed" else 0.0), floor_col)
    if cat == "patterns":
        P.featured.add(floor)
    if light is None:
        P.light(rng.uniform(-20, 20, 3) * s + [0, 25 * s, -10 * s])
    else:
        light(P, rng, s)
    up = (0.0, 1.0, 0.0)
    P.log.append(f"camera from={frm} to={to} up={up} fov={fov} depth={depth}")
    return P, {"from_": tuple(float(x) for x in frm), "to": to, "up": up, "fov": fov}, depth, cat


AREA_MIX = ["nodes", "lights", "levels", "general", "patterns", "glass", "degenerate", "umbra"]
AREA_MIX_SEEDS = range(64)
MIX_NODE_COUNTS = (8, 9, 32, 33, 64, 65, 150, 600)  # `nodes`: the flattened node count per seed // 8
MIX_LEVELS = (1, 5, 7, 16, 17, 33, 64, 181)         # `levels`: the area light's level per seed // 8
MIX_LEVELS_SIZE = (16, 12)                           # `levels`: its frames (the oracle casts level^2 rays per event)
MIX_BLACK_LIGHT, MIX_BLACK_SURFACE = 3, 4            # seed // 8 of a family's all-black light / all-black surface
# What the dispatch reads, per family and k = seed // 8, set and not drawn: (G, light kinds in order, complex pattern,
# transparent).  G: 0 flat, 1 groups, 2 general.  "A" an area light, "p" a point light; None: drawn by the family, the
# number given.  Three or more lights switch the prelit stage off (kernels.hpp RR_PRELIT_LIGHTS).
MIX_ATTRS = {
    "nodes": [(0, "A", 0, 0), (0, "AA", 0, 0), (0, "A", 1, 0), (0, "AAp", 0, 0), (0, "A", 0, 0), (0, "AA", 1, 0),
              (0, "A", 0, 0), (0, "AA", 0, 0)],
    "lights": [(0, "AA", 0, 0), (1, "Ap", 1, 0), (2, "pA", 1, 0), (0, "ApA", 1, 0), (1, 4, 1, 0), (2, 5, 1, 0), (0, 3, 0, 0),
               (1, 4, 0, 0)],
    "levels": [(0, "A", 0, 0), (1, "A", 0, 0), (2, "A", 0, 0), (0, "Ap", 0, 0), (1, "A", 0, 0), (2, "pAp", 0, 0),
               (0, "A", 0, 0), (1, "A", 0, 0)],
    "general": [(2, "A" if not k & 1 else "pAA" if k & 2 else "ApA", (k >> 1) & 1, (k >> 2) & 1) for k in range(8)],
    "patterns": [(2, "A", 1, 1), (0, "ApA", 1, 1), (1, "pAA", 1, 1), (2, "AAp", 1, 1), (1, "A", 1, 0), (2, "ApA", 1, 0),
                 (0, "A", 1, 0), (1, "pAA", 1, 0)],
    "glass": [(0, "A", 0, 1), (1, "A", 0, 1), (2, "A", 0, 1), (0, "ApA", 0, 1), (1, "pAA", 0, 1), (2, "AAp", 0, 1),
              (0, "A", 1, 1), (1, "A", 1, 1)],
    "degenerate": [(0, "A", 0, 0), (0, "A", 0, 0), (0, "A", 0, 0), (0, "AAp", 0, 0), (0, "A", 0, 0), (0, "AA", 0, 0),
                   (0, "A", 0, 0), (0, "AA", 0, 0)],
    "umbra": [(0, "A", 0, 0), (0, "A", 0, 0), (0, "A", 0, 0), (0, "AA", 0, 0), (0, "A", 0, 0), (0, "A", 0, 0),
              (0, "Ap", 0, 0), (0, "A", 0, 0)],
}


def mix_attrs(seed):
    """(G, light kinds or their number, complex pattern, transparent) of build_area_mix(seed), from MIX_ATTRS"""
    return MIX_ATTRS[AREA_MIX[seed % 8]][(seed // 8) % 8]


def _n_lights(kinds):
    return kinds if isinstance(kinds, int) else len(kinds)


# the depth-0 frames: the first scene without glass of every (G, PRE, CP); at depth 0 it takes the fused level-0 kernel
MIX_DEPTH0_SEEDS = [next(s for s in AREA_MIX_SEEDS if not mix_attrs(s)[3] and
                         (mix_attrs(s)[0], _n_lights(mix_attrs(s)[1]) <= 2, mix_attrs(s)[2]) == (g, pre, cp))
                    for g in (0, 1, 2) for pre in (True, False) for cp in (0, 1)]


def _light_color(rng):
    """a random light colour, brighter or dimmer than white per channel, one channel exactly zero at times"""
    c = [float(round(x, 3)) for x in rng.uniform(0.2, 1.3, 3)]
    if rng.random() < 0.4:
        c[int(rng.integers(3))] = 0.0
    return tuple(c)


class _Area:
    """one area light's numbers before it is added: corner, u, v, level; its centre qc and half diagonal qr"""

    def __init__(self, corner, u, v, level):
        self.corner, self.u, self.v, self.level = (np.array(corner, float), np.array(u, float), np.array(v, float),
                                                   int(level))
        self.qc = self.corner + 0.5 * self.u + 0.5 * self.v
        self.qr = 0.5 * max(np.linalg.norm(self.u + self.v), np.linalg.norm(self.u - self.v))


def _area_above(rng, level, sizes=(1.5, 3.0, 6.0), S=1.0):
    """a parallelogram above the scene like build_area's, but wide: penumbrae of a few samples' width"""
    size = float(rng.choice(sizes)) * S
    corner = np.array([rng.uniform(-5, 5), rng.uniform(4, 8), rng.uniform(-2, 9)]) * S
    u = (np.array([1.0, 0.0, 0.0]) if rng.random() < 0.6 else _unit(rng)) * size
    v = (np.array([0.0, 0.0, 1.0]) if rng.random() < 0.5 else _unit(rng)) * size * rng.uniform(0.4, 1.2)
    return _Area(corner - 0.5 * u - 0.5 * v, u, v, level)


def _mix_levels(rng, n):
    """n different levels, small ones (the frames stay quick), at least one odd and one a power of two"""
    return [int(x) for x in rng.permutation([2, 3, 4, 5, 6, 8])[:n]]


def _draw_kinds(rng, n):
    """n >= 3 light kinds in a drawn order, at least two of them area lights"""
    kinds = ["A", "A"] + [str(rng.choice(["A", "p"])) for _ in range(n - 2)]
    return "".join(kinds[i] for i in rng.permutation(n))


def _back_point(rng, S=1.0):
    """a point light low behind the scene: the sides of the objects that face the camera lie behind it"""
    return np.array([rng.uniform(-6, 6), rng.uniform(0.3, 2.5), rng.uniform(5, 10)]) * S


def _add_lights(P, rng, kinds, areas, k, S=1.0, points=None):
    """The lights in the order of `kinds`.  The family's all-black light, in its MIX_BLACK_LIGHT scene, is the scene's last
    point light, or its last light where it has none (MIX_ATTRS gives `nodes` and `degenerate` a point light there): a
    black light's lanes are counted and never walked, so it must not be a light whose geometry the scene is about."""
    areas, points = list(areas), list(points or [])
    black = max(kinds.rfind("p"), -1) if "p" in kinds else len(kinds) - 1
    for i, c in enumerate(kinds):
        col = (0.0, 0.0, 0.0) if k == MIX_BLACK_LIGHT and i == black else _light_color(rng)
        if c == "A":
            a = areas.pop(0)
            P.area_light(a.corner, a.u, a.v, a.level, col)
        else:
            P.light(points.pop(0) if points else _back_point(rng, S), col)
        P.log[-1] += f" colour={col}"


def _capsule_point(rng, area, r, S=1.0):
    """build_area's rule: a centre at distance ~ r + qr t from the segment between a visible floor point and the light's
    centre, just inside or just outside the light hull of that point"""
    fp = np.array([rng.uniform(-3, 3), 0.0, rng.uniform(-1, 5)]) * S
    t = rng.uniform(0.1, 0.6)
    a = fp + t * (area.qc - fp)
    off = (r + area.qr * t) * (1.0 + float(rng.choice([-1e-3, 1e-6, 1e-3, 0.05, -0.05, -0.5, -0.9])))
    return a + _unit(rng) * off


def _mix_content(P, rng, areas, G, n, k, cp=False, glass=False, patterned=False, S=1.0, reflective_p=0.4):
    """A floor and n occluders under the lights `areas`: spheres (G = 2: every other a cube) by the capsule rule, turn
    by turn per light; G >= 1: every other one inside a scaled and sheared group, with a plane far behind the scene in a
    group of its own.  cp: the floor carries a gradient (a complex pattern whatever the trees draw); patterned: pattern
    trees and textures on the floor and the occluders; glass: one occluder in three is glass and one is for certain.
    The floor is reflective, so a scene without glass takes the chain kernel at its depth.  The family's all-black surface
    (no diffuse, no specular term under any light) is the first occluder of its MIX_BLACK_SURFACE scene."""
    M = P.M

    def colour():
        if patterned and rng.random() < 0.7:
            if rng.random() < 0.3:
                img = rng.integers(0, 256, (int(rng.integers(1, 5)), int(rng.integers(1, 5)), 4), dtype=np.uint8)
                return P.pat("texture", a=P.tex(img))
            return _pattern_tree(P, rng)
        return _color(rng)

    floor_col = colour()
    if cp:
        floor_col = P.pat("gradient", a=P.pat("solid", _color(rng)), b=floor_col if isinstance(floor_col, Pat) else
                          P.pat("solid", floor_col), transform=M.scale(3.0 * S, 3.0 * S, 3.0 * S))
    fm = _material(rng, 0.0)
    P.obj("plane", M.identity(), fm[:4] + (float(rng.choice([0.2, 0.4])), 0.0, 1.0), floor_col)
    group, ginv = -1, None
    if G >= 1:
        gt = _mul(M, M.scale(*rng.uniform(0.6, 1.6, 3)), M.shear(*[float(x) for x in rng.uniform(-0.4, 0.4, 6)]),
                  M.translate(*[float(x) for x in rng.uniform(-1, 1, 3) * S]))
        group, ginv = P.obj("group", gt), M.inverse(gt)
        back = P.obj("group", M.translate(0.0, 0.0, 14.0 * S))
        P.obj("plane", M.rotate("x", math.pi / 2), _material(rng), _color(rng), parent=back)
    for i in range(n):
        r = _logu(rng, 0.15, 0.9) * S
        c = _capsule_point(rng, areas[i % len(areas)], r, S)
        c[1] = max(c[1], 0.3 * r)
        if i == 0:  # a large one on the visible floor: a core of full shadow, a side turned away from the lights
            r = float(rng.uniform(0.9, 1.5)) * S
            c = np.array([rng.uniform(-2, 2) * S, 0.7 * r, rng.uniform(1, 4) * S])
        m7 = _material(rng, reflective_p)
        col = colour()
        if glass and (i == 1 or rng.random() < 0.33):
            m7 = m7[:4] + (float(rng.choice([0.0, 0.3, 0.9])), float(rng.choice([0.5, 0.9, 1.0])),
                           float(rng.choice([1.33, 1.5, 2.4])))
        if i == 0 and k == MIX_BLACK_SURFACE:
            m7, col = (m7[0], m7[1], 0.0, SHININESS, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
        tr = _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in c]))
        kind = "sphere"
        if G == 2 and i % 2 == 0:
            kind, tr = "cube", _mul(M, M.scale(r, r * rng.uniform(0.3, 1.5), r), _rot(M, rng), M.translate(*[float(x) for x in c]))
        parent = group if G >= 1 and i % 2 == 1 else -1
        P.obj(kind, M.multiply(ginv, tr) if parent >= 0 else tr, m7, col, parent)


def _mix_camera(rng, S=1.0):
    frm = (float(rng.uniform(-2, 2)) * S, float(rng.uniform(1.5, 4)) * S, -6.0 * S)
    return {"from_": frm, "to": (0.0, 0.5 * S, 2.0 * S), "up": (0.0, 1.0, 0.0), "fov": float(rng.uniform(0.8, 1.2))}


def build_area_mix(seed):
    """Area lights across every kernel variant, light mix and level (tests/test_gpu_fuzz.py
    test_area_mix_fuzz_bit_exact): what build_area leaves out.  Eight families by seed % 8; inside a family k = seed // 8
    sets what the dispatch reads from MIX_ATTRS (G, the lights' kinds and order, a complex pattern, transparency), so
    the coverage table of tests/test_area_mix_host.py holds by construction.  Lights take random colours, some with a
    zero channel; every family holds an all-black light (k = 3) and an all-black surface (k = 4).

      nodes       flat scenes of exactly 8, 9, 32, 33, 64, 65, 150 and 600 nodes (a floor, a wall in the odd ones, spheres)
                  under one or two area lights: the per-node regime (RR_BUNDLE_MIN_NODES), the 32-bit node mask, the hull
                  pre-test's limit (RR_AREA_PRETEST_NODES) and, at 600 nodes, culls in global memory.  Capsule-rule
                  occluders are the first and the last spheres added, small clutter between them.  The flattening
                  orders the nodes itself (flatten.cpp: leaves in Morton order, the planes last), so where an occluder
                  lands follows from its position: from 64 nodes on some land at node indices >= 32
                  (tests/test_area_mix_host.py asserts it from node_of_object); in the 33-node scene nodes 31 and 32
                  are the floor and the wall.  The 33-node scene has a third, black point light
      lights      2 to 5 lights: area + area, area + point, point + area, then three and more in a drawn order with at
                  least two area lights of different level (the stage's reuse, li in the jitter key, the LDS layout
                  behind n_lights prelit terms); flat, grouped and general in turn
      levels      level 1, 5, 7, 16, 17, 33, 64 and 181 (frames of MIX_LEVELS_SIZE)
      general     an area light over build_general's content: cones, tori, nested CSG, patterns, everything mixed in
                  sheared groups, planes inside groups (unbounded culls: the pre-test's `pass = true` branch)
      patterns    pattern trees and small textures on the floor and the occluders, under one and three lights
      glass       transparent and reflective materials under one and three lights, flat, grouped and general; depth 4
      degenerate  valid scenes at the edges of the pre-tests' geometry, by k: v the zero vector; u parallel to v; a light
                  that crosses the floor; a light in a plane through visible points with another inside a sphere; a wide light so low
                  that visible points lie within qr of its centre (narrow == false); two lights 3e5 and 3e6 units away
                  (area_beyond_tangent's 1e6 bound); a light below the floor in a scene scaled by 1e-3; a scene scaled
                  by 1e3 with a second light of zero size
      umbra       at most 8 nodes: sheared and rotated ellipsoids large against the light (area_in_umbra), a sphere of
                  radius ~10 (|w| ~ r (1 + 1e-6) on its own surface), a tiny one ~1e3 radii from the floor under it, low
                  lights whose corners straddle the tangent planes of visible points

    -> (Pair, camera spec, max_depth, family)."""
    rng = np.random.default_rng(70_000 + seed)
    cat, k = AREA_MIX[seed % len(AREA_MIX)], (seed // len(AREA_MIX)) % 8
    G, kinds, cp, glass = MIX_ATTRS[cat][k]
    if cat == "general":
        return _mix_general(seed, k, kinds, cp, glass)
    P = Pair()
    M = P.M
    depth, S = 3, 1.0
    spec = _mix_camera(rng)
    if isinstance(kinds, int):
        kinds = _draw_kinds(rng, kinds)
    n_area = kinds.count("A")
    if cat == "nodes":
        areas = [_area_above(rng, lv, (3.0, 6.0)) for lv in _mix_levels(rng, n_area)]
        total = MIX_NODE_COUNTS[k]
        P.obj("plane", M.identity(), (0.1, 0.7, 0.3, SHININESS, 0.3, 0.0, 1.0),
              P.pat("gradient", a=P.pat("solid", _color(rng)), b=P.pat("solid", _color(rng))) if cp else _color(rng))
        if total % 2:  # a wall behind the scene
            P.obj("plane", _mul(M, M.rotate("x", math.pi / 2), M.translate(0.0, 0.0, float(rng.uniform(8, 12)))),
                  _material(rng), _color(rng))
        n = total - 1 - total % 2
        head, tail = min(3, n), min(6, max(n - 3, 0))
        for i in range(n):
            if i < head or i >= n - tail:  # capsule-rule occluders: the first nodes and the last
                r = _logu(rng, 0.2, 0.9)
                c = _capsule_point(rng, areas[i % n_area], r)
                c[1] = max(c[1], 0.3 * r)
                if i == 0:  # a large one on the visible floor
                    r = float(rng.uniform(0.9, 1.5))
                    c = np.array([rng.uniform(-2, 2), 0.7 * r, rng.uniform(1, 4)])
            else:  # clutter that shadows a little
                r = _logu(rng, 0.03, 0.2)
                c = np.array([rng.uniform(-5, 5), rng.uniform(0.0, 3.0), rng.uniform(-2, 8)])
            m7, col = _material(rng, 0.3), _color(rng)
            if i == 0 and k == MIX_BLACK_SURFACE:
                m7, col = (m7[0], m7[1], 0.0, SHININESS, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
            P.obj("sphere", _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in c])), m7, col)
        _add_lights(P, rng, kinds, areas, k)
    elif cat in ("lights", "levels", "patterns", "glass"):
        if cat == "levels":
            levels = [MIX_LEVELS[k]]
        else:
            levels = _mix_levels(rng, n_area)
        areas = [_area_above(rng, lv) for lv in levels]
        if cat == "glass":
            depth = 4
        _mix_content(P, rng, areas, G, int(rng.integers(4, 10)), k, cp=bool(cp), glass=bool(glass),
                     patterned=cat == "patterns")
        _add_lights(P, rng, kinds, areas, k)
    elif cat == "degenerate":
        S = {6: 1e-3, 7: 1e3}.get(k, 1.0)
        spec = _mix_camera(rng, S)
        lv = int(rng.integers(2, 6))
        a = _area_above(rng, lv, S=S)
        if k == 0:
            areas = [_Area(a.corner, a.u, (0.0, 0.0, 0.0), lv)]
        elif k == 1:
            areas = [_Area(a.corner, a.u, a.u * float(rng.choice([0.5, -1.0, 2.0])), lv)]
        elif k == 2:  # crosses the floor: corners on both sides of its plane
            areas = [_Area((float(rng.uniform(-2, 2)), -1.0, float(rng.uniform(1, 4))), (1.5, 0.0, 0.5), (0.0, 3.0, 0.3), lv)]
        elif k == 3:  # in a plane through visible points, the second inside a sphere: both set below, from the first occluder
            areas = [None, None]
        elif k == 4:  # wide and low, over the visible floor: points within qr of its centre
            areas = [_Area((-3.0, float(rng.uniform(0.4, 1.0)), -1.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), lv)]
        elif k == 5:  # on both sides of area_beyond_tangent's light-distance bound
            d1, d2 = _unit(rng), _unit(rng)
            d1[1], d2[1] = abs(d1[1]) + 0.5, abs(d2[1]) + 0.5
            areas = [_Area(d1 * 3e5, (2e4, 0.0, 0.0), (0.0, 0.0, 2e4), lv), _Area(d2 * 3e6, (0.0, 2e5, 0.0), (2e5, 0.0, 0.0), lv + 1)]
        elif k == 6:  # below the floor
            areas = [_Area(np.array([rng.uniform(-2, 2), -3.0, rng.uniform(0, 4)]) * S, (2.0 * S, 0.0, 0.0), (0.0, 0.0, 2.0 * S), lv)]
        else:  # scaled by 1e3; the second light has no size at all
            areas = [a, _Area(a.qc + np.array([3.0, 1.0, -2.0]) * S, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), lv + 1)]
        aim = [x for x in areas if x is not None and x.qc[1] > 0.0 and np.linalg.norm(x.qc) < 1e5 * S] or \
            [_area_above(rng, lv, S=S)]
        n = int(rng.integers(3, 6))
        _mix_content(P, rng, aim, 0, n, k, S=S)
        if k == 3:  # the first occluder (object 1: the floor is object 0) is a large sphere on the floor
            tr = np.array(P.b.transform[16:32]).reshape(4, 4)
            # beside it in the horizontal plane through its centre: the plane holds the sphere's visible equator, floor
            # points see the light from the front (in the floor's own plane every floor sample would have it behind)
            areas[0] = _Area(tr[:3, 3] + np.array([1.2 * tr[0, 0], 0.0, -1.0]), (2.0, 0.0, 0.0), (0.0, 0.0, 2.5), lv)
            areas[1] = _Area(tr[:3, 3] - 0.1 * tr[0, 0], (0.2 * tr[0, 0], 0.0, 0.0), (0.0, 0.2 * tr[0, 0], 0.0), lv + 1)
        _add_lights(P, rng, kinds, areas, k, S)
    else:  # umbra
        low = k % 2 == 1  # a low light at the side: its corners straddle the tangent planes of the ellipsoids' tops
        size = float(rng.choice([0.5, 1.0, 2.0]))
        if low:
            centre = np.array([rng.uniform(-7, 7), rng.uniform(1.0, 2.5), rng.uniform(-2, 6)])
            u, v = np.array([0.0, size, 0.0]), _unit(rng) * size
        else:
            centre = np.array([rng.uniform(-4, 4), rng.uniform(6, 10), rng.uniform(-4, 6)])
            u, v = np.array([size, 0.0, 0.0]), np.array([0.0, 0.0, size * rng.uniform(0.5, 1.0)])
        areas = [_Area(centre - 0.5 * u - 0.5 * v, u, v, lv) for lv in _mix_levels(rng, n_area)]
        if n_area == 2:
            areas[1] = _area_above(rng, areas[1].level, (0.3,))
        P.obj("plane", M.identity(), (0.1, 0.7, 0.3, SHININESS, 0.3, 0.0, 1.0), _color(rng))
        for i in range(int(rng.integers(4, 6))):  # ellipsoids between the visible floor and the light
            fp = np.array([rng.uniform(-3, 3), 0.0, rng.uniform(0, 5)])
            r = float(rng.uniform(0.9, 1.8))
            c = fp + (areas[0].qc - fp) / np.linalg.norm(areas[0].qc - fp) * r * rng.uniform(1.1, 2.0)
            c[1] = max(c[1], 0.8 * r)
            tr = _mul(M, M.scale(r * rng.uniform(0.75, 1.3), r, r * rng.uniform(0.75, 1.3)), _rot(M, rng),
                      M.shear(*[float(x) for x in rng.uniform(-0.25, 0.25, 6) * (i % 2)]), M.translate(*[float(x) for x in c]))
            m7, col = _material(rng, 0.4), _color(rng)
            if i == 0 and k == MIX_BLACK_SURFACE:
                m7, col = (m7[0], m7[1], 0.0, SHININESS, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)
            P.obj("sphere", tr, m7, col)
        r = float(rng.uniform(6.0, 14.0))  # over points on it are r (1 + ~1e-6) from its centre
        P.obj("sphere", _mul(M, M.scale(r, r, r), M.translate(float(rng.uniform(-8, 8)), float(r * rng.uniform(-0.6, 0.2)),
                                                               float(8.0 + r))), _material(rng, 0.4), _color(rng))
        fp = np.array([rng.uniform(-2, 2), 0.0, rng.uniform(0, 4)])  # ~1e3 radii above a visible floor point
        d = (areas[0].qc - fp) / np.linalg.norm(areas[0].qc - fp)
        r = float(rng.uniform(0.002, 0.006))
        P.obj("sphere", _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in fp + d * r * float(rng.uniform(600, 1400))])),
              _material(rng, 0.4), _color(rng))
        _add_lights(P, rng, kinds, areas, k)
    P.log.append(f"camera from={spec['from_']} to={spec['to']} fov={spec['fov']} depth={depth}")
    return P, spec, depth, cat


def _mix_general(seed, k, kinds, cp, glass):
    """build_area_mix's `general` family: build_general's content by (complex pattern, transparent) — cones or tori, CSG
    with its glass sphere, patterns or textures, mixed — then a plane inside a group, a glass sphere or a gradient sphere
    where the content may have drawn none, a mirror sphere, and the lights above the content"""
    family = {(0, 0): "cones" if k < 2 else "tori", (0, 1): "csg", (1, 0): "patterns" if k < 4 else "textures",
              (1, 1): "mixed"}[(cp, glass)]

    def lights(P, rng, s):
        M = P.M
        g = P.obj("group", M.translate(0.0, 0.0, 12.0 * s))
        P.obj("plane", M.rotate("x", math.pi / 2), _material(rng), _color(rng), parent=g)
        extra = [(0.1, 0.5, 0.8, SHININESS, 0.6, 0.0, 1.0)]
        if glass:
            extra.append((0.1, 0.4, 0.9, SHININESS, 0.1, 0.9, 1.5))
        for m7 in extra:
            r = s * float(rng.uniform(0.5, 1.0))
            col = P.pat("gradient", a=P.pat("solid", _color(rng)), b=P.pat("solid", _color(rng))) if cp else _color(rng)
            P.obj("sphere", _mul(M, M.scale(r, r, r), M.translate(*[float(x) for x in rng.uniform(-3, 3, 3) * [s, 0.3 * s, s]])),
                  m7, col)
        areas = []
        for lv in _mix_levels(rng, kinds.count("A")):
            a = _area_above(rng, lv, (6.0, 9.0), S=s)
            areas.append(_Area(a.corner + np.array([0.0, 1.0 * s, 0.0]), a.u, a.v, lv))
        _add_lights(P, rng, kinds, areas, k, s, points=[np.array([rng.uniform(-8, 8), rng.uniform(-2, 3), rng.uniform(4, 10)]) * s
                                                         for _ in range(kinds.count("p"))])
        if k == MIX_BLACK_SURFACE:
            P.obj("sphere", _mul(M, M.scale(1.2 * s, 1.2 * s, 1.2 * s), M.translate(0.0, -1.0 * s, -2.0 * s)),
                  (0.1, 0.7, 0.0, SHININESS, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))

    P, spec, depth, _ = build_general(seed, light=lights, family=family, rng_base=71_000)
    return P, spec, depth, "general"


def mix_key(P, depth):
    """The kernel a frame of this scene takes, from the builder's descriptor alone as traits() reads it, extended by
    complex patterns and the lights: (G, PRE, CP, family at this depth, AR) — render.hip launch_level (G),
    render_levels.inc (PRE: at most PRELIT_LIGHTS lights; CP: flatten.cpp complex_patterns), frame_plan.hpp family_of."""
    import rray_amd as R

    L = R._lib
    t = traits(P)
    g = 2 if t["general"] else 1 if t["groups"] else 0
    cp = any(kd in (L.PAT["gradient"], L.PAT["blend"]) or kd >= L.PAT["perturbed"] for kd in P.b.pat_kind)
    family = "Tree" if t["transparent"] else "Chain" if t["reflective"] and depth > 0 else "Level0"
    return g, int(t["lights"] <= PRELIT_LIGHTS), int(cp), family, int(t["area"])


def light_kinds(P):
    """the scene's lights in order: "A" area, "p" point"""
    import rray_amd as R

    return "".join("A" if kd == R._lib.LIGHT_AREA else "p" for kd in P.b.light_kind)


def cameras(P, spec, W, H):
    """Product and oracle cameras from the same view_transform (the oracle's matrix.rs restatement)."""
    import oracle
    import rray_amd as R

    t = P.M.view_transform(spec["from_"], spec["to"], spec["up"])
    return R.camera(W, H, spec["fov"], t), oracle.Oracle.camera(W, H, spec["fov"], t)


# --- the production dispatch paths (tests/test_gpu_fuzz_paths.py, tests/test_fuzz_paths_host.py) -------------------

BUILDERS = {"build": build, "general": build_general, "area": build_area, "own": build_own}
# build_path's names: the mix is a list of its own (MIX_PATH_SCENES) and stays out of BUILDERS, which the mode x builder
# table of tests/test_gpu_fuzz_paths.py iterates and whose 48 PATH_SCENES stay as they are
PATH_BUILDERS = dict(BUILDERS, mix=build_area_mix)
# the first two seeds of every category of every builder: 8, 6, 4 and 6 categories
PATH_SCENES = ([("build", s) for s in range(16)] + [("general", s) for s in range(12)] +
               [("area", s) for s in range(8)] + [("own", s) for s in range(12)])
PATH_IDS = [f"{b}-{s}" for b, s in PATH_SCENES]
# the area-light mix through the same modes, a list of its own: the first two seeds of every family of build_area_mix
MIX_PATH_SCENES = [("mix", s) for s in range(16)]
MIX_PATH_IDS = [f"{b}-{s}" for b, s in MIX_PATH_SCENES]
PRELIT_LIGHTS = 2  # kernels.hpp RR_PRELIT_LIGHTS: the resident tile loop's kernel holds at most two lights' terms
QUERY_SIZE = (33, 17)  # the query batch's camera: partial tiles on both edges
QUERY_PREFIXES = (1, 63, 65, 257)


def build_path(name, seed):
    """-> (Pair, camera spec, max_depth, category, jitter seed) of one PATH_SCENES entry"""
    P, spec, depth, cat = PATH_BUILDERS[name](seed)
    return P, spec, depth, cat, seed


def traits(P):
    """What the dispatch of api.cpp reads, from the builder's descriptor alone (flatten.cpp: has_transparent,
    max_children, groups, has_csg / has_quad; api.cpp rr_scene_upload: has_groups, general, has_area).  flat: the
    G == 0 kernels; loop: the resident tile loop may serve a depth-0 frame of full tiles under global culls
    (render_persist.inc persist_plan_t, render_persist_g0_gl.hip)."""
    import rray_amd as R

    L = R._lib
    b = P.b
    mats = np.array(b.mats).reshape(-1, 7)
    kinds = set(b.kind)
    t = {"reflective": bool((mats[:, 4] != 0.0).any()), "transparent": bool((mats[:, 5] != 0.0).any()),
         "groups": bool(kinds & {L.GROUP, L.CSG}),
         "general": bool(kinds & {L.CUBE, L.CYLINDER, L.CONE, L.TORUS, L.CSG}),
         "area": L.LIGHT_AREA in b.light_kind, "lights": len(b.light_kind),
         "solid_patterns": all(k == L.PAT["solid"] for k in b.pat_kind)}
    t["flat"] = not t["groups"] and not t["general"] and not t["transparent"]
    t["loop"] = t["flat"] and not t["area"] and t["lights"] <= PRELIT_LIGHTS and t["solid_patterns"]
    return t


def oracle_frame(P, ocam, depth, seed=0, libm=False):
    """The oracle's canvas and counters with correctly rounded powers; libm: also with libm's pow, the
    reference's own arithmetic -> (canvas_cr, st_cr) or (canvas_cr, st_cr, (canvas, st))."""
    if libm:
        ref = P.o.render(ocam, max_depth=depth, seed=seed)
    P.o.set_pow_mode(1)
    try:
        canvas_cr, st_cr = P.o.render(ocam, max_depth=depth, seed=seed)
    finally:
        P.o.set_pow_mode(0)
    return (canvas_cr, st_cr, ref) if libm else (canvas_cr, st_cr)


def oracle_counts(st):
    """the oracle's counters under the product's names (its rays include the shadow rays)"""
    return {"rays": st["rays"] - st["shadow_rays"], "shadow_rays": st["shadow_rays"], "shade_events": st["shade_events"]}


def check_frame(got, P, what, canvas_cr, st_cr, libm=None):
    """The exact-cull comparison of one rendered frame: the canvas equals the oracle's (correctly rounded powers) bit for
    bit and rays / shadow_rays / shade_events equal the oracle's.  libm=(canvas, st) of the libm-pow oracle: its counters
    equal the other oracle's, and the frame may differ from it only in samples where the two oracles differ.  A failure
    prints the differing samples and the scene."""
    diff = np.argwhere((got["canvas"] != canvas_cr).any(axis=2))
    counts = {k: (got["stats"][k], v) for k, v in oracle_counts(st_cr).items()}
    ok = len(diff) == 0 and all(a == b for a, b in counts.values())
    pow_only = []
    if libm is not None:
        canvas, st = libm
        pow_only = np.argwhere((got["canvas"] != canvas).any(axis=2))
        oracles_differ = (canvas != canvas_cr).any(axis=2)
        ok = ok and st == st_cr and all(oracles_differ[y, x] for y, x in pow_only)
    if not ok:
        print(f"{what}: {len(diff)} samples differ from the correctly rounded oracle, {len(pow_only)} from the libm one; "
              f"counts (gpu, oracle) {counts}")
        for y, x in diff[:10]:
            print(f"  sample ({x},{y}): gpu {got['canvas'][y, x].tolist()} oracle {canvas_cr[y, x].tolist()}")
        print("\n".join(P.log))
    elif len(pow_only):
        print(f"{what}: {len(pow_only)} samples differ from libm pow by its rounding only")
    assert ok, what


def first_hits(P, ocam):
    """(vsize, hsize) oracle object id of every sample's first entry with t >= 0 (intersection.rs hit()); -1: a miss"""
    import oracle

    out = np.full((ocam.vsize, ocam.hsize), -1, np.int64)
    for y in range(ocam.vsize):
        for x in range(ocam.hsize):
            ro, rd = oracle.Oracle.ray_for_pixel(ocam, x, y)
            hit = next((e for e in P.o.intersect(ro[:3], rd[:3]) if e[0] >= 0.0), None)
            if hit is not None:
                out[y, x] = hit[1]
    return out


def adaptive_threshold(frame):
    """A threshold for adaptive_mask that lists about half of the frame's pixels: the midpoint between two adjacent
    distinct values of the per-pixel largest neighbour difference, the pair whose listed fraction is nearest 1/2 ->
    (threshold, listed fraction); (None, 0.0) for a frame without two distinct values."""
    import rray_amd as R

    f = np.asarray(frame, np.float64)
    H, W = f.shape[:2]
    d = np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yq, xq = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            d[ys, xs] = np.maximum(d[ys, xs], np.max(np.abs(f[ys, xs] - f[yq, xq]), axis=2))
    vals = np.unique(d[np.isfinite(d)])
    best = (None, 0.0)
    for lo, hi in zip(vals[:-1], vals[1:]):
        thr = float(0.5 * (lo + hi))
        if not lo < thr < hi:
            continue
        frac = float(R.adaptive_mask(f, thr).mean())
        if best[0] is None or abs(frac - 0.5) < abs(best[1] - 0.5):
            best = (thr, frac)
    return best


def query_batch(P, spec, key):
    """The seeded ray batch of the query mode, 1408 or 1472 rays of one scene:

      a  the camera's 33 x 17 rays in a seeded shuffle (incoherent waves, invalid bundles)
      b  the same rays in row-major order, direction lengths cycled through shape_rays.LENGTHS
      c  secondary-like rays: over_point and reflectv of the oracle's hits of the camera rays in row-major order, the
         first 30 or 94 of them (so that a + b + c is whole waves); fewer than 30 hits are filled up from a
      d  four 64-ray fans, each the 8 x 8 tile of b with the most hits and an outlier in its first or its last lane: an
         origin 1e5 scene sizes (|from - to|) away aimed at the scene, or the lane's own ray reversed (make_bundle takes
         its centre and axis from the first and the last live lane)

    A ray whose oracle intersection list holds a NaN t is replaced by the batch's first ray without one (the product
    returns RR_E_NAN where the reference panics).  -> (origins (n, 3), directions (n, 3), number of replaced rays)."""
    import oracle
    import shape_rays as S

    rng = np.random.default_rng(50_000 + key)
    Hs, V = QUERY_SIZE
    _, ocam = cameras(P, spec, Hs, V)
    rays = [oracle.Oracle.ray_for_pixel(ocam, x, y) for y in range(V) for x in range(Hs)]
    o = np.array([r[0][:3] for r in rays])
    d = np.array([r[1][:3] for r in rays])
    n = len(o)
    perm = rng.permutation(n)
    lens = np.array([S.LENGTHS[i % len(S.LENGTHS)] for i in range(n)])
    bo, bd = o.copy(), d * lens[:, None]
    co, cd = [], []
    hit_px = np.zeros(n, bool)
    for i in range(n):
        xs = P.o.intersect(tuple(o[i]), tuple(d[i]))
        if any(math.isnan(x[0]) for x in xs):
            continue
        hit = next((k for k, x in enumerate(xs) if x[0] >= 0.0), None)
        if hit is not None:
            hit_px[i] = True
            c = P.o.prepare_computations(tuple(o[i]), tuple(d[i]), xs, hit)
            co.append(c["over_point"][:3])
            cd.append(c["reflectv"][:3])
    n_c = 94 if len(co) >= 94 else 30
    co, cd = co[:n_c], cd[:n_c]
    for i in range(n_c - len(co)):
        co.append(o[perm[i]].tolist())
        cd.append(d[perm[i]].tolist())
    frm, to = np.array(spec["from_"]), np.array(spec["to"])
    size = float(np.linalg.norm(frm - to))
    fo, fd = [], []
    # the fans' tile: the full tile that holds the most hits (a fan of misses walks nothing; the first such tile in
    # row-major order).  The four outlier variants share it: the same 63 rays, so a difference is the outlier's doing
    hits2d = hit_px.reshape(V, Hs)
    tx, ty = max(((tx, ty) for ty in range(V // 8) for tx in range(Hs // 8)),
                 key=lambda t: int(hits2d[t[1] * 8:t[1] * 8 + 8, t[0] * 8:t[0] * 8 + 8].sum()))
    idx = np.array([(ty * 8 + j) * Hs + tx * 8 + i for j in range(8) for i in range(8)])
    for lane, far in ((0, True), (63, True), (0, False), (63, False)):
        to_, td_ = bo[idx].copy(), bd[idx].copy()
        if far:
            to_[lane] = to + _unit(rng) * 1e5 * size
            aim = to - to_[lane]
            td_[lane] = aim / np.linalg.norm(aim)
        else:
            td_[lane] = -td_[lane]
        fo.append(to_)
        fd.append(td_)
    O = np.concatenate([o[perm], bo, np.array(co).reshape(-1, 3)] + fo)
    D = np.concatenate([d[perm], bd, np.array(cd).reshape(-1, 3)] + fd)
    assert (len(O) - 256) % 64 == 0
    nan = [any(math.isnan(x[0]) for x in P.o.intersect(tuple(a), tuple(b))) for a, b in zip(O, D)]
    good = nan.index(False)
    for i, bad in enumerate(nan):
        if bad:
            O[i], D[i] = O[good], D[good]
    return np.ascontiguousarray(O), np.ascontiguousarray(D), int(sum(nan))


def shadow_pairs(P, spec, key, over_points):
    """(points, lights) for is_shadowed: every given over_point with a light that cycles per lane through the scene's
    light positions (an area light's centre), the camera's position and two seeded points inside the bounds of the
    finite over_points."""
    rng = np.random.default_rng(60_000 + key)
    p = np.asarray(over_points, np.float64).reshape(-1, 3)
    lights = [P.b.light[15 * i:15 * i + 3] for i in range(len(P.b.light_kind))] + [list(spec["from_"])]
    fin = p[np.isfinite(p).all(axis=1)]
    lo, hi = (fin.min(axis=0), fin.max(axis=0)) if len(fin) else (np.zeros(3), np.ones(3))
    lights += [(lo + rng.random(3) * (hi - lo)).tolist() for _ in range(2)]
    return p, np.array([lights[i % len(lights)] for i in range(len(p))], np.float64)
