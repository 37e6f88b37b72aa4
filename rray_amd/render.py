"""Host-side mirror of the reference's render-path interface over the C ABI.

Reference names kept where they exist:
  Scene::add_light / add_object, Sphere::new, Plane::new, Group::add_child  -> SceneBuilder
  Camera::new (camera.rs:41) / Camera::render (camera.rs:107)               -> camera(), Renderer.render
  Scene::color_at (scene.rs:128), Scene::is_shadowed (scene.rs:234)         -> Renderer.color_at / is_shadowed
  render_scene_from_str / render_scene_from_file (scene_builder_yaml.rs:387,429)
Every call goes to librray_amd.so's HIP kernels; there is no CPU path.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib

DEFAULT_MATERIAL = (0.1, 0.9, 0.9, 200.0, 0.0, 0.0, 1.0)  # material.rs:47-58
IDENTITY = tuple(float(i == j) for i in range(4) for j in range(4))


def _dp(a):
    return a.ctypes.data_as(_lib._D)


def _ip(a):
    return a.ctypes.data_as(_lib._I)


class SceneBuilder:
    """Programmatic scene with the reference's registry semantics (object/db.rs, scene.rs:24-71)."""

    def __init__(self):
        self.kind, self.parent, self.material, self.transform, self.tri, self.kids, self.top = [], [], [], [], [], [], []
        self.mats, self.mat_pattern = [], []
        self.pat_kind, self.pat_a, self.pat_b, self.pat_color, self.pat_scale, self.pat_transform = [], [], [], [], [], []
        self.pat_octaves, self.pat_persistence = [], []
        self.textures = []  # (height, width, 4) uint8 RGBA arrays
        self.light_kind, self.light, self.light_level = [], [], []
        self.shape, self.csg_op = [], []
        self._keep = None

    # --- materials / patterns (material.rs, pattern.rs)
    def pattern(self, kind, color=(0.0, 0.0, 0.0), a=-1, b=-1, scale=0.5, transform=IDENTITY, octaves=1,
                persistence=1.0):
        """A pattern tree node (pattern.rs:23-27); octaves / persistence are Perturbed / Noise's."""
        self.pat_kind.append(_lib.PAT[kind] if isinstance(kind, str) else int(kind))
        self.pat_a.append(a)
        self.pat_b.append(b)
        self.pat_color.extend(float(x) for x in color)
        self.pat_scale.append(float(scale))
        self.pat_transform.extend(float(x) for x in transform)
        self.pat_octaves.append(int(octaves))
        self.pat_persistence.append(float(persistence))
        return len(self.pat_kind) - 1

    def texture(self, rgba):
        """Register an RGBA8 image (rows top to bottom, texture.rs:15-19); returns its index for
        pattern("texture", a=index)."""
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("texture must be a non-empty (height, width, 4) uint8 array")
        self.textures.append(a)
        return len(self.textures) - 1

    def new_material(self, mat7=DEFAULT_MATERIAL, pattern=-1):
        self.mats.extend(float(x) for x in mat7)
        self.mat_pattern.append(pattern)
        return len(self.mat_pattern) - 1

    # --- objects
    def _obj(self, kind, parent, transform, material, pattern, tri=None):
        oid = len(self.kind)
        self.kind.append(kind)
        self.parent.append(parent)
        if kind in (_lib.GROUP, _lib.CSG):
            self.material.append(-1)
        else:
            self.material.append(material if isinstance(material, int) else self.new_material(
                material or DEFAULT_MATERIAL, pattern))
        self.transform.extend(float(x) for x in (transform or IDENTITY))
        self.tri.extend([float(x) for x in tri] if tri is not None else [0.0] * 18)
        self.kids.append([])
        self.shape.extend([-math.inf, math.inf, 0.0])
        self.csg_op.append(0)
        (self.kids[parent] if parent >= 0 else self.top).append(oid)
        return oid

    def sphere(self, transform=None, material=None, pattern=-1, parent=-1):
        return self._obj(_lib.SPHERE, parent, transform, material, pattern)

    def plane(self, transform=None, material=None, pattern=-1, parent=-1):
        return self._obj(_lib.PLANE, parent, transform, material, pattern)

    def group(self, transform=None, parent=-1):
        return self._obj(_lib.GROUP, parent, transform, None, -1)

    def cube(self, transform=None, material=None, pattern=-1, parent=-1):
        return self._obj(_lib.CUBE, parent, transform, material, pattern)

    def cylinder(self, minimum=-math.inf, maximum=math.inf, closed=False, transform=None, material=None, pattern=-1,
                 parent=-1, cone=False):
        oid = self._obj(_lib.CONE if cone else _lib.CYLINDER, parent, transform, material, pattern)
        self.shape[3 * oid:3 * oid + 3] = [float(minimum), float(maximum), 1.0 if closed else 0.0]
        return oid

    def cone(self, minimum=-math.inf, maximum=math.inf, closed=False, transform=None, material=None, pattern=-1,
             parent=-1):
        return self.cylinder(minimum, maximum, closed, transform, material, pattern, parent, cone=True)

    def csg(self, op, transform=None, parent=-1):
        """CSG node; add its left then its right child with parent=<this id> (csg.rs:51-65)."""
        oid = self._obj(_lib.CSG, parent, transform, None, -1)
        self.csg_op[oid] = _lib.CSG_OPS[op] if isinstance(op, str) else int(op)
        return oid

    def torus(self, minor_radius, transform=None, material=None, pattern=-1, parent=-1):
        """Torus in the xy plane, major radius 1 (torus.rs:23-31)."""
        oid = self._obj(_lib.TORUS, parent, transform, material, pattern)
        self.shape[3 * oid] = float(minor_radius)
        return oid

    def triangle(self, p1, p2, p3, transform=None, material=None, pattern=-1, parent=-1):
        return self._obj(_lib.TRIANGLE, parent, transform, material, pattern, list(p1) + list(p2) + list(p3) + [0.0] * 9)

    def smooth_triangle(self, p1, p2, p3, n1, n2, n3, transform=None, material=None, pattern=-1, parent=-1):
        return self._obj(_lib.SMOOTH_TRIANGLE, parent, transform, material, pattern,
                         list(p1) + list(p2) + list(p3) + list(n1) + list(n2) + list(n3))

    # --- lights (light.rs:37-45)
    def point_light(self, position, intensity):
        self.light_kind.append(_lib.LIGHT_POINT)
        self.light_level.append(0)
        self.light.extend([float(x) for x in position] + [float(x) for x in intensity] + [0.0] * 9)
        return len(self.light_kind) - 1

    def area_light(self, corner, u, v, intensity, level):
        c, u, v = [float(x) for x in corner], [float(x) for x in u], [float(x) for x in v]
        center = [(c[k] + u[k] * 0.5) + v[k] * 0.5 for k in range(3)]  # Python floats == f64 ops
        self.light_kind.append(_lib.LIGHT_AREA)
        self.light_level.append(int(level))
        self.light.extend(center + [float(x) for x in intensity] + c + u + v)
        return len(self.light_kind) - 1

    def desc(self):
        child_start, child_count, children = [], [], []
        for ks in self.kids:
            child_start.append(len(children))
            child_count.append(len(ks))
            children.extend(ks)
        arr = {
            "kind": np.array(self.kind, np.int32), "parent": np.array(self.parent, np.int32),
            "transform": np.array(self.transform, np.float64), "material": np.array(self.material, np.int32),
            "tri": np.array(self.tri, np.float64), "child_start": np.array(child_start, np.int32),
            "child_count": np.array(child_count, np.int32), "children": np.array(children or [0], np.int32),
            "top": np.array(self.top or [0], np.int32), "mat": np.array(self.mats or [0.0], np.float64),
            "mat_pattern": np.array(self.mat_pattern or [0], np.int32),
            "pat_kind": np.array(self.pat_kind or [0], np.int32), "pat_a": np.array(self.pat_a or [0], np.int32),
            "pat_b": np.array(self.pat_b or [0], np.int32), "pat_color": np.array(self.pat_color or [0.0], np.float64),
            "pat_scale": np.array(self.pat_scale or [0.0], np.float64),
            "pat_transform": np.array(self.pat_transform or [0.0], np.float64),
            "light_kind": np.array(self.light_kind or [0], np.int32),
            "light": np.array(self.light or [0.0], np.float64),
            "light_level": np.array(self.light_level or [0], np.int32),
            "shape": np.array(self.shape or [0.0], np.float64), "csg_op": np.array(self.csg_op or [0], np.int32),
            "pat_octaves": np.array(self.pat_octaves or [0], np.int32),
            "pat_persistence": np.array(self.pat_persistence or [0.0], np.float64),
        }
        tex_size = [v for t in self.textures for v in (t.shape[1], t.shape[0])]
        texels = np.concatenate([t.reshape(-1) for t in self.textures]) if self.textures else np.zeros(4, np.uint8)
        arr["tex_size"] = np.array(tex_size or [0], np.int32)
        arr["texels"] = texels
        d = _lib.SceneDesc()
        d.n_objects = len(self.kind)
        d.n_top = len(self.top)
        d.n_materials = len(self.mat_pattern)
        d.n_patterns = len(self.pat_kind)
        d.n_lights = len(self.light_kind)
        d.n_textures = len(self.textures)
        for k, v in arr.items():
            if v.dtype == np.uint8:
                setattr(d, k, v.ctypes.data_as(C.POINTER(C.c_uint8)))
            else:
                setattr(d, k, _dp(v) if v.dtype == np.float64 else _ip(v))
        d.inverse = None
        self._keep = arr
        return d


class YamlScene:
    """Product front-end: scene_builder_yaml.rs restated in C++ (rr_scene_from_yaml)."""

    def __init__(self, text, width, height, aa=1, obj_root=None):
        h = C.c_void_p()
        cam = _lib.Camera()
        check(lib().rr_scene_from_yaml(text.encode(), obj_root.encode() if obj_root else None, width, height, aa,
                                       C.byref(h), C.byref(cam)))
        self.h, self.camera, self.width, self.height, self.aa = h, cam, width, height, aa

    def desc(self):
        return lib().rr_scene_desc_of(self.h).contents

    def __del__(self):
        try:
            if self.h:
                lib().rr_scene_free(self.h)
                self.h = None
        except Exception:
            pass


def camera(hsize, vsize, field_of_view, transform=None):
    """Camera::new (camera.rs:41-63); sizes are the supersampled W*aa x H*aa."""
    cam = _lib.Camera()
    t = (C.c_double * 16)(*(transform or IDENTITY))
    check(lib().rr_camera_new(hsize, vsize, field_of_view, t, C.byref(cam)))
    return cam


def part_rows(height, part, nparts, block_rows=8):
    n = lib().rr_part_rows(height, part, nparts, block_rows, None)
    if n < 0:
        check(int(n))
    out = np.zeros(max(n, 1), np.int64)
    lib().rr_part_rows(height, part, nparts, block_rows, out.ctypes.data_as(C.POINTER(C.c_int64)))
    return out[:n]


def stage_row_offset(height, part, nparts, block_rows=8):
    """rr_stage_row_offset: first row of part `part`'s tile in the staging buffer (the rows of parts below it)."""
    n = lib().rr_stage_row_offset(height, part, nparts, block_rows)
    if n < 0:
        check(int(n))
    return int(n)


def unshuffle(staged, height, nparts, block_rows=8):
    """rr_unshuffle_host: the root's un-interleave on the host.  staged: (height, W, 3) f64, the parts' tiles back to
    back and unpadded, part p's rows at stage_row_offset(height, p, nparts, block_rows) — the staging buffer the
    library's per-part receives fill on rank 0 (multi.cpp)."""
    g = np.ascontiguousarray(staged, np.float64)
    if nparts < 1 or block_rows < 1 or height < 0:
        raise ValueError(f"unshuffle: bad partition (height {height}, nparts {nparts}, block_rows {block_rows})")
    # the library reads height rows of W * 3 doubles: refuse any other buffer before it does
    if g.ndim != 3 or g.shape[0] != height or g.shape[2] != 3:
        raise ValueError(f"unshuffle: staged must have shape ({height}, W, 3) for height {height}; got {g.shape}")
    W = g.shape[1]
    frame = np.zeros((height, W, 3), np.float64)
    check(lib().rr_unshuffle_host(_dp(g), _dp(frame), W, height, nparts, block_rows))
    return frame


def balance_bands(row_cost, nparts, root_extra=0.0, align=8):
    """rr_balance_bands: band bounds (nparts + 1) over len(row_cost) rows with even cost per band, part 0 carrying
    root_extra on top, inner bounds multiples of align."""
    c = np.ascontiguousarray(row_cost, np.float64)
    out = np.zeros(nparts + 1, np.int64)
    check(lib().rr_balance_bands(_dp(c), len(c), nparts, float(root_extra), align,
                                 out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def device_count():
    n = C.c_int(0)
    lib().rr_device_count(C.byref(n))
    return n.value


def rccl_unique_id():
    """rr_rccl_unique_id: the bytes rank 0 shares with the other ranks before Renderer.rank(...)."""
    buf = (C.c_uint8 * _lib.RCCL_ID_BYTES)()
    check(lib().rr_rccl_unique_id(buf, _lib.RCCL_ID_BYTES))
    return bytes(buf)


class Renderer:
    """A gfx950 render context (rr_ctx): scene in HBM + the wavefront kernels.  Renderer(d) drives one
    device; Renderer.multi(ids) several devices of this process, Renderer.rank(d, n, r, uid) one rank of
    a one-process-per-GPU group — both split each frame in row tiles and gather them with RCCL."""

    def __init__(self, device=0, _handle=None):
        self.h = C.c_void_p()
        if _handle is not None:
            self.h = _handle
        else:
            check(lib().rr_create(device, C.byref(self.h)))
        self.device = device

    @classmethod
    def multi(cls, device_ids):
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        check(lib().rr_create_multi(len(device_ids), ids, C.byref(h)))
        return cls(device_ids[0], _handle=h)

    @classmethod
    def rank(cls, device, nranks, rank, unique_id):
        uid = (C.c_uint8 * _lib.RCCL_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        check(lib().rr_create_rank(device, nranks, rank, uid, C.byref(h)))
        return cls(device, _handle=h)

    @classmethod
    def virtual(cls, device, nparts):
        """rr_create_virtual: nparts virtual ranks on one device (the multi-GPU frame assembly with the
        RCCL transfer replaced by device-local copies)."""
        h = C.c_void_p()
        check(lib().rr_create_virtual(device, nparts, C.byref(h)))
        return cls(device, _handle=h)

    def info(self):
        """(nranks, first global rank of this context, local devices)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().rr_context_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def render_gather_device(self, cam, opts, d_frame, stream=None):
        """Whole frame (row tiles over the group's devices + one RCCL send / receive per part) into d_frame on rank 0's
        device, in `stream` order (asynchronous)."""
        check(lib().rr_render_gather_device(self.h, C.byref(cam), C.byref(opts), C.c_void_p(d_frame) if d_frame else None,
                                            C.c_void_p(stream) if stream else None))

    def bands(self):
        """rr_group_bands: the band bounds of a multi-device context (nranks + 1 rows), or None before its first
        band frame calibrated them."""
        nranks = self.info()[0]
        out = (C.c_int64 * (nranks + 1))()
        n = lib().rr_group_bands(self.h, out, nranks + 1)
        if n < 0:
            check(n)
        return list(out) if n else None

    def set_bands(self, bounds):
        """rr_group_set_bands: impose the band bounds (every rank the same)."""
        b = (C.c_int64 * len(bounds))(*bounds)
        check(lib().rr_group_set_bands(self.h, b, len(bounds)))

    def close(self):
        if getattr(self, "h", None):
            lib().rr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene):
        d = scene.desc()
        check(lib().rr_scene_upload(self.h, C.byref(d)))
        self._scene = scene

    def render(self, cam, aa=1, max_depth=5, seed=0, jitter_mode=0, part=0, nparts=1, block_rows=8, canvas=False,
               avg=True, band=None, interleave=False):
        """Camera::render -> dict(avg=(rows, W, 3) f64 before `as u8`, canvas=(rows*aa, W*aa, 3), stats).
        band=(row_begin, row_end): only those output rows (ABI 10); interleave: a multi-device context splits the
        frame in interleaved tiles (RR_PART_INTERLEAVE) instead of cost-balanced bands."""
        o = _lib.RenderOpts(aa, max_depth, seed, jitter_mode, part, nparts, block_rows,
                            (_lib.RR_OUT_CANVAS if canvas else 0) | (_lib.RR_OUT_AVG if avg else 0) |
                            (_lib.RR_PART_INTERLEAVE if interleave else 0), *(band or (0, 0)))
        H, W = cam.vsize // aa, cam.hsize // aa
        rows = max(band[1] - band[0], 0) if band else len(part_rows(H, part, nparts, block_rows))
        out_avg = np.zeros((rows, W, 3), np.float64) if avg else None
        out_canvas = np.zeros((rows * aa, cam.hsize, 3), np.float64) if canvas else None
        st = _lib.Stats()
        check(lib().rr_render(self.h, C.byref(cam), C.byref(o), _dp(out_canvas) if canvas else None,
                              _dp(out_avg) if avg else None, C.byref(st)))
        return {"avg": out_avg, "canvas": out_canvas, "stats": st.as_dict()}

    def render_device(self, cam, opts, d_canvas, d_avg, stream=None):
        """Renders into device buffers (ints: device pointers), ordered on `stream` (int or None)."""
        check(lib().rr_render_device(self.h, C.byref(cam), C.byref(opts), C.c_void_p(d_canvas or 0) if d_canvas else None,
                                     C.c_void_p(d_avg) if d_avg else None, C.c_void_p(stream) if stream else None))

    def kernel_profile(self, enable=True):
        check(lib().rr_kernel_profile(self.h, 1 if enable else 0))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} accumulated since kernel_profile(True)."""
        ms = (C.c_double * 16)()
        n = (C.c_uint64 * 16)()
        k = lib().rr_kernel_times(self.h, ms, n, 16)
        if k < 0:
            check(k)
        return {_lib.KERNELS[i]: (ms[i], int(n[i])) for i in range(k)}

    def resident_launch(self):
        """(blocks, heads) of the last frame's resident tile-loop launch; (0, 0): it ran the per-tile launch."""
        blocks, heads = C.c_int32(0), C.c_int32(0)
        check(lib().rr_resident_launch(self.h, C.byref(blocks), C.byref(heads)))
        return blocks.value, heads.value

    def last_stats(self):
        st = _lib.Stats()
        check(lib().rr_last_stats(self.h, C.byref(st)))
        return st.as_dict()

    def color_at(self, origins, directions, remaining=5, seed=0, jitter_mode=0):
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
        out = np.zeros_like(o)
        check(lib().rr_color_at(self.h, len(o), _dp(o), _dp(d), remaining, seed, jitter_mode, _dp(out)))
        return out

    def hit_at(self, origins, directions):
        """Scene::intersect -> hit -> prepare_computations per ray (rr_hit_at): a structured array (_lib.hit_dtype():
        object, inside, t, u, v, point, eyev, normalv, over_point, under_point, reflectv, n1, n2); a miss has
        object -1 and zeros."""
        o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
        out = np.zeros(len(o), _lib.hit_dtype())
        check(lib().rr_hit_at(self.h, len(o), _dp(o), _dp(d), out.ctypes.data_as(C.POINTER(_lib.Hit))))
        return out

    @staticmethod
    def _aov_mask(planes):
        unknown = [p for p in planes if p not in _lib.AOV_PLANES]
        if unknown:
            raise ValueError(f"unknown AOV planes {unknown}: choose from {sorted(_lib.AOV_PLANES)}")
        mask = 0
        for p in planes:
            mask |= _lib.AOV_PLANES[p]
        return mask

    def render_aov(self, cam, aa=1, planes=("depth", "normal", "object", "albedo"), part=0, nparts=1, band=None):
        """The camera rays' first hits as planes per canvas sample (rr_render_aov): dict of depth (vsize, hsize) f64
        (+inf: miss), normal (vsize, hsize, 3), object (vsize, hsize) int32 (-1: miss), albedo (vsize, hsize, 3), and
        stats.  Never averaged: aa only has to divide the camera sizes.  Whole frames only (part / nparts / band are
        passed through so that the library refuses them)."""
        mask = self._aov_mask(planes)
        o = _lib.RenderOpts(aa, 0, 0, 0, part, nparts, 8, 0, *(band or (0, 0)))
        V, Hs = cam.vsize, cam.hsize
        out = {"depth": np.zeros((V, Hs), np.float64) if "depth" in planes else None,
               "normal": np.zeros((V, Hs, 3), np.float64) if "normal" in planes else None,
               "object": np.zeros((V, Hs), np.int32) if "object" in planes else None,
               "albedo": np.zeros((V, Hs, 3), np.float64) if "albedo" in planes else None}
        st = _lib.Stats()
        check(lib().rr_render_aov(self.h, C.byref(cam), C.byref(o), mask,
                                  _dp(out["depth"]) if out["depth"] is not None else None,
                                  _dp(out["normal"]) if out["normal"] is not None else None,
                                  _ip(out["object"]) if out["object"] is not None else None,
                                  _dp(out["albedo"]) if out["albedo"] is not None else None, C.byref(st)))
        res = {k: v for k, v in out.items() if v is not None}
        res["stats"] = st.as_dict()
        return res

    def render_aov_device(self, cam, opts, planes, d_depth=None, d_normal=None, d_object=None, d_albedo=None,
                          stream=None):
        """rr_render_aov_device: the planes into device buffers (ints: device pointers), ordered on `stream` (int or
        None), not synchronised.  planes: names or an RR_AOV_* mask."""
        mask = planes if isinstance(planes, int) else self._aov_mask(planes)
        p = [C.c_void_p(x) if x else None for x in (d_depth, d_normal, d_object, d_albedo)]
        check(lib().rr_render_aov_device(self.h, C.byref(cam), C.byref(opts), mask, *p,
                                         C.c_void_p(stream) if stream else None))

    def render_adaptive(self, cam, aa, threshold, max_depth=5, seed=0, jitter_mode=0):
        """rr_render_adaptive: the aa 1 frame of the view with the pixels adaptive_mask(that frame, threshold) marks
        replaced by the pixels render(cam, aa) gives, bit for bit.  cam is the full camera (W*aa x H*aa; its
        field_of_view and transform define the aa 1 probe camera).  -> dict(avg=(H, W, 3) f64, mask=(H, W) uint8,
        n_refined, stats); stats['samples'] == W*H + aa*aa*n_refined."""
        o = _lib.RenderOpts(aa, max_depth, seed, jitter_mode, 0, 1, 8, 0, 0, 0)
        H, W = cam.vsize // max(aa, 1), cam.hsize // max(aa, 1)
        avg = np.zeros((H, W, 3), np.float64)
        mask = np.zeros((H, W), np.uint8)
        n = C.c_int64(0)
        st = _lib.Stats()
        check(lib().rr_render_adaptive(self.h, C.byref(cam), C.byref(o), float(threshold), _dp(avg),
                                       mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n), C.byref(st)))
        return {"avg": avg, "mask": mask, "n_refined": int(n.value), "stats": st.as_dict()}

    def render_adaptive_device(self, cam, opts, threshold, d_avg, d_mask=None, d_n_refined=None, stream=None):
        """rr_render_adaptive_device: the same into device buffers (ints: device pointers; d_avg H*W*3 f64, d_mask H*W
        bytes, d_n_refined one int64), ordered on `stream` (int or None), not synchronised."""
        p = [C.c_void_p(x) if x else None for x in (d_avg, d_mask, d_n_refined, stream)]
        check(lib().rr_render_adaptive_device(self.h, C.byref(cam), C.byref(opts), float(threshold), *p))

    @staticmethod
    def _camera_array(cams):
        cams = list(cams)
        return (_lib.Camera * max(len(cams), 1))(*cams), len(cams)

    def render_views(self, cams, aa=1, max_depth=5, seed=0, jitter_mode=0, canvas=False):
        """rr_render_views: a batch of cameras of one size in one call -> dict(avg=(N, H, W, 3) f64,
        canvas=(N, vsize, hsize, 3) f64 or None, stats).  View k is render(cams[k], ...) bit for bit."""
        arr, n = self._camera_array(cams)
        o = _lib.RenderOpts(aa, max_depth, seed, jitter_mode, 0, 1, 8,
                            _lib.RR_OUT_AVG | (_lib.RR_OUT_CANVAS if canvas else 0), 0, 0)
        hs, vs = (arr[0].hsize, arr[0].vsize) if n else (0, 0)
        out_avg = np.zeros((n, vs // max(aa, 1), hs // max(aa, 1), 3), np.float64)
        out_canvas = np.zeros((n, vs, hs, 3), np.float64) if canvas else None
        st = _lib.Stats()
        check(lib().rr_render_views(self.h, arr, n, C.byref(o), _dp(out_canvas) if canvas else None, _dp(out_avg),
                                    C.byref(st)))
        return {"avg": out_avg, "canvas": out_canvas, "stats": st.as_dict()}

    def render_views_device(self, cams, opts, d_canvas, d_avg, stream=None):
        """rr_render_views_device: the batch into device buffers (ints: device pointers; d_avg N*H*W*3 f64 with
        RR_OUT_AVG in opts.flags, d_canvas N*vsize*hsize*3 f64 with RR_OUT_CANVAS), ordered on `stream` (int or None),
        not synchronised."""
        arr, n = self._camera_array(cams)
        p = [C.c_void_p(x) if x else None for x in (d_canvas, d_avg, stream)]
        check(lib().rr_render_views_device(self.h, arr, n, C.byref(opts), *p))

    def render_views_aov(self, cams, aa=1, planes=("depth", "normal", "object", "albedo")):
        """rr_render_views_aov: the first-hit planes of a batch of cameras of one size in one call -> dict of depth
        (N, vsize, hsize) f64 (+inf: miss), normal (N, vsize, hsize, 3), object (N, vsize, hsize) int32 (-1: miss),
        albedo (N, vsize, hsize, 3), and stats.  Slice k of each plane is render_aov(cams[k], aa, planes)'s, bit for
        bit; never averaged: aa only has to divide the camera sizes."""
        mask = self._aov_mask(planes)
        arr, n = self._camera_array(cams)
        o = _lib.RenderOpts(aa, 0, 0, 0, 0, 1, 8, 0, 0, 0)
        hs, vs = (arr[0].hsize, arr[0].vsize) if n else (0, 0)
        out = {"depth": np.zeros((n, vs, hs), np.float64) if "depth" in planes else None,
               "normal": np.zeros((n, vs, hs, 3), np.float64) if "normal" in planes else None,
               "object": np.zeros((n, vs, hs), np.int32) if "object" in planes else None,
               "albedo": np.zeros((n, vs, hs, 3), np.float64) if "albedo" in planes else None}
        st = _lib.Stats()
        check(lib().rr_render_views_aov(self.h, arr, n, C.byref(o), mask,
                                        _dp(out["depth"]) if out["depth"] is not None else None,
                                        _dp(out["normal"]) if out["normal"] is not None else None,
                                        _ip(out["object"]) if out["object"] is not None else None,
                                        _dp(out["albedo"]) if out["albedo"] is not None else None, C.byref(st)))
        res = {k: v for k, v in out.items() if v is not None}
        res["stats"] = st.as_dict()
        return res

    def render_views_aov_device(self, cams, opts, planes, d_depth=None, d_normal=None, d_object=None, d_albedo=None,
                                stream=None):
        """rr_render_views_aov_device: the stacked planes into device buffers (ints: device pointers; depth N*vsize*hsize
        f64, normal and albedo N*vsize*hsize*3 f64, object N*vsize*hsize int32), ordered on `stream` (int or None), not
        synchronised.  planes: names or an RR_AOV_* mask."""
        mask = planes if isinstance(planes, int) else self._aov_mask(planes)
        arr, n = self._camera_array(cams)
        p = [C.c_void_p(x) if x else None for x in (d_depth, d_normal, d_object, d_albedo, stream)]
        check(lib().rr_render_views_aov_device(self.h, arr, n, C.byref(opts), mask, *p))

    def is_shadowed(self, points, light_positions):
        p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        lp = np.ascontiguousarray(light_positions, np.float64).reshape(-1, 3)
        out = np.zeros(len(p), np.int32)
        check(lib().rr_is_shadowed(self.h, len(p), _dp(p), _dp(lp), _ip(out)))
        return out.astype(bool)

    # ---- device-resident ray queries (rray.h RR_HAS_RAYS_DEVICE): device pointers as ints, nothing synchronised ----
    def camera_rays_device(self, cam, d_rays, stream=None):
        """rr_camera_rays_device: the hsize * vsize rays of `cam` into d_rays (int: a device pointer to hsize * vsize * 6
        f64), row-major, ray py * hsize + px = origin xyz, direction xyz — the colour frame's rays bit for bit.  Ordered
        on `stream` (int or None), not synchronised; no scene needed.  With torch:
            rays = torch.empty((cam.vsize * cam.hsize, 6), dtype=torch.float64, device=dev)
            r.camera_rays_device(cam, rays.data_ptr(), torch.cuda.current_stream().cuda_stream)"""
        p = [C.c_void_p(x) if x else None for x in (d_rays, stream)]
        check(lib().rr_camera_rays_device(self.h, C.byref(cam), *p))

    def color_at_device(self, n, d_rays, d_rgb, remaining=5, seed=0, jitter_mode=0, stream=None):
        """rr_color_at_device: Scene::color_at of n rays read in place from d_rays (n x 6 f64: origin, direction;
        torch.cat([origins, directions], 1) for a caller who holds the two apart) into d_rgb (n x 3 f64), what
        color_at returns for the same rays bit for bit.  Ray i's area-light jitter identity is sample i, so the rays
        of camera_rays_device(cam) give render(cam, canvas=True)'s canvas.  NaN rays are counted in
        last_stats()['nan_rays'], never raised."""
        p = [C.c_void_p(x) if x else None for x in (d_rays,)]
        q = [C.c_void_p(x) if x else None for x in (d_rgb, stream)]
        check(lib().rr_color_at_device(self.h, n, *p, remaining, seed, jitter_mode, *q))

    def hit_at_device(self, n, d_rays, d_hits, stream=None):
        """rr_hit_at_device: n rr_hit records (192 bytes each, _lib.hit_dtype()'s layout) into d_hits, record i what
        hit_at returns for ray i bit for bit.  With torch:
            hits = torch.empty((n, 192), dtype=torch.uint8, device=dev)
            r.hit_at_device(n, rays.data_ptr(), hits.data_ptr(), stream)
            hits.view(torch.float64)      # (n, 24): column 1 t, 4:7 point, 10:13 normalv, 22:24 n1, n2
            hits.view(torch.int32)[:, :2]  # object, inside (a miss: object -1, everything else 0)"""
        p = [C.c_void_p(x) if x else None for x in (d_rays, d_hits, stream)]
        check(lib().rr_hit_at_device(self.h, n, *p))

    def is_shadowed_device(self, n, d_points, d_light_positions, d_out, stream=None):
        """rr_is_shadowed_device: Scene::is_shadowed of n (point, light position) pairs — two n x 3 f64 device arrays —
        into d_out (n int32: 0 / 1), is_shadowed's values.  last_stats() is left as it is."""
        p = [C.c_void_p(x) if x else None for x in (d_points, d_light_positions, d_out, stream)]
        check(lib().rr_is_shadowed_device(self.h, n, *p))


    # ---- ordered ray batches (rray.h RR_HAS_RAY_ORDER) ----
    def ray_order_device(self, n, d_rays, d_perm, stream=None):
        """rr_ray_order_device: the coherent order of the n rays at d_rays into d_perm (int: a device pointer to n
        uint32): d_perm[j] is the ray at position j, argsort(ray_order_keys(rays), kind="stable").  No scene needed.
        With torch: perm = torch.empty(n, dtype=torch.int32, device=dev) (the bits are unsigned)."""
        p = [C.c_void_p(x) if x else None for x in (d_rays, d_perm, stream)]
        check(lib().rr_ray_order_device(self.h, n, *p))

    def color_at_device_ordered(self, n, d_rays, d_rgb, d_perm=None, remaining=5, seed=0, jitter_mode=0, stream=None):
        """rr_color_at_device_ordered: color_at_device's d_rgb bit for bit, with the waves walking the batch in the
        order d_perm (None: the library orders the batch itself first, on the same stream).  A d_perm of the caller's
        must be a permutation of 0..n-1; it is not checked."""
        p = [C.c_void_p(x) if x else None for x in (d_rays, d_perm)]
        q = [C.c_void_p(x) if x else None for x in (d_rgb, stream)]
        check(lib().rr_color_at_device_ordered(self.h, n, *p, remaining, seed, jitter_mode, *q))

    def hit_at_device_ordered(self, n, d_rays, d_hits, d_perm=None, stream=None):
        """rr_hit_at_device_ordered: hit_at_device's records bit for bit (record i is ray i's), walked in the order
        d_perm (None: the library's own)."""
        p = [C.c_void_p(x) if x else None for x in (d_rays, d_perm, d_hits, stream)]
        check(lib().rr_hit_at_device_ordered(self.h, n, *p))

    # ---- lens frames (rray.h RR_HAS_LENS): depth of field and jittered samples per pixel ----
    def lens_rays_device(self, cam, lens, d_rays, first_pixel=0, n_pixels=None, stream=None):
        """rr_lens_rays_device: the rays of pixels [first_pixel, first_pixel + n_pixels) of `cam` under `lens` into
        d_rays (int: a device pointer to n_pixels * lens.samples * 6 f64), lens_rays(cam, lens, ...) bit for bit.
        Ordered on `stream` (int or None), not synchronised; no scene needed."""
        n = cam.hsize * cam.vsize - first_pixel if n_pixels is None else n_pixels
        d = lens.desc()
        p = [C.c_void_p(x) if x else None for x in (d_rays, stream)]
        check(lib().rr_lens_rays_device(self.h, C.byref(cam), C.byref(d), first_pixel, n, *p))

    def render_lens(self, cam, lens, max_depth=5, seed=0, jitter_mode=0):
        """rr_render_lens: a frame of lens.samples rays per pixel of `cam` (at output size, aa 1) ->
        dict(avg=(H, W, 3) f64, stats): lens_resolve of color_at_device over lens_rays_device(cam, lens), bit for bit;
        sample s of pixel p has the area-light jitter identity of sample p * S + s.  stats['samples'] == W * H * S."""
        o = _lib.RenderOpts(1, max_depth, seed, jitter_mode, 0, 1, 8, 0, 0, 0)
        d = lens.desc()
        avg = np.zeros((cam.vsize, cam.hsize, 3), np.float64)
        st = _lib.Stats()
        check(lib().rr_render_lens(self.h, C.byref(cam), C.byref(o), C.byref(d), _dp(avg), C.byref(st)))
        return {"avg": avg, "stats": st.as_dict()}

    def render_lens_device(self, cam, opts, lens, d_avg, stream=None):
        """rr_render_lens_device: the frame into d_avg (int: a device pointer to H * W * 3 f64), ordered on `stream`
        (int or None), not synchronised; NaN rays are counted in last_stats()['nan_rays'], never raised."""
        d = lens.desc()
        p = [C.c_void_p(x) if x else None for x in (d_avg, stream)]
        check(lib().rr_render_lens_device(self.h, C.byref(cam), C.byref(opts), C.byref(d), *p))

    # ---- ambient occlusion (rray.h RR_HAS_AO): how open the surface is at a point ----
    def ao_at_device(self, n, d_points, d_normals, ao, d_ao, stream=None):
        """rr_ao_at_device: the occlusion value of n points — two n x 3 f64 device arrays, positions and unit normals
        (ints: device pointers) — into d_ao (n f64): ao_resolve of is_shadowed_device over ao_targets(points, normals,
        ao), bit for bit.  Ordered on `stream` (int or None), not synchronised; last_stats() is left as it is."""
        d = ao.desc()
        p = [C.c_void_p(x) if x else None for x in (d_points, d_normals)]
        q = [C.c_void_p(x) if x else None for x in (d_ao, stream)]
        check(lib().rr_ao_at_device(self.h, n, *p, C.byref(d), *q))

    def render_ao(self, cam, ao, aa=1):
        """rr_render_ao: the occlusion plane of `cam` -> dict(ao=(vsize, hsize) f64, stats): one value per canvas sample,
        never averaged; ao_at_device at over_point / normalv of hit_at_device over camera_rays_device(cam), bit for bit,
        1.0 where the sample misses.  stats['shadow_rays'] == ao.samples * hits."""
        o = _lib.RenderOpts(aa, 0, 0, 0, 0, 1, 8, 0, 0, 0)
        d = ao.desc()
        out = np.zeros((cam.vsize, cam.hsize), np.float64)
        st = _lib.Stats()
        check(lib().rr_render_ao(self.h, C.byref(cam), C.byref(o), C.byref(d), _dp(out), C.byref(st)))
        return {"ao": out, "stats": st.as_dict()}

    def render_ao_device(self, cam, opts, ao, d_ao, stream=None):
        """rr_render_ao_device: the plane into d_ao (int: a device pointer to vsize * hsize f64), ordered on `stream`
        (int or None), not synchronised."""
        d = ao.desc()
        p = [C.c_void_p(x) if x else None for x in (d_ao, stream)]
        check(lib().rr_render_ao_device(self.h, C.byref(cam), C.byref(opts), C.byref(d), *p))

    # ---- the edge-avoiding denoiser (rray.h RR_HAS_DENOISE) ----
    # ---- one-bounce indirect light (rray.h RR_HAS_INDIRECT): what the surroundings send to a point ----
    def indirect_at_device(self, n, d_points, d_normals, ind, d_out, seed=0, jitter_mode=0, stream=None):
        """rr_indirect_at_device: the gathered radiance of n points — two n x 3 f64 device arrays, positions and unit
        normals (ints: device pointers) — into d_out (n x 3 f64): indirect_resolve of color_at_device (remaining =
        ind.remaining, this seed and jitter_mode) over indirect_rays(points, normals, ind).  Ordered on `stream` (int or
        None), not synchronised; last_stats() afterwards is the colour trace's, with samples == n."""
        d = ind.desc()
        p = [C.c_void_p(x) if x else None for x in (d_points, d_normals)]
        q = [C.c_void_p(x) if x else None for x in (d_out, stream)]
        check(lib().rr_indirect_at_device(self.h, n, *p, C.byref(d), seed & 0xFFFFFFFFFFFFFFFF, jitter_mode, *q))

    def render_indirect(self, cam, ind, aa=1, seed=0, jitter_mode=0):
        """rr_render_indirect: the gathered radiance of `cam`'s canvas samples -> dict(indirect=(vsize, hsize, 3) f64,
        stats): one value per canvas sample, never averaged and not multiplied by the surface's albedo (indirect_compose
        does that); indirect_at_device at over_point / normalv of hit_at_device over camera_rays_device(cam), (0, 0, 0)
        where the sample misses — a miss traces nothing: stats['rays'] == the camera's rays + the rays of a color_at_device
        over the hits' gathered rays only."""
        o = _lib.RenderOpts(aa, 0, seed & 0xFFFFFFFFFFFFFFFF, jitter_mode, 0, 1, 8, 0, 0, 0)
        d = ind.desc()
        out = np.zeros((cam.vsize, cam.hsize, 3), np.float64)
        st = _lib.Stats()
        check(lib().rr_render_indirect(self.h, C.byref(cam), C.byref(o), C.byref(d), _dp(out), C.byref(st)))
        return {"indirect": out, "stats": st.as_dict()}

    def render_indirect_device(self, cam, opts, ind, d_out, stream=None):
        """rr_render_indirect_device: the plane into d_out (int: a device pointer to vsize * hsize * 3 f64), ordered on
        `stream` (int or None), not synchronised; NaN rays are counted in last_stats()['nan_rays'], never raised."""
        d = ind.desc()
        p = [C.c_void_p(x) if x else None for x in (d_out, stream)]
        check(lib().rr_render_indirect_device(self.h, C.byref(cam), C.byref(opts), C.byref(d), *p))

    def denoise(self, img, dn, depth=None, normal=None, object=None, albedo=None):
        """rr_denoise: `img` (H, W) or (H, W, 1) or (H, W, 3) f64 filtered on the device with the guide planes that are
        given (render_aov's layouts) -> an array of img's shape; denoise_filter of the same arguments, bit for bit."""
        a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
        out = np.zeros_like(a)
        d = dn.desc()
        check(lib().rr_denoise(self.h, C.byref(d), W, H, Cn, _dp(a), *_denoise_ptrs(planes), _dp(out)))
        return out.reshape(np.shape(img))

    def denoise_device(self, dn, width, height, channels, d_in, d_out, d_depth=None, d_normal=None, d_object=None,
                       d_albedo=None, stream=None):
        """rr_denoise_device: device buffers (ints: device pointers; d_in and d_out height * width * channels f64),
        ordered on `stream` (int or None), not synchronised; last_stats() is left as it is."""
        d = dn.desc()
        p = [C.c_void_p(x) if x else None for x in (d_in, d_depth, d_normal, d_object, d_albedo, d_out, stream)]
        check(lib().rr_denoise_device(self.h, C.byref(d), width, height, channels, *p))

    # ---- temporal accumulation (rray.h RR_HAS_TEMPORAL) ----
    def temporal(self, img, tp, cam, prev_cam, depth, normal=None, object=None, prev=None, moments=False):
        """rr_temporal: `img` (H, W), (H, W, 1) or (H, W, 3) f64 blended on the device with the history `prev` (what the
        previous call returned; None: no history) seen from `prev_cam` -> dict(out, n, m2, depth, normal, object): the
        accumulated image (img's shape), the int32 history lengths, the second moments (None unless `moments`) and this
        frame's planes — a valid `prev` for the next call.  temporal_filter of the same arguments, bit for bit."""
        return _temporal_call(lambda *a: lib().rr_temporal(self.h, *a), img, tp, cam, prev_cam, depth, normal, object, prev,
                              moments)

    def temporal_device(self, tp, width, height, channels, cam, prev_cam, cur, prev, d_out, d_n, d_m2=None, stream=None):
        """rr_temporal_device: device buffers (ints: device pointers).  `cur` and `prev` are dicts of rr_temporal_frame's
        fields (image, depth, normal, object, count, m2; a missing key or None: no plane); d_out height * width *
        channels f64, d_n height * width int32, d_m2 like d_out or None.  Ordered on `stream` (int or None), not
        synchronised; last_stats() is left as it is."""
        d = tp.desc()
        fc, fp = (_lib.TemporalFrame(*[f.get(k) or None for k in ("image", "depth", "normal", "object", "count", "m2")])
                  for f in (cur, prev))
        p = [C.c_void_p(x) if x else None for x in (d_out, d_n, d_m2, stream)]
        check(lib().rr_temporal_device(self.h, C.byref(d), width, height, channels, C.byref(cam), C.byref(fc),
                                       C.byref(prev_cam), C.byref(fp), *p))

    # ---- variance-guided denoising (rray.h RR_HAS_DENOISE_VAR) ----
    def variance(self, img, vr, m2=None, count=None, depth=None, normal=None, object=None, albedo=None):
        """rr_variance: the per-pixel noise estimate of `img` ((H, W), (H, W, 1) or (H, W, 3) f64) on the device, from
        temporal()'s m2 and n where they are given and a pixel has vr.min_history frames, from a guided window
        otherwise -> the (H, W) plane; variance_estimate of the same arguments, bit for bit."""
        a, m2, count, planes, (H, W, Cn) = _variance_args(img, m2, count, depth, normal, object, albedo)
        var = np.zeros((H, W), np.float64)
        d = vr.desc()
        check(lib().rr_variance(self.h, C.byref(d), W, H, Cn, _dp(a), None if m2 is None else _dp(m2),
                                None if count is None else _ip(count), *_denoise_ptrs(planes), _dp(var)))
        return var

    def variance_device(self, vr, width, height, channels, d_in, d_var, d_m2=None, d_count=None, d_depth=None,
                        d_normal=None, d_object=None, d_albedo=None, stream=None):
        """rr_variance_device: device buffers (ints: device pointers; d_var height * width f64), ordered on `stream`
        (int or None), not synchronised; last_stats() is left as it is."""
        d = vr.desc()
        p = [C.c_void_p(x) if x else None for x in (d_in, d_m2, d_count, d_depth, d_normal, d_object, d_albedo, d_var, stream)]
        check(lib().rr_variance_device(self.h, C.byref(d), width, height, channels, *p))

    def denoise_var(self, img, var, dv, depth=None, normal=None, object=None, albedo=None, return_var=False):
        """rr_denoise_var: `img` filtered on the device under the (H, W) variance plane `var` (variance()'s result or
        the caller's own) -> an array of img's shape, or (image, variance plane of the filtered image) with return_var;
        denoise_var_filter of the same arguments, bit for bit."""
        a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
        v = _var_plane(var, H, W)
        out = np.zeros_like(a)
        vout = np.zeros((H, W), np.float64) if return_var else None
        d = dv.desc()
        check(lib().rr_denoise_var(self.h, C.byref(d), W, H, Cn, _dp(a), _dp(v), *_denoise_ptrs(planes), _dp(out),
                                   None if vout is None else _dp(vout)))
        out = out.reshape(np.shape(img))
        return (out, vout) if return_var else out

    def denoise_var_device(self, dv, width, height, channels, d_in, d_var, d_out, d_var_out=None, d_depth=None,
                           d_normal=None, d_object=None, d_albedo=None, stream=None):
        """rr_denoise_var_device: device buffers (ints: device pointers; d_in and d_out height * width * channels f64,
        d_var and d_var_out height * width f64, d_var_out may be None), ordered on `stream` (int or None), not
        synchronised; last_stats() is left as it is."""
        d = dv.desc()
        p = [C.c_void_p(x) if x else None for x in (d_in, d_var, d_depth, d_normal, d_object, d_albedo, d_out, d_var_out, stream)]
        check(lib().rr_denoise_var_device(self.h, C.byref(d), width, height, channels, *p))


def _spread(q, bits, step):
    out = np.zeros(q.shape, np.uint32)
    for k in range(bits):
        out |= ((q >> np.uint32(k)) & np.uint32(1)) << np.uint32(step * k)
    return out


def ray_order_keys(rays):
    """The sort key of rr_ray_order_device in numpy (rray.h RR_HAS_RAY_ORDER), the kernels' definition and their
    tests' reference: rays (n, 6) f64 (origin, direction) -> (n,) uint32, morton3(qx, qy, qz) << 14 | morton2(qu, qv)
    with the x and u bits lowest.  (u, v): the octahedral map of the direction, in f64 in this order: s = (|dx| + |dy|)
    + |dz|, px = dx / s, py = dy / s; for dz < 0, u = (1 - |py|) * copysign(1, px), v = (1 - |px|) * copysign(1, py),
    else u = px, v = py.  A ray is valid iff its six components, u and v are finite; every other ray has the key
    0xFFFFFFFF.  lo / hi of ox, oy, oz, u, v are taken over the valid rays; q = clamp(floor((c - lo) / (hi - lo) * 2^b),
    0, 2^b - 1) with b = 6 (origin) or 7 (direction), and 0 where the quotient is not finite (hi == lo)."""
    r = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    keys = np.full(len(r), 0xFFFFFFFF, np.uint32)
    with np.errstate(all="ignore"):
        dx, dy, dz = r[:, 3], r[:, 4], r[:, 5]
        s = (np.abs(dx) + np.abs(dy)) + np.abs(dz)
        px, py = dx / s, dy / s
        u = np.where(dz < 0.0, (1.0 - np.abs(py)) * np.copysign(1.0, px), px)
        v = np.where(dz < 0.0, (1.0 - np.abs(px)) * np.copysign(1.0, py), py)
        valid = np.isfinite(r).all(axis=1) & np.isfinite(u) & np.isfinite(v)
        if not valid.any():
            return keys
        q = []
        for c, bits in ((r[:, 0], 6), (r[:, 1], 6), (r[:, 2], 6), (u, 7), (v, 7)):
            lo, hi = c[valid].min(), c[valid].max()
            t = (c[valid] - lo) / (hi - lo)
            f = np.clip(np.floor(t * float(1 << bits)), 0.0, float((1 << bits) - 1))
            q.append(np.where(np.isfinite(t), f, 0.0).astype(np.uint32))
    m3 = _spread(q[0], 6, 3) | (_spread(q[1], 6, 3) << np.uint32(1)) | (_spread(q[2], 6, 3) << np.uint32(2))
    m2 = _spread(q[3], 7, 2) | (_spread(q[4], 7, 2) << np.uint32(1))
    keys[valid] = (m3 << np.uint32(14)) | m2
    return keys


class Lens:
    """rr_lens (rray.h RR_HAS_LENS): `samples` rays per pixel, each through the pixel centre or (pixel_jitter) a point
    uniform in the pixel, from a point of a lens of radius `aperture` (0: a pinhole) focused at camera-space distance
    focal_distance; `seed` seeds the pixel / lens samples (the render's own seed stays the area lights')."""

    def __init__(self, samples=1, pixel_jitter=False, aperture=0.0, focal_distance=1.0, seed=0):
        self.samples, self.pixel_jitter = int(samples), bool(pixel_jitter)
        self.aperture, self.focal_distance, self.seed = float(aperture), float(focal_distance), int(seed)

    def desc(self):
        return _lib.LensDesc(self.samples, 1 if self.pixel_jitter else 0, self.aperture, self.focal_distance,
                             self.seed & 0xFFFFFFFFFFFFFFFF)

    def __repr__(self):
        return (f"Lens(samples={self.samples}, pixel_jitter={self.pixel_jitter}, aperture={self.aperture}, "
                f"focal_distance={self.focal_distance}, seed={self.seed})")


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def lens_hash(seed, ray, k):
    """u(k) of ray `ray` (arrays broadcast) under `seed`: the counter hash of the lens frames, jitter_value(jitter_base(
    seed, ray, path 0), light 0, k >> 1, k & 1) = lowbias32(base ^ k) * 2^-32 in [0, 1) — the area lights' hash with
    the path shading never uses."""
    with np.errstate(over="ignore"):
        i = np.asarray(ray, np.uint64)
        base = (_splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _splitmix64(i)) >> np.uint64(32)).astype(np.uint32)
        return _lowbias32(base ^ np.asarray(k, np.uint32)).astype(np.float64) * (1.0 / 4294967296.0)


def camera_inverse(cam):
    """rr_camera_inverse: the 16 doubles of the camera's inverse as the frames compute it (host only)."""
    out = np.zeros(16, np.float64)
    check(lib().rr_camera_inverse(C.byref(cam), _dp(out)))
    return out


def lens_rays(cam, lens, first_pixel=0, n_pixels=None):
    """The lens frames' rays in numpy (rray.h RR_HAS_LENS), the kernel's definition and its tests' reference: the rays of
    pixels [first_pixel, first_pixel + n_pixels) of `cam` (at output size) under `lens`, (n_pixels * samples, 6) f64 —
    origin, direction; sample s of pixel p = py * W + px is ray i = p * S + s.  Plain f64 in this order, with u(k) =
    lens_hash(lens.seed, i, k) and M = camera_inverse(cam):
      jx, jy = (u(0), u(1)) with pixel_jitter, else (0.5, 0.5); wx = half_width - (px + jx) * pixel_size, wy likewise
      X(x, y, z)[r] = ((M[4r] x + M[4r+1] y) + M[4r+2] z) + M[4r+3] * 1.0
      pinhole (aperture == 0): o = X(0, 0, 0), f = X(wx, wy, -1)
      thin lens: (A, B) = the first of (2 u(2 + 2a) - 1, 2 u(3 + 2a) - 1), a = 0..7, with A A + B B <= 1, else (0, 0);
        o = X(aperture A, aperture B, 0), f = X(wx fd, wy fd, -fd)
      d = f - o, mag = sqrt((dx dx + dy dy) + dz dz), direction d / mag."""
    W, H, S = int(cam.hsize), int(cam.vsize), int(lens.samples)
    n_pixels = W * H - first_pixel if n_pixels is None else n_pixels
    if S < 1 or first_pixel < 0 or n_pixels < 0 or first_pixel + n_pixels > W * H or W * H * S >= 1 << 32:
        raise ValueError("lens_rays: samples >= 1, a pixel window inside the frame and fewer than 2^32 rays")
    M = camera_inverse(cam)
    i = np.arange(first_pixel * S, (first_pixel + n_pixels) * S, dtype=np.uint64)
    p = i // np.uint64(S)
    py = p // np.uint64(W)
    px = p - py * np.uint64(W)

    def u(k):
        return lens_hash(lens.seed, i, k)

    def X(x, y, z):
        return [((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] * 1.0 for r in range(3)]

    half = np.full(len(i), 0.5)
    jx, jy = (u(0), u(1)) if lens.pixel_jitter else (half, half)
    with np.errstate(all="ignore"):
        wx = cam.half_width - (px.astype(np.float64) + jx) * cam.pixel_size
        wy = cam.half_height - (py.astype(np.float64) + jy) * cam.pixel_size
        zero = np.zeros(len(i))
        if lens.aperture == 0.0:
            o, f = X(zero, zero, zero), X(wx, wy, np.full(len(i), -1.0))
        else:
            A, B, found = zero.copy(), zero.copy(), np.zeros(len(i), bool)
            for a in range(8):
                ca, cb = 2.0 * u(2 + 2 * a) - 1.0, 2.0 * u(3 + 2 * a) - 1.0
                take = ~found & (ca * ca + cb * cb <= 1.0)
                A, B = np.where(take, ca, A), np.where(take, cb, B)
                found |= take
            fd = float(lens.focal_distance)
            o, f = X(lens.aperture * A, lens.aperture * B, zero), X(wx * fd, wy * fd, np.full(len(i), -fd))
        dx, dy, dz = f[0] - o[0], f[1] - o[1], f[2] - o[2]
        mag = np.sqrt((dx * dx + dy * dy) + dz * dz)
        return np.stack([o[0], o[1], o[2], dx / mag, dy / mag, dz / mag], axis=1)


def lens_resolve(colours, samples):
    """The lens frames' resolve step in numpy: colours (n_pixels * samples, 3) -> (n_pixels, 3), per channel
    (((c_0 + c_1) + ...) + c_{S-1}) / float(S) — summed in increasing sample order, which matters in f64."""
    S = int(samples)
    c = np.ascontiguousarray(colours, np.float64).reshape(-1, S, 3)
    with np.errstate(all="ignore"):
        acc = c[:, 0].copy()
        for s in range(1, S):
            acc = acc + c[:, s]
        return acc / float(S)


class Ao:
    """rr_ao (rray.h RR_HAS_AO): `samples` occlusion segments of length `radius` per point, cosine-weighted around the
    normal; `seed` seeds their directions (for k = 0 the counters are the lens frames': give the two different seeds)."""

    def __init__(self, samples, radius, seed=0):
        self.samples, self.radius, self.seed = int(samples), float(radius), int(seed)

    def desc(self):
        return _lib.AoDesc(self.samples, 0, self.radius, self.seed & 0xFFFFFFFFFFFFFFFF)

    def __repr__(self):
        return f"Ao(samples={self.samples}, radius={self.radius}, seed={self.seed})"


def ao_directions(normals, ao, first=0):
    """The occlusion directions in numpy (rray.h RR_HAS_AO), the kernel's definition and its tests' reference: normals
    (n, 3) f64, taken as unit -> w (n, K, 3) f64 for points first .. first + n - 1 (their hash indices).  Plain f64 in
    this order, with u(k, j) = lens_hash(ao.seed, i, (k << 21) | j):
      (A, B) = the first of (2 u(k, 2a) - 1, 2 u(k, 2a + 1) - 1), a = 0..7, with A A + B B <= 1, else (0, 0)
      c = sqrt(1.0 - (A A + B B)); s = copysign(1.0, N.z); q = -1.0 / (s + N.z); b = (N.x N.y) q
      T = (1.0 + (s (N.x N.x)) q, s b, -(s N.x)); Bv = (b, s + (N.y N.y) q, -N.y)
      w[r] = (A T[r] + B Bv[r]) + c N[r]."""
    N = np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    n, K = len(N), int(ao.samples)
    if K < 1 or first < 0:
        raise ValueError("ao_directions: samples >= 1 and first >= 0")
    i = (np.arange(n, dtype=np.uint64) + np.uint64(first))[:, None]
    k = np.arange(K, dtype=np.uint32)[None, :] << np.uint32(21)
    A, B, found = np.zeros((n, K)), np.zeros((n, K)), np.zeros((n, K), bool)
    with np.errstate(all="ignore"):
        for a in range(8):
            ca = 2.0 * lens_hash(ao.seed, i, k | np.uint32(2 * a)) - 1.0
            cb = 2.0 * lens_hash(ao.seed, i, k | np.uint32(2 * a + 1)) - 1.0
            take = ~found & (ca * ca + cb * cb <= 1.0)
            A, B = np.where(take, ca, A), np.where(take, cb, B)
            found |= take
        c = np.sqrt(1.0 - (A * A + B * B))
        nx, ny, nz = N[:, 0:1], N[:, 1:2], N[:, 2:3]
        s = np.copysign(1.0, nz)
        q = -1.0 / (s + nz)
        b = (nx * ny) * q
        T = [1.0 + (s * (nx * nx)) * q, s * b, -(s * nx)]
        Bv = [b, s + (ny * ny) * q, -ny]
        return np.stack([(A * T[r] + B * Bv[r]) + c * N[:, r:r + 1] for r in range(3)], axis=2)


def ao_targets(points, normals, ao, first=0):
    """The far ends of the occlusion segments in numpy: target[i][k][r] = P[i][r] + radius * w[i][k][r], (n, K, 3) f64 —
    point i's pairs for is_shadowed are (P[i], target[i][k])."""
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    return P[:, None, :] + float(ao.radius) * ao_directions(normals, ao, first)


def ao_resolve(occluded, samples):
    """The occlusion value in numpy: occluded (n * K,) or (n, K) of 0 / 1 -> (n,) f64, (K - sum_k occluded) / float(K)."""
    K = int(samples)
    c = np.asarray(occluded).astype(np.int64).reshape(-1, K).sum(axis=1)
    return (K - c).astype(np.float64) / float(K)


class Indirect:
    """rr_indirect (rray.h RR_HAS_INDIRECT): `samples` gathered rays per point, cosine-weighted around the normal, each
    traced with `remaining` further reflections / refractions; `seed` seeds their directions (ambient occlusion and the
    lens frames draw from the same counters: give them different seeds)."""

    def __init__(self, samples, remaining=1, seed=0):
        self.samples, self.remaining, self.seed = int(samples), int(remaining), int(seed)

    def desc(self):
        return _lib.IndirectDesc(self.samples, self.remaining, self.seed & 0xFFFFFFFFFFFFFFFF)

    def __repr__(self):
        return f"Indirect(samples={self.samples}, remaining={self.remaining}, seed={self.seed})"


def indirect_rays(points, normals, ind, first=0):
    """The gathered rays in numpy (rray.h RR_HAS_INDIRECT), the kernel's definition and its tests' reference: points and
    unit normals (n, 3) f64 -> (n * K, 6) f64 in camera_rays_device's layout; ray i * K + k is origin points[i] and
    direction ao_directions(normals, ind, first)[i][k], taken as it is, for points first .. first + n - 1 (their hash
    indices)."""
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    w = ao_directions(normals, ind, first)
    K = int(ind.samples)
    if len(w) != len(P):
        raise ValueError("indirect_rays: as many normals as points")
    out = np.empty((len(P), K, 6), np.float64)
    out[:, :, 0:3] = P[:, None, :]
    out[:, :, 3:6] = w
    return out.reshape(-1, 6)


def indirect_resolve(colours, samples):
    """The gathered value in numpy: colours (n * K, 3) -> (n, 3), per channel (((L_0 + L_1) + ...) + L_{K-1}) / float(K),
    summed in increasing k (lens_resolve's sum)."""
    return lens_resolve(colours, samples)


def object_diffuse(scene):
    """material.diffuse of every object of a scene (a SceneBuilder or a YamlScene), read from scene.desc():
    mat[material[id]][1], (n_objects,) f64 — what indirect_compose weighs the bounce with.  A group or a CSG node has
    no material (material[id] < 0) and is never a sample's first hit: 0.0."""
    d = scene.desc()
    n = int(d.n_objects)
    return np.array([d.mat[7 * d.material[i] + 1] if d.material[i] >= 0 else 0.0 for i in range(n)], np.float64)


def indirect_compose(base, indirect, albedo, object, diffuse):
    """A colour frame plus its bounce, per sample in plain f64 in this order: base + (albedo * diffuse[object]) * indirect
    where object >= 0, base elsewhere.  base, indirect, albedo: (H, W, 3) f64 (render, render_indirect and render_aov's
    albedo plane, or their filtered forms); object: (H, W) int32 (render_aov's object plane); diffuse: object_diffuse."""
    base = np.asarray(base, np.float64)
    ind = np.asarray(indirect, np.float64).reshape(base.shape)
    alb = np.asarray(albedo, np.float64).reshape(base.shape)
    obj = np.asarray(object).reshape(base.shape[:-1])
    kd = np.asarray(diffuse, np.float64)
    hit = obj >= 0
    with np.errstate(all="ignore"):
        w = alb * kd[np.where(hit, obj, 0)][..., None]
        return np.where(hit[..., None], base + w * ind, base)


class Denoise:
    """rr_denoise_desc (rray.h RR_HAS_DENOISE): `iterations` a-trous levels (level i has holes of 2^i pixels); a sigma
    of 0 switches its term off; object=True skips taps on another object id (leave it off for meshes: every triangle
    is an object)."""

    def __init__(self, iterations, sigma_color=0.0, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1, object=False):
        self.iterations = int(iterations)
        self.sigma_color, self.sigma_normal = float(sigma_color), float(sigma_normal)
        self.sigma_depth, self.sigma_albedo = float(sigma_depth), float(sigma_albedo)
        self.object = bool(object)

    def desc(self):
        return _lib.DenoiseDesc(self.iterations, _lib.RR_DN_OBJECT if self.object else 0, self.sigma_color,
                                self.sigma_normal, self.sigma_depth, self.sigma_albedo)

    def __repr__(self):
        return (f"Denoise(iterations={self.iterations}, sigma_color={self.sigma_color}, sigma_normal={self.sigma_normal}, "
                f"sigma_depth={self.sigma_depth}, sigma_albedo={self.sigma_albedo}, object={self.object})")


def _denoise_args(img, depth, normal, object, albedo):
    """The image as a contiguous (H, W, C) f64 array, the planes as contiguous arrays of rr_denoise's types (None stays
    None), and (H, W, C)."""
    a = np.ascontiguousarray(img, np.float64)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3:
        raise ValueError("denoise: the image is (H, W), (H, W, 1) or (H, W, 3)")
    H, W, Cn = a.shape
    planes = {"depth": (depth, np.float64, (H, W)), "normal": (normal, np.float64, (H, W, 3)),
              "object": (object, np.int32, (H, W)), "albedo": (albedo, np.float64, (H, W, 3))}
    out = {}
    for k, (v, t, shape) in planes.items():
        if v is None:
            out[k] = None
            continue
        v = np.ascontiguousarray(v, t)
        if v.shape != shape:
            raise ValueError(f"denoise: the {k} plane has shape {v.shape}, the image needs {shape}")
        out[k] = v
    return a, out, (H, W, Cn)


def _denoise_ptrs(planes):
    return [None if planes[k] is None else (_ip(planes[k]) if k == "object" else _dp(planes[k]))
            for k in ("depth", "normal", "object", "albedo")]


def denoise_reference(img, dn, depth=None, normal=None, object=None, albedo=None):
    """rr_denoise_reference: the C definition on the host (single thread, no device), by the function the kernel calls."""
    a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
    out = np.zeros_like(a)
    d = dn.desc()
    check(lib().rr_denoise_reference(C.byref(d), W, H, Cn, _dp(a), *_denoise_ptrs(planes), _dp(out)))
    return out.reshape(np.shape(img))


def denoise_filter(img, dn, depth=None, normal=None, object=None, albedo=None):
    """The denoiser in numpy (rray.h RR_HAS_DENOISE), the kernel's definition and its tests' reference, vectorised over
    the frame: 25 shifted slices per level.  Guides are rounded to f32 and widened; plain f64 in the header's order:
      void(p): depth given and not z_p < inf, or object given and id_p < 0; a void pixel keeps its value
      per level i (s = 2^i, sc = sigma_color 2^-i), taps dy = -2..2 (outer), dx = -2..2 (inner), q = p + (dx s, dy s)
      inside the frame and not void: w = h[dy+2] h[dx+2]; off-centre taps take the terms that are on, each skipping the
      tap unless its t > 0: object (id_q == id_p); colour t = 1 + dc / (sc sc), w *= 1 / (t t); normal
      t = 1 - max(1 - dot, 0) / sigma_normal, w *= t t; depth t = 1 - |z_p - z_q| / ((sigma_depth |z_p|) max(|dx|,|dy|) s);
      albedo t = 1 - da / (sigma_albedo sigma_albedo); taps with w > 0 add w F[q] to acc and w to ws; F' = acc / ws."""
    a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
    I = int(dn.iterations)
    sig = (dn.sigma_color, dn.sigma_normal, dn.sigma_depth, dn.sigma_albedo)
    if not 1 <= I <= _lib.RR_MAX_DENOISE_ITERATIONS or Cn not in (1, 3) or W < 1 or H < 1:
        raise ValueError("denoise_filter: iterations in 1..8, 1 or 3 channels, a frame of at least one pixel")
    if not all(math.isfinite(x) and x >= 0.0 for x in sig):
        raise ValueError("denoise_filter: every sigma is finite and >= 0")
    on_c, on_n, on_z, on_a = (x > 0.0 for x in sig)
    if (dn.object and planes["object"] is None) or (on_n and planes["normal"] is None) or \
            (on_z and planes["depth"] is None) or (on_a and planes["albedo"] is None):
        raise ValueError("denoise_filter: a term that is switched on needs its plane")
    with np.errstate(all="ignore"):
        f32 = lambda v: None if v is None else v.astype(np.float32).astype(np.float64)  # noqa: E731
        z, nrm, alb, ids = f32(planes["depth"]), f32(planes["normal"]), f32(planes["albedo"]), planes["object"]
        void = np.zeros((H, W), bool)
        if z is not None:
            void |= ~(z < np.inf)
        if ids is not None:
            void |= ids < 0
        h = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
        F = a
        for i in range(I):
            s = 1 << i
            sc = dn.sigma_color * (1.0 / float(s))
            sc2 = np.float64(sc) * np.float64(sc)
            sa2 = np.float64(dn.sigma_albedo) * np.float64(dn.sigma_albedo)
            acc = np.zeros((H, W, Cn))
            ws = np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * s, dy * s
                    if abs(ox) >= W or abs(oy) >= H:
                        continue
                    # p over the pixels whose tap lies inside the frame, q the tap
                    P = (slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox)))
                    Q = (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox)))
                    ok = ~void[P] & ~void[Q]
                    w = np.full(ok.shape, h[dy + 2] * h[dx + 2])
                    Fp, Fq = F[P], F[Q]
                    if dx or dy:
                        if dn.object:
                            ok &= ids[Q] == ids[P]
                        if on_c:
                            d = Fp - Fq
                            dc = d[..., 0] * d[..., 0]
                            if Cn == 3:
                                dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                            t = 1.0 + dc / sc2
                            ok &= t > 0.0
                            w = w * (1.0 / (t * t))
                        if on_n:
                            np_, nq = nrm[P], nrm[Q]
                            dot = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
                            e = 1.0 - dot
                            e = np.where(e < 0.0, 0.0, e)
                            t = 1.0 - e / dn.sigma_normal
                            ok &= t > 0.0
                            w = w * (t * t)
                        if on_z:
                            r = float(max(abs(dx), abs(dy)) * s)
                            t = 1.0 - np.abs(z[P] - z[Q]) / ((dn.sigma_depth * np.abs(z[P])) * r)
                            ok &= t > 0.0
                            w = w * (t * t)
                        if on_a:
                            da_ = alb[P] - alb[Q]
                            da = (da_[..., 0] * da_[..., 0] + da_[..., 1] * da_[..., 1]) + da_[..., 2] * da_[..., 2]
                            t = 1.0 - da / sa2
                            ok &= t > 0.0
                            w = w * (t * t)
                    ok &= w > 0.0
                    # a tap that is skipped adds nothing: x + 0.0 keeps every x the sums can hold (they are never -0.0)
                    acc[P] = np.where(ok[..., None], acc[P] + w[..., None] * Fq, acc[P])
                    ws[P] = np.where(ok, ws[P] + w, ws[P])
            F = np.where(void[..., None], F, acc / np.where(void, 1.0, ws)[..., None])
    return F.reshape(np.shape(img))


class Variance:
    """rr_variance_desc (rray.h RR_HAS_DENOISE_VAR): a pixel whose history holds at least `min_history` frames takes
    its variance from rr_temporal's moments, the others from a guided 7 x 7 window of the image; a sigma of 0 switches
    its guide term off; object=True skips taps on another object id."""

    def __init__(self, min_history=4, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.0, object=False):
        self.min_history = int(min_history)
        self.sigma_normal, self.sigma_depth, self.sigma_albedo = float(sigma_normal), float(sigma_depth), float(sigma_albedo)
        self.object = bool(object)

    def desc(self):
        return _lib.VarianceDesc(_lib.RR_DN_OBJECT if self.object else 0, self.min_history, self.sigma_normal,
                                 self.sigma_depth, self.sigma_albedo)

    def __repr__(self):
        return (f"Variance(min_history={self.min_history}, sigma_normal={self.sigma_normal}, sigma_depth={self.sigma_depth}, "
                f"sigma_albedo={self.sigma_albedo}, object={self.object})")


class DenoiseVar:
    """rr_denoise_var_desc (rray.h RR_HAS_DENOISE_VAR): Denoise's fields, with `sigma_color` in standard deviations of
    each pixel's own noise (not halved per level), and `epsilon`, the squared colour tolerance of a noise-free pixel."""

    def __init__(self, iterations, sigma_color=4.0, epsilon=1e-12, sigma_normal=0.25, sigma_depth=0.05, sigma_albedo=0.1,
                 object=False):
        self.iterations = int(iterations)
        self.sigma_color, self.epsilon = float(sigma_color), float(epsilon)
        self.sigma_normal, self.sigma_depth, self.sigma_albedo = float(sigma_normal), float(sigma_depth), float(sigma_albedo)
        self.object = bool(object)

    def desc(self):
        return _lib.DenoiseVarDesc(self.iterations, _lib.RR_DN_OBJECT if self.object else 0, self.sigma_color,
                                   self.sigma_normal, self.sigma_depth, self.sigma_albedo, self.epsilon)

    def __repr__(self):
        return (f"DenoiseVar(iterations={self.iterations}, sigma_color={self.sigma_color}, epsilon={self.epsilon}, "
                f"sigma_normal={self.sigma_normal}, sigma_depth={self.sigma_depth}, sigma_albedo={self.sigma_albedo}, "
                f"object={self.object})")


def _variance_args(img, m2, count, depth, normal, object, albedo):
    """_denoise_args and the moments and counts as contiguous arrays of rr_variance's types (None stays None)."""
    a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
    if (m2 is None) != (count is None):
        raise ValueError("variance: m2 and count go together")
    if m2 is not None:
        m2 = np.ascontiguousarray(m2, np.float64).reshape(H, W, Cn)
        count = np.ascontiguousarray(count, np.int32)
        if count.shape != (H, W):
            raise ValueError(f"variance: the counts have shape {count.shape}, the image needs {(H, W)}")
    return a, m2, count, planes, (H, W, Cn)


def _var_plane(var, H, W):
    v = np.ascontiguousarray(var, np.float64)
    if v.shape != (H, W):
        raise ValueError(f"denoise_var: the variance plane has shape {v.shape}, the image needs {(H, W)}")
    return v


def variance_reference(img, vr, m2=None, count=None, depth=None, normal=None, object=None, albedo=None):
    """rr_variance_reference: the C definition on the host (single thread, no device), by the function the kernel calls
    -> the (H, W) variance plane."""
    a, m2, count, planes, (H, W, Cn) = _variance_args(img, m2, count, depth, normal, object, albedo)
    var = np.zeros((H, W), np.float64)
    d = vr.desc()
    check(lib().rr_variance_reference(C.byref(d), W, H, Cn, _dp(a), None if m2 is None else _dp(m2),
                                      None if count is None else _ip(count), *_denoise_ptrs(planes), _dp(var)))
    return var


def denoise_var_reference(img, var, dv, depth=None, normal=None, object=None, albedo=None, return_var=False):
    """rr_denoise_var_reference: the C definition on the host -> the filtered image, or (image, (H, W) variance of the
    filtered image) with return_var."""
    a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
    v = _var_plane(var, H, W)
    out = np.zeros_like(a)
    vout = np.zeros((H, W), np.float64) if return_var else None
    d = dv.desc()
    check(lib().rr_denoise_var_reference(C.byref(d), W, H, Cn, _dp(a), _dp(v), *_denoise_ptrs(planes), _dp(out),
                                         None if vout is None else _dp(vout)))
    out = out.reshape(np.shape(img))
    return (out, vout) if return_var else out


def _dv_guides(planes, H, W):
    """The guides as the definition reads them (rounded to f32 and widened) and the void mask."""
    f32 = lambda v: None if v is None else v.astype(np.float32).astype(np.float64)  # noqa: E731
    z, nrm, alb, ids = f32(planes["depth"]), f32(planes["normal"]), f32(planes["albedo"]), planes["object"]
    void = np.zeros((H, W), bool)
    if z is not None:
        void |= ~(z < np.inf)
    if ids is not None:
        void |= ids < 0
    return z, nrm, alb, ids, void


def _dv_guide_terms(ok, w, P, Q, reach, g, on_o, sigma_normal, sigma_depth, sigma_albedo):
    """The guide terms of rr_denoise (object, normal, depth, albedo, in this order) of the taps Q seen from the pixels
    P, applied to the weights w -> (ok, w): a term whose t is not > 0 clears ok."""
    z, nrm, alb, ids, _ = g
    if on_o:
        ok = ok & (ids[Q] == ids[P])
    if sigma_normal > 0.0:
        np_, nq = nrm[P], nrm[Q]
        dot = (np_[..., 0] * nq[..., 0] + np_[..., 1] * nq[..., 1]) + np_[..., 2] * nq[..., 2]
        e = 1.0 - dot
        e = np.where(e < 0.0, 0.0, e)
        t = 1.0 - e / sigma_normal
        ok = ok & (t > 0.0)
        w = w * (t * t)
    if sigma_depth > 0.0:
        t = 1.0 - np.abs(z[P] - z[Q]) / ((sigma_depth * np.abs(z[P])) * float(reach))
        ok = ok & (t > 0.0)
        w = w * (t * t)
    if sigma_albedo > 0.0:
        sa2 = np.float64(sigma_albedo) * np.float64(sigma_albedo)
        da_ = alb[P] - alb[Q]
        da = (da_[..., 0] * da_[..., 0] + da_[..., 1] * da_[..., 1]) + da_[..., 2] * da_[..., 2]
        t = 1.0 - da / sa2
        ok = ok & (t > 0.0)
        w = w * (t * t)
    return ok, w


def _dv_check_terms(who, obj, sigmas, planes):
    if not all(math.isfinite(x) and x >= 0.0 for x in sigmas):
        raise ValueError(f"{who}: every sigma is finite and >= 0")
    sn, sz, sa = sigmas[-3:]
    if (obj and planes["object"] is None) or (sn > 0.0 and planes["normal"] is None) or \
            (sz > 0.0 and planes["depth"] is None) or (sa > 0.0 and planes["albedo"] is None):
        raise ValueError(f"{who}: a term that is switched on needs its plane")


def _shifted(H, W, ox, oy):
    """(P, Q): the pixels whose tap at offset (ox, oy) lies inside the frame, and the taps"""
    return ((slice(max(0, -oy), H - max(0, oy)), slice(max(0, -ox), W - max(0, ox))),
            (slice(max(0, oy), H - max(0, -oy)), slice(max(0, ox), W - max(0, -ox))))


def _channel_sum(v):
    return (v[..., 0] + v[..., 1]) + v[..., 2] if v.shape[-1] == 3 else v[..., 0]


def variance_estimate(img, vr, m2=None, count=None, depth=None, normal=None, object=None, albedo=None):
    """The per-pixel noise estimate in numpy (rray.h RR_HAS_DENOISE_VAR), the kernel's definition and its tests'
    reference, vectorised over the frame with shifted slices -> the (H, W) plane.  Plain f64 in the header's order:
      void(p): V = 0
      count given and count[p] >= min_history: v_c = max(m2 - in in, 0) (a NaN gives 0); V = sum_c v_c / count[p]
      otherwise, over dy = -3..3 (outer), dx = -3..3 (inner), q = p + (dx, dy) inside the frame and not void: w = 1,
      off-centre taps take denoise_filter's object, normal, depth and albedo terms with step 1; taps with w > 0 add
      w in[q] to s1, w (in[q] in[q]) to s2 and w to ws; m = s1 / ws, v_c = max(s2 / ws - m m, 0); V = sum_c v_c."""
    a, m2, count, planes, (H, W, Cn) = _variance_args(img, m2, count, depth, normal, object, albedo)
    if Cn not in (1, 3) or W < 1 or H < 1 or not 0 <= vr.min_history <= _lib.RR_MAX_TEMPORAL_HISTORY:
        raise ValueError("variance_estimate: 1 or 3 channels, a frame of at least one pixel, min_history in 0..2^20")
    sig = (vr.sigma_normal, vr.sigma_depth, vr.sigma_albedo)
    _dv_check_terms("variance_estimate", vr.object, sig, planes)
    with np.errstate(all="ignore"):
        g = _dv_guides(planes, H, W)
        void = g[4]
        s1, s2, ws = np.zeros((H, W, Cn)), np.zeros((H, W, Cn)), np.zeros((H, W))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if abs(dx) >= W or abs(dy) >= H:
                    continue
                P, Q = _shifted(H, W, dx, dy)
                ok = ~void[P] & ~void[Q]
                w = np.ones(ok.shape)
                if dx or dy:
                    ok, w = _dv_guide_terms(ok, w, P, Q, max(abs(dx), abs(dy)), g, vr.object, *sig)
                ok = ok & (w > 0.0)
                Fq = a[Q]
                # a tap that is skipped adds nothing (the sums are kept, not increased by 0.0)
                s1[P] = np.where(ok[..., None], s1[P] + w[..., None] * Fq, s1[P])
                s2[P] = np.where(ok[..., None], s2[P] + w[..., None] * (Fq * Fq), s2[P])
                ws[P] = np.where(ok, ws[P] + w, ws[P])
        m = s1 / ws[..., None]
        v = s2 / ws[..., None] - m * m
        V = _channel_sum(np.where(v > 0.0, v, 0.0))
        if count is not None:
            vt = m2 - a * a
            Vt = _channel_sum(np.where(vt > 0.0, vt, 0.0)) / count.astype(np.float64)
            V = np.where(count >= vr.min_history, Vt, V)
        return np.where(void, 0.0, V)


def denoise_var_filter(img, var, dv, depth=None, normal=None, object=None, albedo=None, return_var=False):
    """The variance-guided filter in numpy (rray.h RR_HAS_DENOISE_VAR), the kernel's definition and its tests'
    reference, vectorised over the frame: 9 + 25 shifted slices per level -> the filtered image, or (image, variance
    plane of the filtered image) with return_var.  denoise_filter's levels with two differences.  The colour term of an
    off-centre tap, applied after the guide terms, is t = 1 + dc / den, w *= 1 / (t t) with den = (sigma_color
    sigma_color) gv + epsilon, sigma_color not halved per level and gv the 3 x 3 binomial (1/4, 1/2, 1/4) of the
    level's variance plane around p over the pixels that are inside the frame and not void.  And the variance is
    carried along: V' = sum (w w) V[q] / (ws ws) beside F' = sum w F[q] / ws; a void pixel keeps both."""
    a, planes, (H, W, Cn) = _denoise_args(img, depth, normal, object, albedo)
    V = _var_plane(var, H, W)
    I = int(dv.iterations)
    if not 1 <= I <= _lib.RR_MAX_DENOISE_ITERATIONS or Cn not in (1, 3) or W < 1 or H < 1:
        raise ValueError("denoise_var_filter: iterations in 1..8, 1 or 3 channels, a frame of at least one pixel")
    if not (math.isfinite(dv.epsilon) and dv.epsilon > 0.0):
        raise ValueError("denoise_var_filter: epsilon is finite and > 0")
    sig = (dv.sigma_normal, dv.sigma_depth, dv.sigma_albedo)
    _dv_check_terms("denoise_var_filter", dv.object, (dv.sigma_color,) + sig, planes)
    with np.errstate(all="ignore"):
        g = _dv_guides(planes, H, W)
        void = g[4]
        h = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
        b = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)
        sc2 = np.float64(dv.sigma_color) * np.float64(dv.sigma_color)
        F = a
        for i in range(I):
            s = 1 << i
            ga, gs = np.zeros((H, W)), np.zeros((H, W))
            for ey in range(-1, 2):
                for ex in range(-1, 2):
                    if abs(ex) >= W or abs(ey) >= H:
                        continue
                    P, Q = _shifted(H, W, ex, ey)
                    ok = ~void[P] & ~void[Q]
                    gw = b[ey + 1] * b[ex + 1]
                    ga[P] = np.where(ok, ga[P] + gw * V[Q], ga[P])
                    gs[P] = np.where(ok, gs[P] + gw, gs[P])
            den = sc2 * (ga / gs) + dv.epsilon
            acc, va, ws = np.zeros((H, W, Cn)), np.zeros((H, W)), np.zeros((H, W))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ox, oy = dx * s, dy * s
                    if abs(ox) >= W or abs(oy) >= H:
                        continue
                    P, Q = _shifted(H, W, ox, oy)
                    ok = ~void[P] & ~void[Q]
                    w = np.full(ok.shape, h[dy + 2] * h[dx + 2])
                    Fq = F[Q]
                    if dx or dy:
                        ok, w = _dv_guide_terms(ok, w, P, Q, max(abs(dx), abs(dy)) * s, g, dv.object, *sig)
                        if dv.sigma_color > 0.0:
                            d = F[P] - Fq
                            dc = d[..., 0] * d[..., 0]
                            if Cn == 3:
                                dc = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                            t = 1.0 + dc / den[P]
                            ok = ok & (t > 0.0)
                            w = w * (1.0 / (t * t))
                    ok = ok & (w > 0.0)
                    acc[P] = np.where(ok[..., None], acc[P] + w[..., None] * Fq, acc[P])
                    va[P] = np.where(ok, va[P] + (w * w) * V[Q], va[P])
                    ws[P] = np.where(ok, ws[P] + w, ws[P])
            F = np.where(void[..., None], F, acc / ws[..., None])
            V = np.where(void, V, va / (ws * ws))
    F = F.reshape(np.shape(img))
    return (F, V) if return_var else F


class Temporal:
    """rr_temporal_desc (rray.h RR_HAS_TEMPORAL): the history length is capped at `max_history`; `alpha` is the floor of
    the blend factor (0: a running mean); a sigma of 0 switches its term off; object=True skips taps on another object
    id."""

    def __init__(self, max_history=32, alpha=0.0, sigma_plane=0.01, sigma_normal=0.1, object=True):
        self.max_history = int(max_history)
        self.alpha, self.sigma_plane, self.sigma_normal = float(alpha), float(sigma_plane), float(sigma_normal)
        self.object = bool(object)

    def desc(self):
        return _lib.TemporalDesc(_lib.RR_TP_OBJECT if self.object else 0, self.max_history, self.alpha, self.sigma_plane,
                                 self.sigma_normal)

    def __repr__(self):
        return (f"Temporal(max_history={self.max_history}, alpha={self.alpha}, sigma_plane={self.sigma_plane}, "
                f"sigma_normal={self.sigma_normal}, object={self.object})")


def _temporal_args(img, depth, normal, object, prev, moments):
    """The current frame and the history as contiguous arrays of rr_temporal's types -> (a, cur, hist, (H, W, C)).
    prev=None is a history of zero counts over the current planes."""
    if depth is None:
        raise ValueError("temporal: the depth plane is required")
    a, cur, (H, W, Cn) = _denoise_args(img, depth, normal, object, None)
    if prev is None:
        hist = {"out": np.zeros_like(a), "n": np.zeros((H, W), np.int32), "m2": np.zeros_like(a) if moments else None,
                "depth": cur["depth"], "normal": cur["normal"], "object": cur["object"]}
        return a, cur, hist, (H, W, Cn)
    if prev.get("out") is None or prev.get("n") is None or prev.get("depth") is None:
        raise ValueError("temporal: a history holds at least out, n and depth")
    pa, planes, shape = _denoise_args(prev["out"], prev["depth"], prev.get("normal"), prev.get("object"), None)
    if shape != (H, W, Cn):
        raise ValueError(f"temporal: the history has shape {shape}, the image {(H, W, Cn)}")
    n = np.ascontiguousarray(prev["n"], np.int32)
    if n.shape != (H, W):
        raise ValueError(f"temporal: the history's counts have shape {n.shape}, the image needs {(H, W)}")
    m2 = None
    if moments:
        if prev.get("m2") is None:
            raise ValueError("temporal: moments=True needs a history with m2")
        m2 = np.ascontiguousarray(prev["m2"], np.float64).reshape(H, W, Cn)
    return a, cur, {"out": pa, "n": n, "m2": m2, **planes}, (H, W, Cn)


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _temporal_call(entry, img, tp, cam, prev_cam, depth, normal, object, prev, moments):
    a, cur, hist, (H, W, Cn) = _temporal_args(img, depth, normal, object, prev, moments)
    out, n = np.zeros_like(a), np.zeros((H, W), np.int32)
    m2 = np.zeros_like(a) if moments else None
    d = tp.desc()
    fc = _lib.TemporalFrame(_vp(a), _vp(cur["depth"]), _vp(cur["normal"]), _vp(cur["object"]), None, None)
    fp = _lib.TemporalFrame(_vp(hist["out"]), _vp(hist["depth"]), _vp(hist["normal"]), _vp(hist["object"]), _vp(hist["n"]),
                            _vp(hist["m2"]))
    check(entry(C.byref(d), W, H, Cn, C.byref(cam), C.byref(fc), C.byref(prev_cam), C.byref(fp), _vp(out), _vp(n), _vp(m2)))
    shape = np.shape(img)
    return {"out": out.reshape(shape), "n": n, "m2": None if m2 is None else m2.reshape(shape), "depth": cur["depth"],
            "normal": cur["normal"], "object": cur["object"]}


def temporal_reference(img, tp, cam, prev_cam, depth, normal=None, object=None, prev=None, moments=False):
    """rr_temporal_reference: the C definition on the host (single thread, no device), by the function the kernel calls.
    Renderer.temporal's arguments and result."""
    return _temporal_call(lib().rr_temporal_reference, img, tp, cam, prev_cam, depth, normal, object, prev, moments)


def temporal_variance(out, m2):
    """The per-pixel variance estimate of an accumulated image and its second moments: maximum(m2 - out * out, 0)."""
    out, m2 = np.asarray(out, np.float64), np.asarray(m2, np.float64)
    return np.maximum(m2 - out * out, 0.0)


def _camera_fields(cam):
    return (cam.hsize, cam.vsize, cam.field_of_view, cam.pixel_size, cam.half_width, cam.half_height) + tuple(cam.transform)


def temporal_filter(img, tp, cam, prev_cam, depth, normal=None, object=None, prev=None, moments=False,
                    return_history=False):
    """Temporal accumulation in numpy (rray.h RR_HAS_TEMPORAL), the kernel's definition and its tests' reference,
    vectorised over the frame: Renderer.temporal's arguments and result.  Plain f64 in the header's order, with
    M = camera_inverse(cam), M' = camera_inverse(prev_cam), T' = prev_cam.transform:
      void(p): not z_p < inf, or object given and id_p < 0: out = in, n = 1, m2 = in in
      P = o + z d of the pinhole ray through the pixel centre
      static cameras (every field ==): the one tap q = p, w = 1, te = z
      else c = T' P; no tap unless c_z < 0; fx = (half_width' - c_x / -c_z) / pixel_size' - 0.5, fy likewise; no tap
      unless -1 < fx < W and -1 < fy < H; the four bilinear taps around (fx, fy), te = |P - o'|
      a tap is skipped when it lies outside the frame, is void or has count < 1 in the history, lies on another object
      (tp.object), has 1 - n_p.n_q > sigma_normal, lies further than sigma_plane te from p's tangent plane, or w is not > 0
      h = sum w hist / sum w; n = min(min count + 1, max_history); a = max(1 / n, alpha); out = h + (in - h) a
    return_history=True adds h (NaN where no tap survived), ws, fx and fy to the result."""
    a, cur, hist, (H, W, Cn) = _temporal_args(img, depth, normal, object, prev, moments)
    sig = (tp.sigma_plane, tp.sigma_normal)
    if Cn not in (1, 3) or not 1 <= tp.max_history <= _lib.RR_MAX_TEMPORAL_HISTORY or not 0.0 <= tp.alpha <= 1.0 or \
            not all(math.isfinite(x) and x >= 0.0 for x in sig):
        raise ValueError("temporal_filter: 1 or 3 channels, max_history in 1..2^20, alpha in 0..1, sigmas finite and >= 0")
    on_p, on_n = (x > 0.0 for x in sig)
    if (tp.object and (cur["object"] is None or hist["object"] is None)) or (on_p and cur["normal"] is None) or \
            (on_n and (cur["normal"] is None or hist["normal"] is None)):
        raise ValueError("temporal_filter: a term that is switched on needs its planes")
    if (cam.hsize, cam.vsize, prev_cam.hsize, prev_cam.vsize) != (W, H, W, H):
        raise ValueError("temporal_filter: both cameras must have the frame's size")
    M, Mp = camera_inverse(cam), camera_inverse(prev_cam)
    T = np.array(list(prev_cam.transform), np.float64)

    def X(m, x, y, z):
        return [((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] * 1.0 for r in range(3)]

    def dirs(m, c, o, xs, ys):
        wx = c.half_width - (xs.astype(np.float64) + 0.5) * c.pixel_size
        wy = c.half_height - (ys.astype(np.float64) + 0.5) * c.pixel_size
        f = X(m, wx, wy, -1.0)
        d = [f[r] - o[r] for r in range(3)]
        mag = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return [d[r] / mag for r in range(3)]

    with np.errstate(all="ignore"):
        z, ids, nrm = cur["depth"], cur["object"], cur["normal"]
        pz, pid, pn, pcnt, pimg, pm2 = hist["depth"], hist["object"], hist["normal"], hist["n"], hist["out"], hist["m2"]
        void = ~(z < np.inf)
        if ids is not None:
            void |= ids < 0
        pvoid = ~(pz < np.inf)
        if pid is not None:
            pvoid |= pid < 0
        ys, xs = np.mgrid[0:H, 0:W]
        o = [np.float64(v) for v in X(M, 0.0, 0.0, 0.0)]
        op = [np.float64(v) for v in X(Mp, 0.0, 0.0, 0.0)]
        d = dirs(M, cam, o, xs, ys)
        P = [o[r] + z * d[r] for r in range(3)]
        cand = ~void
        if all(u == v for u, v in zip(_camera_fields(cam), _camera_fields(prev_cam))):  # a NaN is unequal to itself
            taps = [(xs, ys, np.ones((H, W)))]
            te = z
            fx, fy = xs.astype(np.float64), ys.astype(np.float64)
        else:
            c = [((T[4 * r] * P[0] + T[4 * r + 1] * P[1]) + T[4 * r + 2] * P[2]) + T[4 * r + 3] * 1.0 for r in range(3)]
            cand &= c[2] < 0.0
            m = -c[2]
            sx, sy = c[0] / m, c[1] / m
            fx = (prev_cam.half_width - sx) / prev_cam.pixel_size - 0.5
            fy = (prev_cam.half_height - sy) / prev_cam.pixel_size - 0.5
            cand &= (fx > -1.0) & (fx < float(W)) & (fy > -1.0) & (fy < float(H))
            fx0, fy0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - fx0, fy - fy0
            x0 = np.where(cand, fx0, 0.0).astype(np.int64)
            y0 = np.where(cand, fy0, 0.0).astype(np.int64)
            taps = [(x0 + i, y0 + j, (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)) for j in (0, 1) for i in (0, 1)]
            e = [P[r] - op[r] for r in range(3)]
            te = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        acc, accm2 = np.zeros((H, W, Cn)), np.zeros((H, W, Cn))
        ws = np.zeros((H, W))
        nmin = np.full((H, W), np.iinfo(np.int32).max, np.int64)
        cnt = np.zeros((H, W), np.int64)
        for qx, qy, w in taps:
            ok = cand & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            ok &= ~pvoid[qy, qx]
            nq = pcnt[qy, qx].astype(np.int64)
            ok &= nq >= 1
            if tp.object:
                ok &= pid[qy, qx] == ids
            if on_n:
                nqv = pn[qy, qx]
                dot = (nrm[..., 0] * nqv[..., 0] + nrm[..., 1] * nqv[..., 1]) + nrm[..., 2] * nqv[..., 2]
                ok &= (1.0 - dot) <= tp.sigma_normal
            if on_p:
                dq = dirs(Mp, prev_cam, op, qx, qy)
                zq = pz[qy, qx]
                Q = [op[r] + zq * dq[r] for r in range(3)]
                g = (nrm[..., 0] * (Q[0] - P[0]) + nrm[..., 1] * (Q[1] - P[1])) + nrm[..., 2] * (Q[2] - P[2])
                ok &= np.abs(g) <= tp.sigma_plane * te
            ok &= w > 0.0
            acc = np.where(ok[..., None], acc + w[..., None] * pimg[qy, qx], acc)
            if pm2 is not None:
                accm2 = np.where(ok[..., None], accm2 + w[..., None] * pm2[qy, qx], accm2)
            ws = np.where(ok, ws + w, ws)
            nmin = np.where(ok, np.minimum(nmin, nq), nmin)
            cnt += ok
        keep = cnt > 0
        n = np.where(keep, np.minimum(nmin + 1, tp.max_history), 1).astype(np.int32)
        bl = 1.0 / n.astype(np.float64)
        bl = np.where(bl < tp.alpha, tp.alpha, bl)[..., None]
        h = acc / ws[..., None]
        out = np.where(keep[..., None], h + (a - h) * bl, a)
        m2 = None
        if pm2 is not None:
            hm2 = accm2 / ws[..., None]
            m2 = np.where(keep[..., None], hm2 + (a * a - hm2) * bl, a * a)
    shape = np.shape(img)
    res = {"out": out.reshape(shape), "n": n, "m2": None if m2 is None else m2.reshape(shape), "depth": cur["depth"],
           "normal": cur["normal"], "object": cur["object"]}
    if return_history:
        res.update(h=np.where(keep[..., None], h, np.nan), ws=ws, fx=fx, fy=fy)
    return res


def adaptive_mask(frame, threshold):
    """The adaptive frames' criterion in numpy (rray.h rr_render_adaptive, rule 2): pixel p of frame (H, W, 3) is
    refined iff some q of its 3x3 neighbourhood, clipped to the frame (q = p included), has
    !(max_c |frame[p][c] - frame[q][c]| <= threshold).  A NaN colour refines its neighbourhood; threshold < 0 refines
    every pixel.  -> (H, W) bool.  A preview of what Renderer.render_adaptive will supersample, and its tests' reference."""
    f = np.asarray(frame, np.float64)
    if f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"adaptive_mask: frame must have shape (H, W, 3); got {f.shape}")
    if threshold != threshold:
        raise ValueError("adaptive_mask: the threshold is NaN")
    H, W = f.shape[:2]
    out = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore"):  # inf - inf is NaN, which refines
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
                yq, xq = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
                d = np.max(np.abs(f[ys, xs] - f[yq, xq]), axis=2)  # np.max propagates NaN
                out[ys, xs] |= ~(d <= threshold)
    return out


def quantize(avg):
    """canvas.rs:97-100: `(v*255.0) as u8` per channel + alpha 255."""
    avg = np.ascontiguousarray(avg, np.float64)
    n = avg.shape[0] * avg.shape[1]
    out = np.zeros((avg.shape[0], avg.shape[1], 4), np.uint8)
    check(lib().rr_quantize(_dp(avg), n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


def write_png(path, rgba):
    rgba = np.ascontiguousarray(rgba, np.uint8)
    check(lib().rr_write_png(path.encode(), rgba.ctypes.data_as(C.POINTER(C.c_uint8)), rgba.shape[1], rgba.shape[0]))


def render_scene_from_str(text, width, height, png_file, aa=1, device=0, obj_root=None):
    """scene_builder_yaml.rs:387-410 on the GPU."""
    s = YamlScene(text, width, height, aa, obj_root)
    r = Renderer(device)
    r.upload(s)
    res = r.render(s.camera, aa=aa)
    write_png(png_file, quantize(res["avg"]))
    return res


def render_scene_from_file(path, width, height, png_file, aa=1, device=0, devices=None):
    """scene_builder_yaml.rs:429-436 on the GPU (same error as the reference for a missing file);
    devices=[...] splits the frame over several GPUs (rr_create_multi)."""
    if devices:
        ids = (C.c_int * len(devices))(*devices)
        check(lib().rr_render_scene_from_file_devices(path.encode(), width, height, png_file.encode(), aa, len(devices),
                                                      ids))
        return
    check(lib().rr_render_scene_from_file(path.encode(), width, height, png_file.encode(), aa, device))
