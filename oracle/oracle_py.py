"""ctypes loaders for the CPU checkers under oracle/.

TEST INFRASTRUCTURE ONLY: importable from tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py. The product package never imports this module.

`Oracle("oracle")` -> oracle/libsrt_oracle.so  (our C restatement, prefix orc_)
`Oracle("ref")`    -> oracle/_ref/libsrt_ref.so (the reference's render.cl compiled for
                      x86-64, prefix ref_; exists only where it was built)
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
COUNTER_NAMES = ["paths", "rays", "sphere_tests", "plane_tests", "aabb_tests", "tri_tests", "tri_pass_u", "bounces", "sky", "nan_pixels"]


def build(ref=False):
    """Compile the checker(s); `ref` additionally needs the reference's source (reference_readable())."""
    targets = ["all"] + (["ref"] if ref else [])
    subprocess.run(["make", "-C", str(HERE)] + targets, check=True, capture_output=True)


def reference_readable():
    """True where this user can read the reference's render.cl at the Makefile's REFERENCE (absent or unreadable: False)."""
    return subprocess.run(["make", "-s", "-C", str(HERE), "have-ref"], capture_output=True).returncode == 0


def ref_available():
    return (HERE / "_ref" / "libsrt_ref.so").exists()


def ref_libm_available():
    return (HERE / "_ref" / "libsrt_ref_libm.so").exists()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rec():
    import sys
    sys.path.insert(0, str(HERE.parent))
    import srt_pkg
    srt_pkg.load()
    from simple_raytracer_amd import records
    return records


def _scene_arrays(shapes, tris, mats, rd, sd):
    R = _rec()
    return (R.as_records(shapes, R.SHAPE), R.as_records(tris, R.TRIANGLE), R.as_records(mats, R.MATERIAL),
            R.as_records(rd, R.RENDER_DATA), R.as_records(sd, R.SCENE_DATA))


class _TexDesc(C.Structure):  # srt_texture_desc
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class _PlaneFrame(C.Structure):  # orc_plane_frame
    _fields_ = [("has_frame", C.c_int32), ("T", C.c_float * 3), ("B", C.c_float * 3)]


class _Textures(C.Structure):  # orc_textures
    _fields_ = [("images", C.POINTER(_TexDesc)), ("num_images", C.c_int32), ("first_hit_only", C.c_int32), ("bindings", C.c_void_p),
                ("tri_uvs", C.c_void_p), ("frames", C.POINTER(_PlaneFrame))]


class TextureTable:
    """The texture table of the orc_*_textured entry points (srt_oracle.c orc_textures), kept alive with its arrays.
    images: list of (H, W, 4) float32, row 0 = bottom; bindings: one records.MATERIAL_TEXTURE per material (index -1: none);
    uvs: (n_triangles, 3, 2) float32 or None; frames: one entry per shape, None or (T, B) -- the caller makes them
    (tests/texture_ref.py plane_frame), this module and the C file never do. first_hit_only: hits after a path's first keep
    the material colour (the tests' coverage probe)."""

    def __init__(self, images, bindings, n_materials, n_shapes, n_triangles, frames, uvs=None, first_hit_only=False):
        R = _rec()
        self.images = [np.ascontiguousarray(im, np.float32) for im in images]
        self.bindings = R.as_records(bindings, R.MATERIAL_TEXTURE).copy()
        assert len(self.bindings) == n_materials and len(frames) == n_shapes
        for b in self.bindings:
            assert -1 <= int(b["texture"]) < len(self.images) and int(b["filter"]) in (0, 1)
        self.descs = (_TexDesc * max(len(self.images), 1))()
        for d, im in zip(self.descs, self.images):
            assert im.ndim == 3 and im.shape[2] == 4 and im.shape[0] >= 1 and im.shape[1] >= 1
            d.rgba, d.width, d.height = im.ctypes.data, im.shape[1], im.shape[0]
        self.frames = (_PlaneFrame * max(n_shapes, 1))()
        for f, tb in zip(self.frames, frames):
            if tb is not None:
                f.has_frame = 1
                f.T[:] = [float(x) for x in np.asarray(tb[0], np.float32)]
                f.B[:] = [float(x) for x in np.asarray(tb[1], np.float32)]
        self.uvs = None
        if uvs is not None:
            self.uvs = np.ascontiguousarray(uvs, np.float32)
            assert self.uvs.shape == (n_triangles, 3, 2)
        self.c = _Textures(self.descs, len(self.images), int(bool(first_hit_only)), self.bindings.ctypes.data,
                           self.uvs.ctypes.data if self.uvs is not None else None, self.frames)

    def ref(self):
        return C.byref(self.c)


def _tex(textures):
    return textures.ref() if textures is not None else None


class Oracle:
    def __init__(self, kind="oracle"):
        self.kind = kind
        if kind == "oracle":
            path, self.px = HERE / "libsrt_oracle.so", "orc_"
            if not path.exists():
                build()
        elif kind == "ref":
            path, self.px = HERE / "_ref" / "libsrt_ref.so", "ref_"
        elif kind == "ref_libm":  # the reference object with glibc behind cos / log / pow / atan2 (statistics only)
            path, self.px = HERE / "_ref" / "libsrt_ref_libm.so", "ref_"
        else:
            raise ValueError(kind)
        self.lib = C.CDLL(str(path))
        f = self._f
        f("render").restype = None
        f("average").restype = None
        f("trace_paths").restype = None
        f("random_float").restype = C.c_float
        f("shlick_reflectance").restype = C.c_float
        f("shlick_reflectance").argtypes = [C.c_float, C.c_float]
        f("intersection_aabb").argtypes = [C.c_void_p] * 4 + [C.c_float]
        for n in ("intersect_sphere", "intersect_plane", "intersect_triangle", "intersection_aabb"):
            f(n).restype = C.c_int

    def _f(self, name):
        return getattr(self.lib, self.px + name)

    # ---- kernels ---------------------------------------------------------------
    def render(self, rd, sd, shapes, tris, mats, sky, canvas=None, rows=None, nthreads=0, counters=False, row_stride=1):
        """`render` kernel over rows [y0,y1) (default all): canvas += colour. Returns the
        canvas (h, w, 4) float32, and the counter dict when counters=True (oracle only)."""
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        w, h = int(rd["width"]), int(rd["height"])
        if canvas is None:
            canvas = np.zeros((h, w, 4), np.float32)
        y0, y1 = (0, h) if rows is None else rows
        sky = np.ascontiguousarray(sky, np.float32)
        args = [_p(rd), _p(sd), _p(canvas), _p(shapes), _p(tris), _p(mats), _p(sky),
                C.c_int(sky.shape[1]), C.c_int(sky.shape[0]), C.c_int(y0), C.c_int(y1)]
        ctr = None
        if self.kind == "oracle":
            ctr = np.zeros(len(COUNTER_NAMES), np.uint64)
            args += [C.c_int(row_stride), C.c_int(nthreads), _p(ctr)]
            self.lib.orc_render_strided.restype = None
            self.lib.orc_render_strided(*args)
        else:
            assert row_stride == 1
            args.append(C.c_int(nthreads))
            self._f("render")(*args)
        if counters:
            return canvas, dict(zip(COUNTER_NAMES, (int(v) for v in ctr))) if ctr is not None else None
        return canvas

    def render_textured(self, rd, sd, shapes, tris, mats, sky, textures, canvas=None, rows=None, nthreads=0, counters=False, row_stride=1):
        """render() with albedo textures (include/srt_abi.h "albedo textures"; oracle only): `textures` is a TextureTable or
        None (none: exactly render()). Same rows / stride / counters."""
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        w, h = int(rd["width"]), int(rd["height"])
        if canvas is None:
            canvas = np.zeros((h, w, 4), np.float32)
        y0, y1 = (0, h) if rows is None else rows
        sky = np.ascontiguousarray(sky, np.float32)
        ctr = np.zeros(len(COUNTER_NAMES), np.uint64)
        self.lib.orc_render_textured.restype = None
        self.lib.orc_render_textured(_p(rd), _p(sd), _p(canvas), _p(shapes), _p(tris), _p(mats), _p(sky), C.c_int(sky.shape[1]),
                                     C.c_int(sky.shape[0]), _tex(textures), C.c_int(y0), C.c_int(y1), C.c_int(row_stride),
                                     C.c_int(nthreads), _p(ctr))
        if counters:
            return canvas, dict(zip(COUNTER_NAMES, (int(v) for v in ctr)))
        return canvas

    def trace_paths_textured(self, rd, sd, shapes, tris, mats, sky, textures, pixel_ids, samples):
        """trace_paths() with albedo textures (oracle only) -> radiance (n, 3) float32, lookups (n, 3) int32: per path the
        texels read at its first hit and at its later hits (a hit reads one when its material has a texture bound, a plane
        has a frame and the path bounces on), and the specular bounces among them whose mix(texel, 1, 1) is not 1.0f."""
        pixel_ids = np.ascontiguousarray(pixel_ids, np.int32)
        samples = np.ascontiguousarray(samples, np.int32)
        out = np.zeros((len(pixel_ids), 3), np.float32)
        looks = np.zeros((len(pixel_ids), 3), np.int32)
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        sky = np.ascontiguousarray(sky, np.float32)
        self.lib.orc_trace_paths_textured.restype = None
        self.lib.orc_trace_paths_textured(_p(rd), _p(sd), _p(shapes), _p(tris), _p(mats), _p(sky), C.c_int(sky.shape[1]),
                                          C.c_int(sky.shape[0]), _tex(textures), _p(pixel_ids), _p(samples),
                                          C.c_int(len(pixel_ids)), _p(out), _p(looks))
        return out, looks

    def features_textured(self, rd, sd, shapes, tris, mats, textures, feature_samples, normal_depth=None, albedo_hits=None, nthreads=0):
        """features() with albedo textures (oracle only): the albedo of a hit is the texel where its material has one."""
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        w, h = int(rd["width"]), int(rd["height"])
        if normal_depth is None:
            normal_depth = np.zeros((h, w, 4), np.float32)
        if albedo_hits is None:
            albedo_hits = np.zeros((h, w, 4), np.float32)
        for a in (normal_depth, albedo_hits):
            assert a.dtype == np.float32 and a.shape == (h, w, 4) and a.flags.c_contiguous
        self.lib.orc_features_textured.restype = None
        self.lib.orc_features_textured(_p(rd), _p(sd), _p(shapes), _p(tris), _p(mats), _tex(textures), C.c_int(feature_samples),
                                       _p(normal_depth), _p(albedo_hits), C.c_int(nthreads))
        return normal_depth, albedo_hits

    def sample_texture(self, image, filt, u, v, scale_u=1.0, scale_v=1.0):
        """The C texture sampler alone (oracle only): image (H, W, 4) float32, u, v (n,) before the scale -> (n, 3)."""
        image = np.ascontiguousarray(image, np.float32)
        u, v = np.ascontiguousarray(u, np.float32).reshape(-1), np.ascontiguousarray(v, np.float32).reshape(-1)
        out = np.zeros((len(u), 3), np.float32)
        self.lib.orc_sample_texture.restype = None
        self.lib.orc_sample_texture(_p(image), C.c_int(image.shape[1]), C.c_int(image.shape[0]), C.c_int(filt), C.c_float(scale_u),
                                    C.c_float(scale_v), _p(u), _p(v), C.c_size_t(len(u)), _p(out))
        return out

    def average(self, num_steps, canvas):
        canvas = np.ascontiguousarray(canvas, np.float32)
        n = canvas.size // 4
        out = np.zeros(n * 4, np.uint8)
        self._f("average")(C.c_uint32(num_steps), _p(canvas), _p(out), C.c_size_t(n))
        return out.reshape(canvas.shape[:-1] + (4,))

    def trace_paths(self, rd, sd, shapes, tris, mats, sky, pixel_ids, samples):
        pixel_ids = np.ascontiguousarray(pixel_ids, np.int32)
        samples = np.ascontiguousarray(samples, np.int32)
        out = np.zeros((len(pixel_ids), 3), np.float32)
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        sky = np.ascontiguousarray(sky, np.float32)
        self._f("trace_paths")(_p(rd), _p(sd), _p(shapes), _p(tris), _p(mats), _p(sky), C.c_int(sky.shape[1]),
                               C.c_int(sky.shape[0]), _p(pixel_ids), _p(samples), C.c_int(len(pixel_ids)), _p(out))
        return out

    def primary_hits(self, rd, sd, shapes, tris, mats, pixel_ids, samples):
        """The camera rays of (pixel, sample) pairs and their closest hits (oracle only) -> dict of numpy arrays:
        dir (n, 3) unit direction, t (n,) tmin (inf: nothing hit), normal (n, 3) front-facing (0 without a shaded hit),
        material (n,) int (-1: sky, or a shape without a material). The origin is camera_to_world[3]."""
        pixel_ids = np.ascontiguousarray(pixel_ids, np.int32)
        samples = np.ascontiguousarray(samples, np.int32)
        out = np.zeros((len(pixel_ids), 8), np.float32)
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        self.lib.orc_primary_hits.restype = None
        self.lib.orc_primary_hits(_p(rd), _p(sd), _p(shapes), _p(tris), _p(mats), _p(pixel_ids), _p(samples),
                                  C.c_int(len(pixel_ids)), _p(out))
        return {"dir": out[:, :3], "t": out[:, 3], "normal": out[:, 4:7], "material": out[:, 7].astype(np.int64)}

    def features(self, rd, sd, shapes, tris, mats, feature_samples, normal_depth=None, albedo_hits=None, nthreads=0):
        """One dispatch of the denoiser's feature pass (oracle only): adds its sums into normal_depth and albedo_hits
        ((h, w, 4) float32, zeros when None) in place and returns both."""
        shapes, tris, mats, rd, sd = _scene_arrays(shapes, tris, mats, rd, sd)
        w, h = int(rd["width"]), int(rd["height"])
        if normal_depth is None:
            normal_depth = np.zeros((h, w, 4), np.float32)
        if albedo_hits is None:
            albedo_hits = np.zeros((h, w, 4), np.float32)
        for a in (normal_depth, albedo_hits):
            assert a.dtype == np.float32 and a.shape == (h, w, 4) and a.flags.c_contiguous
        self.lib.orc_features.restype = None
        self.lib.orc_features(_p(rd), _p(sd), _p(shapes), _p(tris), _p(mats), C.c_int(feature_samples), _p(normal_depth),
                              _p(albedo_hits), C.c_int(nthreads))
        return normal_depth, albedo_hits

    # ---- function-level known-answer entry points ------------------------------
    def random_floats(self, seed, n):
        s = C.c_uint32(seed)
        out = np.zeros(n, np.float32)
        for i in range(n):
            out[i] = self._f("random_float")(C.byref(s))
        return out, s.value

    def random_direction(self, seed):
        """random_direction (oracle only) -> (the unit vector (3,) float32, the seed advanced by its six draws)"""
        s = C.c_uint32(seed)
        out = np.zeros(3, np.float32)
        self.lib.orc_random_direction.restype = None
        self.lib.orc_random_direction(C.byref(s), _p(out))
        return out, s.value

    def normalize3(self, v):
        """vnormalize (oracle only): (3,) -> (3,) float32, or (n, 3) -> (n, 3) row by row"""
        a = np.ascontiguousarray(v, np.float32)
        out = np.zeros_like(a)
        self.lib.orc_normalize3.restype = None
        fn, pa, po = self.lib.orc_normalize3, a.ctypes.data, out.ctypes.data
        for k in range(a.size // 3):
            fn(C.c_void_p(pa + 12 * k), C.c_void_p(po + 12 * k))
        return out

    def closest_hits(self, shapes, tris, mats, rays):
        """closest_intersection over caller rays (records.RAY, directions used as given; oracle only) -> dict: t (n,) (inf:
        nothing hit), normal (n, 3) turned to face the ray, shape and triangle (n,) int32 (-1: none). A shape without a
        material is a hit."""
        R = _rec()
        rays = np.ascontiguousarray(R.as_records(rays, R.RAY))
        shapes, tris, mats = R.as_records(shapes, R.SHAPE), R.as_records(tris, R.TRIANGLE), R.as_records(mats, R.MATERIAL)
        sd = R.as_records(R.scene_data(len(shapes)), R.SCENE_DATA)
        out = np.zeros((len(rays), 8), np.float32)
        self.lib.orc_closest_hits.restype = None
        with np.errstate(all="ignore"):
            self.lib.orc_closest_hits(_p(sd), _p(shapes), _p(tris), _p(mats), _p(rays), C.c_int(len(rays)), _p(out))
        ids = out[:, 4:6].view(np.int32)
        return {"t": out[:, 0].copy(), "normal": out[:, 1:4].copy(), "shape": ids[:, 0].copy(), "triangle": ids[:, 1].copy()}

    def any_hit(self, shapes, tris, rays):
        """The occlusion contract over caller rays with unit directions (oracle only) -> (n,) bool: some primitive's
        intersector accepts the ray with t < tmax; validity is the caller's business."""
        R = _rec()
        rays = np.ascontiguousarray(R.as_records(rays, R.RAY))
        shapes, tris = R.as_records(shapes, R.SHAPE), R.as_records(tris, R.TRIANGLE)
        sd = R.as_records(R.scene_data(len(shapes)), R.SCENE_DATA)
        out = np.zeros(len(rays), np.uint8)
        self.lib.orc_any_hit.restype = None
        self.lib.orc_any_hit(_p(sd), _p(shapes), _p(tris), _p(rays), C.c_int(len(rays)), _p(out))
        return out.astype(bool)

    def shlick(self, mu, c):
        return np.float32(self._f("shlick_reflectance")(C.c_float(mu), C.c_float(c)))

    def intersect_sphere(self, center, radius, o, d):
        from_records = np.zeros(8, np.float32)
        from_records[:3] = center
        from_records[4] = radius
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        t = C.c_float(np.nan)
        hit = self._f("intersect_sphere")(_p(from_records), _p(o), _p(d), C.byref(t))
        return hit, np.float32(t.value)

    def intersect_plane(self, pos, normal, o, d):
        rec = np.zeros(8, np.float32)
        rec[:3] = pos
        rec[4:7] = normal
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        t = C.c_float(np.nan)
        hit = self._f("intersect_plane")(_p(rec), _p(o), _p(d), C.byref(t))
        return hit, np.float32(t.value)

    def intersect_triangle(self, p0, p1, p2, o, d):
        a = [np.ascontiguousarray(v, np.float32) for v in (p0, p1, p2, o, d)]
        t = C.c_float(np.nan)
        hit = self._f("intersect_triangle")(*[_p(v) for v in a], C.byref(t))
        return hit, np.float32(t.value)

    def intersection_aabb(self, bmin, bmax, o, inv_dir, tmax):
        a = [np.ascontiguousarray(v, np.float32) for v in (bmin, bmax, o, inv_dir)]
        return self._f("intersection_aabb")(*[_p(v) for v in a], C.c_float(tmax))

    def matrix_by_vector(self, m, v):
        m = np.ascontiguousarray(m, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        out = np.zeros(4, np.float32)
        self._f("matrix_by_vector")(_p(m), _p(v), _p(out))
        return out

    def barycentric_weights(self, p0, p1, p2, p):
        a = [np.ascontiguousarray(v, np.float32) for v in (p0, p1, p2, p)]
        out = np.zeros(3, np.float32)
        self._f("barycentric_weights")(*[_p(v) for v in a], _p(out))
        return out

    def sky_box(self, sd, sky, direction):
        sky = np.ascontiguousarray(sky, np.float32)
        sd = _rec().as_records(sd, _rec().SCENE_DATA)
        d = np.ascontiguousarray(direction, np.float32)
        out = np.zeros(3, np.float32)
        self._f("sky_box")(_p(sd), _p(sky), C.c_int(sky.shape[1]), C.c_int(sky.shape[0]), _p(d), _p(out))
        return out

    def math_checksums(self, stride):
        out = (C.c_uint64 * 8)()
        self.lib.orc_math_checksums.restype = None
        self.lib.orc_math_checksums(C.c_uint32(stride), out)
        return [int(v) for v in out]

    def aces(self, rgb):
        a = np.ascontiguousarray(rgb, np.float32)
        out = np.zeros(3, np.float32)
        self._f("aces")(_p(a), _p(out))
        return out
