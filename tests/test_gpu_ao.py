"""The ambient-occlusion pass on the device (include/srt_abi.h "ambient-occlusion pass"; csrc/ao.hip): the rays word for word and
the counts integer for integer against the CPU reference (tests/ao_ref.py, section 11) -- the pinned reference --, the counts
against the occlusion query over the pass's own rays, the rays' properties, their distribution, scenes with known answers, the
view's bytes, what the pass leaves untouched, its order behind scene updates, its errors, and the group and headless routes."""
import ctypes as C

import numpy as np
import pytest

import ao_cases as A
import ao_ref as AR
import gpu_harness as G
from gpu_harness import T  # noqa: F401 (the fixture)
from simple_raytracer_amd import records as R, scenes as S

pytestmark = pytest.mark.gpu
F = np.float32
OK, INVALID, STATE = 0, 1, 3
DEVICE, MEDIAN = 1, 1  # SRT_BUILD_DEVICE, SRT_BUILD_ORDER_MEDIAN; also SRT_REFIT_DEVICE
NONE = A.HIT_NONE


def handle(T, scn, accel="scan", w=24, h=16, refit=False):
    sh, tr, ma = A.scene(scn) if isinstance(scn, str) else scn
    t = T.Tracer(w, h)
    t.set_acceleration(0 if accel == "scan" else 1)
    if accel == "median":
        t.set_acceleration_build(DEVICE, 0)
        t.set_acceleration_build_order(MEDIAN)
    if refit:
        t.set_acceleration_refit(DEVICE)
    t.options = R.render_data(w, h, 1, 1, camera_to_world=S.default_camera())
    t.scene_data = R.scene_data(len(sh))
    t.update_scene(sh, tr, ma)
    return t


def reference_counts(t, rd, **kw):
    """the pinned reference: per pixel, the popcount of srt_occluded_rays over the pass's own rays; NONE without a surface"""
    w, h = int(rd["width"]), int(rd["height"])
    rays = t.ao_rays(rd, **kw)
    s = len(rays) // (w * h)
    occ = t.occluded_rays(rays, unit=True).reshape(w * h, s).sum(axis=1).astype(np.uint32)
    occ[np.isnan(rays["tmax"].reshape(w * h, s)[:, 0])] = NONE
    return occ.reshape(h, w), rays


_planes = {}  # (scene, w, h, S) -> the first acceleration mode's plane: equal across modes


# ---- 1. counts equal the occlusion query -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", A.CASES)
def test_counts_equal_the_occlusion_query(name, accel, T):
    partial = 0
    for w, h in A.FRAMES:
        rd = A.rd(name, w, h)
        t = handle(T, name, accel, w, h)
        t.render_ids(rd)
        no_surface = t.read_id_pass()["shape"] == NONE
        # the frame shows what the test needs, by the ID pass (the pick) alone
        assert 2 * (~no_surface).sum() >= w * h and no_surface.any(), (name, w, h)
        for s in A.SAMPLES:
            t.render_ao(rd, samples=s, seed=s)
            got, samples = t.read_ao()
            want, _ = reference_counts(t, rd, samples=s, seed=s)
            assert samples == s and got.shape == (h, w) and got.dtype == np.uint32
            assert np.array_equal(got, want), (name, accel, w, h, s)
            assert np.array_equal(got == NONE, no_surface), (name, accel, w, h, s)
            assert (got[~no_surface] <= s).all()
            assert np.array_equal(got, _planes.setdefault((name, w, h, s), got)), (name, accel, w, h, s)
            partial += int(((want > 0) & (want < s)).sum()) if s > 1 else 0
        assert t.counters()["watchdog"] == 0
        t.close()
    assert partial > 0  # some pixel is neither open nor closed: by the reference, not by the pass


# ---- 2. the rays are the defined rays ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "scan"), ("mesh_smooth", "sah")])
@pytest.mark.parametrize("w,h", A.FRAMES)
def test_the_rays_are_the_defined_rays(name, accel, w, h, T):
    rd, s, bias = A.rd(name, w, h), 4, 0.01
    radius = F(2.5)
    t = handle(T, name, accel, w, h)
    rays = t.ao_rays(rd, samples=s, radius=radius, bias=bias, seed=7)
    assert len(rays) == w * h * s and not rays["reserved"].any()
    hits = t.pick(A.centres(w, h), rd)
    surf = (hits["flags"] & R.HIT_HIT) != 0
    assert 2 * surf.sum() >= w * h and not surf.all()
    per_ray = np.repeat(surf, s)
    # tmax: the radius' bits, NaN exactly on the pixels without a surface (whose records are otherwise 0)
    assert np.array_equal(np.isnan(rays["tmax"]), ~per_ray)
    assert (rays["tmax"][per_ray].view(np.uint32) == radius.view(np.uint32)).all()
    assert not rays["origin"][~per_ray].any() and not rays["direction"][~per_ray].any()
    # unit directions in the normal's hemisphere
    d, n = rays["direction"][per_ray].astype(np.float64), np.repeat(hits["normal"], s, axis=0)[per_ray].astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    print(f"| |D| - 1 |: worst {np.abs(length - 1).max() / A.U:.2f} x 2^-24")
    assert (np.abs(length - 1.0) <= 4 * A.U).all()
    assert ((d * n).sum(axis=1) > 0.0).all()
    # the origin against cam + dir64 t + N bias in float64, within the bound derived in ao_cases.py
    cam = np.asarray(rd["camera_to_world"], np.float64).reshape(4, 4)[3, :3]
    tt = np.repeat(hits["t"], s)[per_ray].astype(np.float64)
    want = cam + np.repeat(A.centre_dirs64(rd), s, axis=0)[per_ray] * tt[:, None] + n * float(F(bias))
    err, bound = np.abs(rays["origin"][per_ray] - want), A.origin_bound(rd, tt, bias)[:, None]
    print(f"origin: worst error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    # a pixel's S rays share the origin
    o = rays["origin"].view(np.uint32).reshape(w * h, s, 3)
    assert (o == o[:, :1]).all()
    # windows, repeats, another seed
    bits = rays.view(np.uint32).reshape(-1, 8)
    win = t.ao_rays(rd, first=5, n=7, samples=s, radius=radius, bias=bias, seed=7).view(np.uint32).reshape(-1, 8)
    assert np.array_equal(win, bits[5 * s:12 * s])
    last = t.ao_rays(rd, first=w * h - 1, n=1, samples=s, radius=radius, bias=bias, seed=7).view(np.uint32).reshape(-1, 8)
    assert np.array_equal(last, bits[-s:]) and len(t.ao_rays(rd, first=w * h, n=0, samples=s)) == 0
    assert np.array_equal(t.ao_rays(rd, samples=s, radius=radius, bias=bias, seed=7).view(np.uint32).reshape(-1, 8), bits)
    other = t.ao_rays(rd, samples=s, radius=radius, bias=bias, seed=8)
    assert np.array_equal(other["origin"].view(np.uint32), rays["origin"].view(np.uint32))
    assert np.array_equal(other["tmax"].view(np.uint32), rays["tmax"].view(np.uint32))
    assert (other["direction"][per_ray] != rays["direction"][per_ray]).any(axis=1).all()
    t.close()


# ---- 3. distribution ---------------------------------------------------------------------------------------------------------
def hemisphere_sample(T, seed):
    """cos = dot(D, N) and the two tangential components of >= 4,096 rays of surface pixels, in float64"""
    w, h, s = 24, 16, 16
    rd = A.rd("spheres", w, h)
    t = handle(T, "spheres", "scan", w, h)
    rays = t.ao_rays(rd, samples=s, seed=seed)
    hits = t.pick(A.centres(w, h), rd)
    t.close()
    per_ray = np.repeat((hits["flags"] & R.HIT_HIT) != 0, s)
    d, n = rays["direction"][per_ray].astype(np.float64), np.repeat(hits["normal"], s, axis=0)[per_ray].astype(np.float64)
    t1, t2 = A.tangents(n)
    assert len(d) >= 4096
    return (d * n).sum(axis=1), (d * t1).sum(axis=1), (d * t2).sum(axis=1)


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
def test_the_mean_cosine_is_two_thirds(seed, T):
    """The cosine law: E[c] = 2/3, E[c^2] = 1/2, so the mean of c = dot(D, N) over n rays lies within 5 sqrt(1/18) / sqrt(n) of
    2/3. A uniform hemisphere (E[c] = 1/2), the trace's bounce with its hemisphere flip (0.862) or a sign error fails."""
    c, _, _ = hemisphere_sample(T, seed)
    print(f"seed {seed:#x}: n {len(c)}, mean cosine {c.mean():.6f}, tolerance {5 * np.sqrt(1 / 18) / np.sqrt(len(c)):.6f}")
    assert abs(c.mean() - 2.0 / 3.0) <= 5.0 * np.sqrt(1.0 / 18.0) / np.sqrt(len(c))


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
def test_the_tangential_means_are_zero(seed, T):
    """Each tangential component's mean within 5 sigma of 0, sigma = sqrt(1/4) / sqrt(n): a hemisphere sign error or a seed
    rule that correlates a pixel's rays fails here."""
    _, a, b = hemisphere_sample(T, seed)
    sigma = np.sqrt(0.25) / np.sqrt(len(a))
    print(f"seed {seed:#x}: tangential means {a.mean():+.5f} {b.mean():+.5f}, 5 sigma {5 * sigma:.5f}")
    assert abs(a.mean()) <= 5 * sigma and abs(b.mean()) <= 5 * sigma


@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
def test_the_squared_cosine_is_uniform(seed, T):
    """D = normalize(N + rd), rd uniform on the sphere: with a = dot(N, rd) uniform on [-1, 1], |N + rd|^2 = 2 + 2 a and
    c^2 = (1 + a) / 2 is uniform on [0, 1], which is the cosine law. So E[c^2] = 1/2 with Var[c^2] = 1/12, and a quarter of the
    rays lies in each quarter of [0, 1], a count of variance 3 n / 16; each within 5 sigma over n rays."""
    c, _, _ = hemisphere_sample(T, seed)
    n, c2 = len(c), np.clip(c * c, 0.0, 1.0)  # (|D| is 1 to four ulps)
    assert abs(c2.mean() - 0.5) <= 5 * np.sqrt(1.0 / 12.0) / np.sqrt(n)
    counts = np.histogram(c2, bins=4, range=(0.0, 1.0))[0]
    print(f"seed {seed:#x}: mean c^2 {c2.mean():.5f}, quarters {counts.tolist()} of {n}")
    assert (np.abs(counts - n / 4.0) <= 5 * np.sqrt(3.0 * n / 16.0)).all()


# ---- 4. analytic scenes ------------------------------------------------------------------------------------------------------
def arrays(shapes):
    """shapes, no triangles, one material"""
    return R.concat(R.SHAPE, *[np.atleast_1d(s) for s in shapes]), np.zeros(0, R.TRIANGLE), np.atleast_1d(R.material(color=(0.8, 0.8, 0.8)))


def analytic(T, shapes, cam, w=24, h=16, **kw):
    t = handle(T, arrays(shapes), "scan", w, h)
    rd = R.render_data(w, h, 1, 1, camera_to_world=cam)
    t.render_ao(rd, **kw)
    occ, _ = t.read_ao()
    t.close()
    return occ


def test_one_plane_is_open_everywhere(T):
    occ = analytic(T, [R.plane(0, (0, 0, 0), (0, 1, 0))], R.camera_matrix((0.0, 1.0, 5.0), 0.0, 0.0), samples=16)
    surf = occ != NONE
    assert surf.any() and (~surf).any() and not occ[surf].any()


def test_inside_a_sphere_everything_is_closed_unless_the_radius_is_short(T):
    cam = R.camera_matrix((0.0, 0.0, 0.0), 0.0, 0.0)
    for s in (1, 16, 64):
        occ = analytic(T, [R.sphere(0, (0, 0, 0), 10.0)], cam, samples=s)
        assert (occ == s).all(), s
    # no ray points away from the normal, which points at the centre: from an origin 0.01 inside the surface the nearest the
    # sphere can be met is along the tangent, sqrt(10^2 - 9.99^2) = 0.447
    occ = analytic(T, [R.sphere(0, (0, 0, 0), 10.0)], cam, samples=16, radius=0.25, bias=0.01)
    assert not occ.any()


def test_the_floor_darkens_towards_a_resting_sphere(T):
    w, h = 24, 16
    cam = R.camera_matrix((0.0, 3.0, 6.0), 0.0, -0.45)
    shapes = [R.plane(0, (0, 0, 0), (0, 1, 0)), R.sphere(0, (0, 1, 0), 1.0)]
    occ = analytic(T, shapes, cam, w, h, samples=64)
    t = handle(T, arrays(shapes), "scan", w, h)
    rd = R.render_data(w, h, 1, 1, camera_to_world=cam)
    hits = t.pick(A.centres(w, h), rd)
    t.close()
    floor = ((hits["flags"] & R.HIT_HIT) != 0) & (hits["shape"] == 0)
    assert floor.sum() >= 32
    dirs = A.centre_dirs64(rd)
    pos = cam[3, :3].astype(np.float64) + dirs * hits["t"].astype(np.float64)[:, None]
    dist = np.where(floor, np.hypot(pos[:, 0], pos[:, 2]), np.nan)
    near, far = int(np.nanargmin(dist)), int(np.nanargmax(dist))
    flat = occ.reshape(-1)
    print(f"nearest floor pixel {near}: {flat[near]} of 64 at {dist[near]:.2f}; farthest {far}: {flat[far]} at {dist[far]:.2f}")
    assert flat[near] > flat[far]


# ---- 5. the view -------------------------------------------------------------------------------------------------------------
def test_the_view_is_the_table_and_the_background(T):
    w, h = 13, 7
    rd = A.rd("mesh_smooth", w, h)
    t = handle(T, "mesh_smooth", "sah", w, h)
    for s, bg in ((1, 0xFF000000), (8, 0x80102030), (64, 0x00FFFFFF)):
        t.render_ao(rd, samples=s, background=bg)
        occ, _ = t.read_ao()
        t.resolve_ao_view()
        got = t.read_argb().reshape(h, w, 4)
        assert np.array_equal(got, A.view_bytes(occ, s, bg)), s
        assert np.array_equal(A.table(s), T.ao_table(samples=s))
    assert (occ == NONE).any() and len(np.unique(got[..., 1])) > 2
    # a pass at another size is no picture of this handle's
    t.render_ao(A.rd("mesh_smooth", 24, 16), samples=4)
    assert t.lib.srt_resolve_ao_view(t._h) == STATE
    assert t.read_ao()[0].shape == (16, 24)
    t.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------
def test_the_pass_leaves_the_frame_alone(T, sky):
    w, h = 24, 16
    cam, fov = A.VIEWS["mesh_smooth"]
    t = G.make(T, sky, A.scene("mesh_smooth"), w, h, spp=2, accel=1, cam=cam, denoise=dict(feature_samples=1))
    t.set_kernel_timers(True)
    t.set_exposure(mode="auto")
    t.set_selection([1])
    t.render(1)
    t.render_ids()

    def state():
        dn, ids, ex = t.read_denoise_inputs(), t.read_id_pass(), t.read_exposure()
        planes = [t.read_canvas().view(np.uint32).copy()] + [dn[k].view(np.uint32).copy() for k in ("normal_depth", "albedo_hits", "moments")]
        planes += [ids[k].copy() for k in ("shape", "triangle", "material")] + [ex["hist"].copy(), t.read_selection_alpha()]
        return (planes, (dn["T"], dn["P"], np.float32(ex["log2_exposure"]).tobytes(), np.float32(ex["exposure"]).tobytes(), ex["metered"], ex["left_out"],
                         t.counters(), t.debug_counters(), t.last_trace_launches(), t.last_trace_kernel_ms(), t.last_kernel_ms(), t.last_trace_class(),
                         t.last_trace_plane_form(), t.last_trace_textured(), t.last_resolve_selected(), t.last_resolve_exposed(), t.last_resolve_bloomed(),
                         t.last_meter_ran()))

    before = state()
    argb = t.read_argb().copy()
    t.render_ao(samples=8)
    assert t.last_ray_query_ms() > 0.0
    occ, _ = t.read_ao()
    t.ao_rays(first=3, n=5, samples=8)
    assert t.last_ray_query_ms() > 0.0
    after = state()
    assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1] == after[1]
    assert np.array_equal(argb, t.read_argb())  # the bytes change only with resolve_ao_view
    assert ((occ != NONE) & (occ > 0)).any()
    t.resolve_ao_view()
    assert np.array_equal(t.read_argb().reshape(h, w, 4), A.view_bytes(occ, 8)) and state()[1] == before[1]
    t.render(2)  # and the next frame runs as if nothing had been asked
    t.synchronize()
    t.close()


# ---- 7. order ----------------------------------------------------------------------------------------------------------------
def test_the_pass_sees_the_updated_scene(T):
    sh, tr, ma = A.scene("spheres")
    w, h = 24, 16
    rd = A.rd("spheres", w, h)
    t = handle(T, "spheres", "scan", w, h)
    t.render_ao(rd, samples=8)
    first, _ = t.read_ao()
    moved = sh.copy()
    moved["sphere_position"][3:] += np.asarray((0.0, 40.0, 0.0), F)  # the spheres out of sight
    t.update_scene(moved, tr, ma)
    t.render_ao(rd, samples=8)
    second, _ = t.read_ao()
    assert np.array_equal(second, reference_counts(t, rd, samples=8)[0]) and not np.array_equal(first, second)
    t.close()


def test_the_pass_sees_the_device_refit(T):
    sh, tr, ma = A.scene("mesh_smooth")
    w, h = 13, 7
    rd = A.rd("mesh_smooth", w, h)
    t = handle(T, "mesh_smooth", "sah", w, h, refit=True)
    t.render_ao(rd, samples=8)
    first, _ = t.read_ao()
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    t.render_ao(rd, samples=8)
    second, _ = t.read_ao()
    scan = handle(T, (moved, tr, ma), "scan", w, h)  # the moved scene built from nothing, without a hierarchy
    scan.render_ao(rd, samples=8)
    assert np.array_equal(second, scan.read_ao()[0]) and not np.array_equal(first, second)
    assert np.array_equal(second, reference_counts(t, rd, samples=8)[0])
    scan.close(), t.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def test_errors(T):
    w, h = 13, 7
    t = T.Tracer(w, h)
    lib, rd = t.lib, A.rd("spheres", w, h)
    p, ptr = T._ao_params({}, "test"), lambda a: a.ctypes.data_as(C.c_void_p)
    wi, hi, si = C.c_int(0), C.c_int(0), C.c_int(0)
    # before any pass
    assert lib.srt_read_ao(t._h, None, 0, C.byref(wi), C.byref(hi), C.byref(si)) == STATE and lib.srt_resolve_ao_view(t._h) == STATE
    with pytest.raises(T.SrtError):
        t.read_ao()
    # NULL arguments
    rays = np.zeros(w * h * 16, R.RAY)
    assert lib.srt_render_ao(None, ptr(rd), ptr(p)) == INVALID and lib.srt_render_ao(t._h, None, ptr(p)) == INVALID
    assert lib.srt_render_ao(t._h, ptr(rd), None) == INVALID
    assert lib.srt_ao_rays(t._h, None, ptr(p), 0, 1, ptr(rays)) == INVALID and lib.srt_ao_rays(t._h, ptr(rd), None, 0, 1, ptr(rays)) == INVALID
    assert lib.srt_ao_rays(t._h, ptr(rd), ptr(p), 0, 1, None) == INVALID and lib.srt_ao_rays(None, ptr(rd), ptr(p), 0, 1, ptr(rays)) == INVALID
    assert lib.srt_read_ao(None, None, 0, None, None, None) == INVALID and lib.srt_resolve_ao_view(None) == INVALID
    # every refusal of srt_ao_check_host, through the pass and through the rays
    for kw in (dict(samples=0), dict(samples=3), dict(samples=128), dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(bias=-1e-6),
               dict(bias=np.inf), dict(bias=np.nan), dict(reserved=(0, 0, 1))):
        bad = T._ao_params(kw, "test")
        assert lib.srt_render_ao(t._h, ptr(rd), ptr(bad)) == INVALID, kw
        assert lib.srt_ao_rays(t._h, ptr(rd), ptr(bad), 0, 1, ptr(rays)) == INVALID, kw
    for width, height in ((0, h), (w, 0), (-3, h), (1 << 16, 1 << 11)):  # 2^27 pixels x 16 samples = 2^31
        big = rd.copy()
        big["width"], big["height"] = width, height
        assert lib.srt_render_ao(t._h, ptr(big), ptr(p)) == INVALID, (width, height)
    assert lib.srt_read_ao(t._h, None, 0, None, None, None) == STATE  # nothing above made a pass
    # windows beyond the frame
    n = w * h
    for first, count in ((n, 1), (n - 1, 2), (0, n + 1), (n + 1, 0), (2 ** 63, 2 ** 63)):
        assert lib.srt_ao_rays(t._h, ptr(rd), ptr(p), first, count, ptr(rays)) == INVALID, (first, count)
    assert lib.srt_ao_rays(t._h, ptr(rd), ptr(p), n, 0, None) == OK and lib.srt_ao_rays(t._h, ptr(rd), ptr(p), 0, n, ptr(rays)) == OK
    # before any scene is set every pixel is without a surface
    assert np.isnan(rays["tmax"]).all()
    t.render_ao(rd)
    occ, s = t.read_ao()
    assert s == 16 and (occ == NONE).all()
    # the sizes alone, and a capacity too small
    assert lib.srt_read_ao(t._h, None, 0, C.byref(wi), C.byref(hi), C.byref(si)) == OK and (wi.value, hi.value, si.value) == (w, h, 16)
    small = np.zeros(n - 1, np.uint32)
    assert lib.srt_read_ao(t._h, ptr(small), n - 1, None, None, None) == INVALID and lib.srt_read_ao(t._h, ptr(occ), n, None, None, None) == OK
    t.resolve_ao_view()
    assert np.array_equal(t.read_argb().reshape(h, w, 4), A.view_bytes(occ, 16))
    t.close()


# ---- 9. group ----------------------------------------------------------------------------------------------------------------
def test_group_forms_give_the_single_handles_words(T):
    sh, tr, ma = A.scene("mesh_smooth")
    w, h = 24, 16
    rd = A.rd("mesh_smooth", w, h)
    t = handle(T, "mesh_smooth", "sah", w, h)
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=1)
    with pytest.raises(T.SrtError):
        g.read_ao()
    g.set_acceleration(1)
    g.scene_data = R.scene_data(len(sh))
    g.update_scene(sh, tr, ma)
    kw = dict(samples=8, seed=3, radius=4.0, background=0x11223344)
    g.render_ao(rd, **kw), t.render_ao(rd, **kw)
    a, b = g.read_ao(), t.read_ao()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 8 and (b[0] == NONE).any() and ((b[0] != NONE) & (b[0] > 0)).any()
    assert np.array_equal(g.ao_rays(rd, first=2, n=40, **kw).view(np.uint32), t.ao_rays(rd, first=2, n=40, **kw).view(np.uint32))
    g.resolve_ao_view(), t.resolve_ao_view()
    view = g.read_ao_view()
    assert np.array_equal(view, t.read_argb().reshape(h, w, 4)) and np.array_equal(view, A.view_bytes(b[0], 8, 0x11223344))
    g.close(), t.close()


# ---- 10. the headless route --------------------------------------------------------------------------------------------------
def test_headless_prints_what_python_computes(T, tmp_path):
    import subprocess
    from simple_raytracer_amd import build
    exe = str(build.build_headless())
    w, h = 24, 16
    prefix, ppm = str(tmp_path / "s"), tmp_path / "ao.ppm"
    cmd = [exe, "--scene", "spheres", "--width", str(w), "--height", str(h), "--spp", "1", "--bounces", "1", "--frames", "1", "--dump", prefix,
           "--ao", "16", "--ao-view", str(ppm)]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("ao: ")]
    assert len(lines) == 1 and "frame(s)" in out, out
    dumped = (np.fromfile(prefix + ".shapes.bin", R.SHAPE), np.fromfile(prefix + ".tris.bin", R.TRIANGLE), np.fromfile(prefix + ".mats.bin", R.MATERIAL))
    rd = np.fromfile(prefix + ".rd.bin", R.RENDER_DATA)[0]
    t = handle(T, dumped, "scan", w, h)
    t.render_ao(rd, samples=16)
    occ, _ = t.read_ao()
    surf = occ != NONE
    mean = float((occ[surf].astype(np.float64) / 16.0).sum() / surf.sum())
    assert lines[0] == f"ao: pixels {w * h} surfaces {int(surf.sum())} mean {mean:.6f}"
    raw = ppm.read_bytes()
    header = f"P6 {w} {h} 255\n".encode()
    assert raw.startswith(header)
    t.resolve_ao_view()
    assert np.array_equal(np.frombuffer(raw[len(header):], np.uint8).reshape(h, w, 3), t.read_argb().reshape(h, w, 4)[..., 1:])
    t.close()


# ---- 11. the CPU reference (tests/ao_ref.py): rays word for word, counts integer for integer --------------------------------------
# Everything below is an equality of uint32 words or of integers with what tests/ao_ref.py states on the CPU oracle from the
# pick's rays; nothing of the expected side comes from the library's AO or occlusion entry points.
_ref_surfaces, _ref_words = {}, {}  # computed once per key and never changed; shared by the acceleration modes


def ref_surfaces(t, oracle, name, rd, scn=None):
    w, h = int(rd["width"]), int(rd["height"])
    key = (name, w, h)
    if key not in _ref_surfaces:
        _ref_surfaces[key] = AR.surfaces(oracle, A.ref_scene(name) if scn is None else scn, t.pick_rays(A.centres(w, h), rd))
    return _ref_surfaces[key]


def ref_words(t, oracle, name, rd, s, seed=0, radius=np.inf, bias=0.001, scn=None):
    key = (name, int(rd["width"]), int(rd["height"]), s, seed, float(radius), float(bias))
    if key not in _ref_words:
        _ref_words[key] = AR.records(oracle, ref_surfaces(t, oracle, name, rd, scn), s, seed=seed, radius=radius, bias=bias)
    return _ref_words[key]


def assert_words(got, want, what):
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (what, f"{len(bad)} of {len(got)} records differ; the first, record {bad[0]}:", [hex(x) for x in got[bad[0]]], [hex(x) for x in want[bad[0]]])


@pytest.mark.parametrize("name,accel", A.REF_CASES)
def test_the_rays_equal_the_reference_word_for_word(name, accel, T, oracle):
    scn = A.ref_scene(name)
    for fi, (w, h) in enumerate(A.REF_FRAMES):
        rd = A.ref_rd(name, w, h)
        t = handle(T, scn, accel, w, h)
        surf = ref_surfaces(t, oracle, name, rd)
        assert 2 * surf["has"].sum() >= w * h and (name in A.ENCLOSED or not surf["has"].all())
        for shape in A.REF_VIEWS[name][2]:
            assert (surf["shape"] == shape).any(), (name, shape)
        for si, s in enumerate(A.REF_SAMPLES):
            seed, radius, bias = A.ray_parameters(4 * fi + si)
            got = t.ao_rays(rd, samples=s, seed=seed, radius=radius, bias=bias)
            assert_words(got, ref_words(t, oracle, name, rd, s, seed, radius, bias), (name, accel, w, h, s, hex(seed), radius, bias))
        assert t.counters()["watchdog"] == 0
        t.close()


def test_every_seed_radius_and_bias_of_the_ray_cases(T, oracle):
    name, w, h, s = "spheres", 13, 7, 4
    rd = A.ref_rd(name, w, h)
    t = handle(T, A.ref_scene(name), "scan", w, h)
    for seed in A.SEEDS:
        for radius in A.RADII:
            for bias in A.BIASES:
                got = t.ao_rays(rd, samples=s, seed=seed, radius=radius, bias=bias)
                assert_words(got, ref_words(t, oracle, name, rd, s, seed, radius, bias), (hex(seed), radius, bias))
    t.close()


@pytest.mark.parametrize("name,accel", [("spheres", "scan"), ("mesh_smooth", "sah")])
def test_small_frames_and_windows_equal_the_reference(name, accel, T, oracle):
    scn = A.ref_scene(name)
    seen = set()
    for w, h in A.SMALL_FRAMES:  # one pixel, and fewer rays than a wave
        rd = A.ref_rd(name, w, h)
        t = handle(T, scn, accel, w, h)
        seen |= set(ref_surfaces(t, oracle, name, rd)["has"].tolist())
        for s in (64, 1):
            got = t.ao_rays(rd, samples=s, seed=0x9E3779B9, radius=2.5, bias=0.01)
            assert_words(got, ref_words(t, oracle, name, rd, s, 0x9E3779B9, 2.5, 0.01), (name, w, h, s))
            t.render_ao(rd, samples=s, seed=0x9E3779B9, radius=2.5, bias=0.01)
            want = AR.counts(oracle, scn, ref_words(t, oracle, name, rd, s, 0x9E3779B9, 2.5, 0.01), s)
            assert np.array_equal(t.read_ao()[0].reshape(-1), want), (name, w, h, s)
        t.close()
    assert seen == {True, False}
    # windows whose first item is no multiple of 64: the item index, not the lane's, seeds the ray
    w, h = 13, 7
    rd = A.ref_rd(name, w, h)
    t = handle(T, scn, accel, w, h)
    for s in (1, 2):
        whole = ref_words(t, oracle, name, rd, s, 0xFFFFFFFF, np.inf, 0.001)
        for first in (1, w * h - 2):
            assert (first * s) % 64 != 0
            got = t.ao_rays(rd, first=first, n=2, samples=s, seed=0xFFFFFFFF)
            assert_words(got, whole[first * s:(first + 2) * s], (name, s, first))
            mine = AR.records(oracle, ref_surfaces(t, oracle, name, rd), s, seed=0xFFFFFFFF, first=first, n=2)  # the reference's own window
            assert_words(got, mine, (name, s, first, "window"))
    t.close()


def count_cases(name):
    """(seed, radius, bias) per sample count: the scene's radius at the default bias, and a short radius from the surface itself"""
    radius = A.REF_VIEWS[name][3]
    return {1: [(1, radius, 0.001), (0xFFFFFFFF, min(radius, 2.5), 0.0)], 4: [(4, radius, 0.001), (0x9E3779B9, min(radius, 2.5), 0.01)],
            64: [(64, radius, 0.001), (0, min(radius, 2.5), 0.0)]}


@pytest.mark.parametrize("name,accel", A.REF_CASES)
def test_the_counts_equal_the_reference_integer_for_integer(name, accel, T, oracle):
    scn, (w, h) = A.ref_scene(name), (13, 7)
    rd = A.ref_rd(name, w, h)
    t = handle(T, scn, accel, w, h)
    has = ref_surfaces(t, oracle, name, rd)["has"].reshape(h, w)
    partial = 0
    for s in A.REF_SAMPLES:
        for seed, radius, bias in count_cases(name)[s]:
            kw = dict(samples=s, seed=seed, radius=radius, bias=bias)
            want = AR.counts(oracle, scn, ref_words(t, oracle, name, rd, s, seed, radius, bias), s).reshape(h, w)
            t.render_ao(rd, **kw)
            got, samples = t.read_ao()
            assert samples == s and got.dtype == np.uint32
            bad = np.flatnonzero(got != want)
            assert not len(bad), (name, accel, kw, bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist())
            assert np.array_equal(got == NONE, ~has)
            assert np.array_equal(got, reference_counts(t, rd, **kw)[0]), (name, accel, kw)  # and the occlusion query beside it
            partial += int(((want > 0) & (want < s)).sum()) if s > 1 else 0
    assert partial > 0 and t.counters()["watchdog"] == 0
    t.close()


def test_the_counts_of_a_refitted_tree_equal_the_reference(T, oracle):
    sh, tr, ma = A.ref_scene("mesh_smooth")
    w, h, s = 13, 7, 4
    rd = A.ref_rd("mesh_smooth", w, h)
    t = handle(T, (sh, tr, ma), "sah", w, h, refit=True)
    t.render_ao(rd, samples=s)
    first, _ = t.read_ao()
    moved = sh.copy()
    m = int(np.flatnonzero(sh["type"] == R.SHAPE_MODEL)[0])
    moved[m] = R.model(int(sh["material"][m]), tr, int(sh["triangle_index"][m]), int(sh["num_triangles"][m]),
                       R.mat_mul(R.translate((0.3, 0.15, -0.25)), sh["transform"][m]))
    t.update_scene(moved, tr, ma)
    assert t.acceleration_refit_info()["models"] >= 1
    words = ref_words(t, oracle, "mesh_smooth moved", rd, s, scn=(moved, tr, ma))
    assert_words(t.ao_rays(rd, samples=s), words, "refit")
    t.render_ao(rd, samples=s)
    second, _ = t.read_ao()
    want = AR.counts(oracle, (moved, tr, ma), words, s).reshape(h, w)
    assert np.array_equal(second, want) and not np.array_equal(first, second)
    assert np.array_equal(first, AR.counts(oracle, (sh, tr, ma), ref_words(t, oracle, "mesh_smooth", rd, s), s).reshape(h, w))
    t.close()


def test_a_groups_counts_and_rays_equal_the_reference(T, oracle):
    name, w, h, s = "boxes", 13, 7, 4
    scn = A.ref_scene(name)
    rd = A.ref_rd(name, w, h)
    t = handle(T, scn, "sah", w, h)
    words = ref_words(t, oracle, name, rd, s, 0x9E3779B9, 2.5, 0.01)
    t.close()
    g = T.TracerGroup(w, h, n_devices=2, devices=[0, 0], rows_per_block=1)
    g.set_acceleration(1)
    g.scene_data = R.scene_data(len(scn[0]))
    g.update_scene(*scn)
    kw = dict(samples=s, seed=0x9E3779B9, radius=2.5, bias=0.01)
    assert_words(g.ao_rays(rd, **kw), words, "group")
    g.render_ao(rd, **kw)
    got, samples = g.read_ao()
    assert samples == s and np.array_equal(got, AR.counts(oracle, scn, words, s).reshape(h, w))
    g.close()


@pytest.mark.parametrize("value,component", [(np.nan, 0), (np.inf, 1), (-np.inf, 2)])
def test_a_hostile_camera_has_no_surface(value, component, T, oracle):
    name, w, h, s = "spheres", 13, 7, 4
    scn = A.ref_scene(name)
    rd = A.hostile_rd(A.ref_rd(name, w, h), value, component)
    t = handle(T, scn, "scan", w, h)
    none = np.tile(np.array([0, 0, 0, AR.NAN_BITS, 0, 0, 0, 0], np.uint32), (w * h * s, 1))
    surf = AR.surfaces(oracle, scn, t.pick_rays(A.centres(w, h), rd))
    assert not surf["has"].any() and np.array_equal(AR.records(oracle, surf, s), none)  # so says the reference
    assert_words(t.ao_rays(rd, samples=s), none, (value, component))
    t.render_ao(rd, samples=s)
    got, _ = t.read_ao()
    assert (got == NONE).all() and t.counters()["watchdog"] == 0
    t.close()
