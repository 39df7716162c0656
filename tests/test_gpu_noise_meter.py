"""Noise metering on the device (include/srt_abi.h srt_set_noise_meter; csrc/noise_meter.hip) against its numpy restatement
(tests/noise_ref.py), tolerance zero: the kernel through its self-test entry on crafted frames at the lane, wave and workgroup
edges; traced frames; the stopping rule; srt_render_until against a manual loop; the automatic metering of the render calls; a
device group; and srt_headless --until-noise / --noise-view."""
import numpy as np
import pytest

import noise_ref as N
from conftest import bits_equal
from gpu_harness import T, make  # noqa: F401 (T: the fixture)
from simple_raytracer_amd import records as R

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, SPP = 48, 32, 2
SIZES = [1, 63, 64, 65, 255, 256, 257, W * H]
PAST_THE_GRID = 1024 * 256 + 257  # more pixels than one trip of the capped grid takes: the grid-stride loop's second trip
STATE = 3  # SRT_ERR_STATE


@pytest.fixture(scope="module")
def dev(T):
    """a handle for the self-test entry (which needs no scene and no denoiser)"""
    t = T.Tracer(8, 8)
    yield t
    t.close()


def up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def check(dev, canvas, moments, T_, P, what, **params):
    """both instantiations over one frame against the restatement: the record's integers, and the view's bytes"""
    want = N.meter(canvas, moments, T_, P, **params)
    heat = N.view(want["bins"], params.get("threshold", N.DEFAULTS["threshold"]))
    for view in (False, True):
        hist, counts, out = dev.selftest_noise_meter(canvas, moments, T_, P, view=view, **params)
        assert counts == (want["metered"], want["left_out"], want["below"]), (what, view, counts)
        assert np.array_equal(hist, want["hist"]), (what, view)
        if view:
            assert np.array_equal(out, heat), what
    return want


def black(n, r, P, floor=1.0):
    """n black pixels whose relative error is about r against a floor of 1: m2 = r^2 P (T = 1)"""
    r = np.broadcast_to(np.asarray(r, np.float64), (n,))
    return np.zeros((n, 4), F32), (r * r * P).astype(F32), dict(luminance_floor=floor)


def noise_frame(n, seed):
    """ordinary pixels: colours in 0 .. 3 (a tenth of them dark, under the floor), second moments from barely to far above L^2"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), F32)
    c[:, :3] = rng.uniform(0.0, 3.0, (n, 3)) * np.where(rng.uniform(size=(n, 1)) < 0.1, 1e-3, 1.0)
    c[:, 3] = rng.uniform(0, 1, n)
    L = N.D.lum(c[:, :3])
    return c, (L * L * (1 + np.exp2(rng.uniform(-16, 6, n)))).astype(F32)


# ---- 1. the kernel, through the self-test entry --------------------------------------------------------------------------------
def frame_log_uniform(n):
    """r log-uniform over 2^-26 .. 2^10: both clamps of the bin, and r on both sides of every threshold"""
    rng = np.random.default_rng(n)
    return (*black(n, np.exp2(rng.uniform(-26, 10, n)), 4), 1, 4)


def frame_one_bin(n):
    return (*black(n, 2.0 ** -3.3, 8), 1, 8)  # every wave votes: one add of the popcount


def frame_two_bins(n):
    return (*black(n, np.where(np.arange(n) % 2 == 0, 2.0 ** -7.4, 2.0 ** 1.7), 8), 1, 8)


def frame_all_bins(n):
    """bin k's middle for pixel i, k = i % 256: no two lanes of a wave agree"""
    k = np.arange(n) % 256
    return (*black(n, np.exp2((k // 8) - 24.0) * (1 + ((k % 8) + 0.5) / 8), 2), 1, 2)


@pytest.mark.parametrize("frame", [frame_log_uniform, frame_one_bin, frame_two_bins, frame_all_bins], ids=lambda f: f.__name__[6:])
def test_histograms_at_lane_wave_and_workgroup_edges(dev, frame):
    for n in SIZES:
        canvas, moments, params, T_, P = frame(n)
        want = check(dev, canvas, moments, T_, P, (frame.__name__, n), **params)
        assert want["metered"] == n
        if frame is frame_one_bin:
            assert np.count_nonzero(want["hist"]) == 1
        if frame is frame_two_bins and n > 1:
            assert np.count_nonzero(want["hist"]) == 2
        if frame is frame_all_bins and n >= 256:
            assert np.count_nonzero(want["hist"]) == 256
        if frame is frame_log_uniform and n >= 255:
            assert want["hist"][0] > 0 and want["hist"][255] > 0  # both clamps


def test_noise_frames_counts_and_the_second_trip(dev):
    for n in SIZES + [PAST_THE_GRID]:
        canvas, moments = noise_frame(n, seed=n)
        for T_, P in ((1, 1), (7, 13)):
            want = check(dev, canvas * F32(T_), moments * F32(T_), T_, P, (n, T_, P))
            assert want["left_out"] == 0 and (n < 64 or 0 < want["below"] < n)


def test_r_at_the_threshold_and_one_ulp_to_either_side(dev):
    canvas, moments = noise_frame(257, seed=77)
    r, met = N.relative_error(canvas, moments, 1, 4)
    assert met.all()
    for q in (0, 100, 256):
        rq = r[q]
        assert 2.0 ** -24 < rq < 2.0 ** 8
        counts = [check(dev, canvas, moments, 1, 4, (q, k), threshold=float(th))["below"] for k, th in enumerate((down(rq), rq, up(rq)))]
        assert counts[1] == counts[0] + int(np.sum(r == rq)) and counts[2] >= counts[1]  # r <= threshold: equality counts


def test_luminance_at_the_floor_and_one_ulp_to_either_side(dev):
    canvas, moments = noise_frame(257, seed=78)
    L = N.D.lum(canvas[:, :3])
    for q in (3, 130):
        for k, fl in enumerate((down(L[q]), L[q], up(L[q]))):
            assert 2.0 ** -20 <= fl <= 2.0 ** 20
            check(dev, canvas, moments, 1, 4, (q, k), luminance_floor=float(fl))
    # the floor at both ends of its range
    check(dev, canvas, moments, 1, 4, "low floor", luminance_floor=2.0 ** -20)
    check(dev, canvas, moments, 1, 4, "high floor", luminance_floor=2.0 ** 20)


SPECIALS = np.array([0.0, -0.0, 1e-40, np.nan, np.inf, -np.inf, 3e38, -1.0], F32)


def test_special_values_in_the_canvas_and_in_the_moments(dev):
    for n in (64, 65, 257, W * H):
        canvas, moments = noise_frame(n, seed=n + 1)
        where = np.random.default_rng(n).permutation(n)[:48]
        for j, q in enumerate(where):
            if j < 24:
                canvas[q, j % 3] = SPECIALS[j % 8]
            else:
                moments[q] = SPECIALS[j % 8]
        with np.errstate(all="ignore"):
            want = check(dev, canvas, moments, 2, 6, n)
        assert want["left_out"] > 0 and want["metered"] + want["left_out"] == n and want["metered"] > 0
    # a frame of nothing but left-out pixels, and a whole wave of them beside metered waves
    canvas, moments = noise_frame(256, seed=5)
    canvas[64:128, 1] = np.nan
    assert check(dev, canvas, moments, 1, 4, "a NaN wave")["left_out"] == 64
    canvas[:, 1] = np.inf
    want = check(dev, canvas, moments, 1, 4, "all inf")
    assert (want["metered"], want["left_out"], want["level_bin"]) == (0, 256, -1)


def test_nan_alpha_changes_nothing(dev):
    canvas, moments = noise_frame(W * H, seed=9)
    plain = N.meter(canvas, moments, 3, 6)
    canvas[:, 3] = np.nan
    want = check(dev, canvas, moments, 3, 6, "NaN alpha")
    assert want["left_out"] == 0 and np.array_equal(want["hist"], plain["hist"])


def test_converged_rules_at_the_integer_boundary(T, dev):
    """metered = 1000 with 949 and 950 pixels below the threshold, counted by the device; the rule is the library's"""
    for n_below, P, min_samples, want in ((949, 16, 16, 0), (950, 16, 16, 1), (950, 15, 16, 0), (1000, 1, 2, 0), (1000, 2, 2, 1), (0, 64, 16, 0)):
        r = np.where(np.arange(1000) < n_below, 0.01, 0.2)
        canvas, moments, params = black(1000, r, P)
        hist, counts, _ = dev.selftest_noise_meter(canvas, moments, 1, P, **params)
        assert counts == (1000, 0, n_below)
        got = T.noise_evaluate_host(hist, counts, 1, P, min_samples=min_samples)
        ref = N.meter(canvas, moments, 1, P, min_samples=min_samples, **params)
        assert got["converged"] == want == ref["converged"], (n_below, P, min_samples)
        assert got["level_bin"] == ref["level_bin"] and F32(got["level"]) == ref["level"]


# ---- 2. traced frames -----------------------------------------------------------------------------------------------------------
def set_time(t, base, i, stride=7919):
    t.options["time"] = np.uint32((base + i * stride) & 0xFFFFFFFF)


def ref_of(t, **params):
    inputs = t.read_denoise_inputs()
    return N.meter(t.read_canvas().reshape(-1, 4), inputs["moments"].reshape(-1), inputs["T"], inputs["P"], **params)


@pytest.mark.parametrize("scn", ["spheres", "meshes"])
def test_traced_frames_against_the_reference(T, sky, scn):
    params = dict(threshold=0.25, min_samples=8)
    t = make(T, sky, scn, W, H, spp=SPP, denoise=dict(iterations=0))
    off = make(T, sky, scn, W, H, spp=SPP, denoise=dict(iterations=0))
    t.set_noise_meter(**params)
    levels = []
    for i in range(16):
        for x in (t, off):
            set_time(x, 777, i)
            x.trace()
        if i + 1 in (1, 4, 16):
            t.meter_noise()
            got = t.read_noise()
            want = ref_of(t, **params)
            assert (want["dispatches"], want["samples"]) == (i + 1, SPP * (i + 1))
            assert N.same_record(got, want), (scn, i + 1, {k: v for k, v in got.items() if k != "hist"})
            assert want["metered"] + want["left_out"] == W * H and want["metered"] > W * H // 2
            assert np.array_equal(t.read_canvas().view(np.uint32), off.read_canvas().view(np.uint32))  # metering writes nothing the trace reads
            t.resolve_noise_view()
            assert np.array_equal(t.read_argb().reshape(-1, 4), N.view(want["bins"], params["threshold"]))
            assert N.same_record(t.read_noise(), want)
            levels.append(float(got["level"]))
    assert levels[0] > levels[1] > levels[2]  # the noise level falls as samples accumulate
    t.close()
    off.close()


# ---- 3. srt_render_until --------------------------------------------------------------------------------------------------------
EVERY, MIN_SAMPLES, MAXD, BASE = 2, 4, 24, 4242


def manual_loop(t, n, **params):
    """n dispatches with srt_render_until's times and a blocking metering at every eligible interval -> the checks' results"""
    t.clear_canvas()
    t.set_noise_meter(check_every=EVERY, min_samples=MIN_SAMPLES, **params)
    checks = []
    for i in range(n):
        set_time(t, BASE, i)
        t.trace()
        if (i + 1) % EVERY == 0 and SPP * (i + 1) >= MIN_SAMPLES:
            t.meter_noise()
            checks.append(t.read_noise())
    set_time(t, BASE, 0)
    return checks


def test_render_until_against_the_manual_loop(T, sky):
    t = make(T, sky, "spheres", W, H, spp=SPP, time=BASE, denoise=dict(iterations=0))
    checks = manual_loop(t, MAXD)
    assert [c["dispatches"] for c in checks] == list(range(2, MAXD + 1, EVERY))
    threshold = float(checks[2]["level"])  # what the loop measured at its third check
    checks = manual_loop(t, MAXD, threshold=threshold)
    converged = [c["dispatches"] for c in checks if c["converged"]]
    assert converged, "no check of the manual loop converged at the level its third check measured"
    t_star = converged[0]
    assert checks[0]["dispatches"] < t_star < checks[-1]["dispatches"]  # neither the first nor the last check
    done_want = min(t_star + EVERY, MAXD)
    deciding = manual_loop(t, done_want, threshold=threshold)[t_star // EVERY - 1]
    t.resolve_denoised(done_want)
    canvas, argb = t.read_canvas().copy(), t.read_argb().copy()
    # the call itself, from a clear
    t.clear_canvas()
    out, res, done = t.render_until(MAXD, time_stride=7919)
    assert res["converged"] == 1 and res["dispatches"] == t_star and done == done_want
    assert all(res[k] == deciding[k] for k in res), (res, {k: deciding[k] for k in res})
    assert np.array_equal(t.read_canvas().view(np.uint32), canvas.view(np.uint32))
    assert np.array_equal(out.reshape(-1, 4), argb.reshape(-1, 4))
    assert t.read_denoise_inputs()["T"] == done_want
    # max_dispatches == T*: the outstanding check is the deciding one
    t.clear_canvas()
    _, res, done = t.render_until(t_star)
    assert (res["converged"], res["dispatches"], done) == (1, t_star, t_star)
    # a threshold nothing reaches stops at max_dispatches, unconverged, and reports the last check
    t.set_noise_meter(check_every=EVERY, min_samples=MIN_SAMPLES, threshold=2.0 ** -24)
    t.clear_canvas()
    _, res, done = t.render_until(8)
    assert (res["converged"], res["dispatches"], done) == (0, 8, 8)
    # a threshold everything is below stops one interval past the first eligible check
    t.set_noise_meter(check_every=EVERY, min_samples=MIN_SAMPLES, threshold=2.0 ** 8)
    t.clear_canvas()
    _, res, done = t.render_until(MAXD)
    assert (res["converged"], res["dispatches"], done) == (1, 2, 4)
    # fewer dispatches than the first check needs: no check, an empty result
    t.clear_canvas()
    _, res, done = t.render_until(1)
    assert (res["converged"], res["dispatches"], res["metered"], res["level_bin"], done) == (0, 0, 0, -1, 1)
    t.close()


# ---- 4. state, polling, the automatic metering ----------------------------------------------------------------------------------
def test_poll_after_synchronize_and_state_errors(T, sky):
    t = make(T, sky, "spheres", W, H, spp=SPP)
    with pytest.raises(T.SrtError) as e:  # the denoiser is off
        t.set_noise_meter()
    assert e.value.code == STATE
    t.set_denoise(iterations=0)
    t.set_noise_meter()
    for call in (t.meter_noise, t.resolve_noise_view, t.read_noise):  # nothing traced, nothing metered
        with pytest.raises(T.SrtError) as e:
            call()
        assert e.value.code == STATE, call
    assert t.poll_noise() is None  # a front-end that only polls sees "not ready"
    t.trace()
    t.meter_noise()
    t.synchronize()
    polled = t.poll_noise()
    assert polled is not None and N.same_record(polled, t.read_noise()) and N.same_record(polled, ref_of(t))
    t.set_denoise(False)  # the moments stop accumulating: no metering
    with pytest.raises(T.SrtError) as e:
        t.meter_noise()
    assert e.value.code == STATE
    with pytest.raises(T.SrtError) as e:
        t.render_until(4)
    assert e.value.code == STATE
    t.set_noise_meter(False)
    t.set_partition(0, 2)  # a partitioned handle
    with pytest.raises(T.SrtError) as e:
        t.set_noise_meter()
    assert e.value.code == STATE
    with pytest.raises(T.SrtError):
        make(T, sky, "spheres", W, H, spp=SPP, denoise=dict(iterations=0)).set_noise_meter(permille=0)
    t.close()


def test_meter_off_enqueues_what_it_did_and_on_meters_every_interval(T, sky):
    never = make(T, sky, "spheres", W, H, spp=SPP, denoise=dict(iterations=0))
    t = make(T, sky, "spheres", W, H, spp=SPP, denoise=dict(iterations=0))
    t.set_noise_meter(check_every=2)
    t.set_noise_meter(False)
    for k in range(2):
        for x in (never, t):
            set_time(x, 777, k)
        a, b = never.render(k + 1).copy(), t.render(k + 1).copy()
        assert np.array_equal(a, b)
        assert not t.last_meter_ran() and not never.last_meter_ran()
        assert t.last_trace_launches() == never.last_trace_launches()
        assert t.last_resolve_exposed() == never.last_resolve_exposed() and t.last_resolve_bloomed() == never.last_resolve_bloomed()
    with pytest.raises(T.SrtError):  # off, and nothing was ever metered on this handle
        t.read_noise()
    t.set_noise_meter(check_every=2)
    buf = np.zeros(W * H * 4, np.uint8)
    ran = []
    for k in range(2, 6):
        set_time(t, 777, k)
        if k % 2:
            t.render_async(k + 1, buf)
            t.synchronize()
        else:
            t.render(k + 1)
        ran.append(t.last_meter_ran())
        if ran[-1]:
            assert N.same_record(t.read_noise(), ref_of(t, check_every=2))
    assert ran == [False, True, False, True]  # T = 3, 4, 5, 6
    never.close()
    t.close()


def test_pipelined_frames_meter_like_blocking_meterings(T, sky):
    params = dict(check_every=1, threshold=0.5)
    blocking = make(T, sky, "meshes", W, H, spp=SPP, denoise=dict(iterations=0))
    blocking.set_noise_meter(check_every=65536, threshold=0.5)
    piped = make(T, sky, "meshes", W, H, spp=SPP, denoise=dict(iterations=0))
    piped.set_noise_meter(**params)
    buf = np.zeros(W * H * 4, np.uint8)
    for k in range(3):
        for x in (blocking, piped):
            set_time(x, 99, k)
        blocking.trace()
        blocking.meter_noise()
        want = blocking.read_noise()
        piped.render_pipelined(k + 1, buf)
        assert piped.last_meter_ran()
        got = piped.read_noise()
        assert N.same_record(got, want) and got["dispatches"] == k + 1
    piped.pipeline_flush(buf)
    assert N.same_record(piped.poll_noise(), ref_of(piped, **params))
    blocking.close()
    piped.close()


def test_group_meters_the_gathered_planes(T, sky):
    params = dict(threshold=0.3)
    t = make(T, sky, "spheres", W, H, spp=SPP, denoise=dict(iterations=0))
    t.set_noise_meter(**params)
    g = T.TracerGroup(W, H, n_devices=2, devices=[0, 0], rows_per_block=8)
    g.set_skybox(sky)
    g.options, g.scene_data = t.options.copy(), t.scene_data.copy()
    g.update_scene(*t.scene)
    g.clear_canvas()
    with pytest.raises(T.SrtError) as e:  # the group's denoiser is off
        g.set_noise_meter(**params)
    assert e.value.code == STATE
    g.set_denoise(iterations=0)
    g.set_noise_meter(**params)
    for k in range(2):
        for x in (t, g):
            set_time(x, 777, k)
        t.trace()
        g.trace_and_gather()
    t.meter_noise()
    g.meter_noise()
    single, group = t.read_noise(), g.read_noise()
    assert N.same_record(group, single) and N.same_record(single, ref_of(t, **params)) and single["dispatches"] == 2
    t.resolve_noise_view()
    g.resolve_noise_view()
    assert np.array_equal(g.read_noise_view(), t.read_argb())
    assert N.same_record(g.poll_noise() or g.read_noise(), single)
    g.set_noise_meter(False)
    with pytest.raises(T.SrtError):
        g.meter_noise()
    g.close()
    t.close()


# ---- 5. srt_headless ------------------------------------------------------------------------------------------------------------
def test_headless_until_noise_equals_the_library_call(T, tmp_path):
    import re
    import subprocess
    from simple_raytracer_amd import build
    exe = build.build_headless()
    pre, heat = tmp_path / "h", tmp_path / "heat.ppm"
    run = subprocess.run([str(exe), "--scene", "spheres", "--width", str(W), "--height", str(H), "--spp", str(SPP), "--time", "4242", "--until-noise", "0.5:40:900",
                          "--noise-view", str(heat), "--dump", str(pre)], check=True, timeout=120, capture_output=True, text=True)
    m = re.search(r"until-noise: (\w+ ?\w*) after (\d+) dispatches; deciding check at T = (\d+), P = (\d+): level (\S+) \(bin (-?\d+)\)", run.stdout)
    assert m, run.stdout
    rd = np.fromfile(f"{pre}.rd.bin", R.RENDER_DATA).reshape(())
    sd = np.fromfile(f"{pre}.sd.bin", R.SCENE_DATA).reshape(())
    shapes, tris, mats = np.fromfile(f"{pre}.shapes.bin", R.SHAPE), np.fromfile(f"{pre}.tris.bin", R.TRIANGLE), np.fromfile(f"{pre}.mats.bin", R.MATERIAL)
    t = T.Tracer(W, H)
    t.set_skybox(np.fromfile(f"{pre}.sky.bin", np.float32).reshape(1024, 2048, 4))
    t.set_denoise(iterations=0)
    t.set_noise_meter(threshold=0.5, permille=900)
    t.scene_data = sd.copy()
    t.scene_data["num_shapes"] = 0  # as Tracer::update_scene before its first call
    t.clear_canvas()
    t.update_scene(shapes, tris, mats)
    t.options = rd.copy()
    assert int(rd["time"]) == 4242 and int(rd["num_samples"]) == SPP
    out, res, done = t.render_until(40, time_stride=7919)
    assert m.group(1) == ("converged" if res["converged"] else "NOT converged")
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(6))) == (done, res["dispatches"], res["samples"], res["level_bin"])
    assert res["converged"] == 1 and 4 < done < 40  # the rule decided, not a limit: min_samples 16 at 2 spp makes T = 8 the first check
    assert F32(float(m.group(5))) == F32(float(f"{float(res['level']):.6g}"))
    assert np.array_equal(np.fromfile(f"{pre}.argb.bin", np.uint8), out)
    assert bits_equal(np.fromfile(f"{pre}.canvas.bin", np.float32), t.read_canvas().reshape(-1))
    t.resolve_noise_view()
    want = t.read_argb().reshape(-1, 4)[:, 1:]
    data = heat.read_bytes()
    assert data.startswith(b"P6") and np.array_equal(np.frombuffer(data[-W * H * 3:], np.uint8).reshape(-1, 3), want)
    t.close()
    bad = subprocess.run([str(exe), "--gpus", "2", "--until-noise", "0.1", "--parse-only"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--until-noise" in bad.stderr
