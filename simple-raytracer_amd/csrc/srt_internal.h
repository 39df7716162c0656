// srt_internal.h — the handle behind `srt_tracer *` and the small helpers the translation units of
// libsrt_hip.so share (srt_abi.hip: life cycle, scene upload, trace; accel_device.hip: BVH upkeep on the device;
// srt_collect.hip: multi-GPU collection; srt_group.hip: the device group; frame_pipeline.hip: the frame pipeline). What of the host side needs no handle and no HIP is not here: bvh_host.h, scene_prep.h, trace_plan.h, denoise_plan.h.
// Not part of the public ABI.
#ifndef SRT_INTERNAL_H
#define SRT_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "../../include/srt_abi.h"
#include "denoise_plan.h"
#include "device_types.h"
#include "scene_prep.h"

template <class T>
struct DevBuf {
	T *ptr = nullptr;
	size_t cap = 0; // elements
	// "buffers only ever grow" (src/tracer.cpp:5-9)
	hipError_t reserve(size_t n) {
		if (n < 1) n = 1;
		if (n <= cap) return hipSuccess;
		if (ptr) (void)hipFree(ptr);
		ptr = nullptr;
		cap = 0;
		hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr), n * sizeof(T));
		if (e == hipSuccess) cap = n;
		return e;
	}
	void release() {
		if (ptr) (void)hipFree(ptr);
		ptr = nullptr;
		cap = 0;
	}
};

// A device result on its way to the host: a pinned host copy that only ever grows, the event behind the copy (made with the
// first buffer), `pending` until somebody has waited for it
template <class T>
struct PinnedReadback {
	T *host = nullptr; // pinned, cap elements
	size_t cap = 0;
	hipEvent_t done = nullptr;
	bool pending = false;
	hipError_t reserve(size_t n) {
		if (cap < n) {
			if (host) (void)hipHostFree(host);
			host = nullptr, cap = 0;
			if (hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&host), n * sizeof(T), hipHostMallocDefault)) return e;
			cap = n;
		}
		return done ? hipSuccess : hipEventCreateWithFlags(&done, hipEventDisableTiming);
	}
	hipError_t copy(const T *dev, size_t n, hipStream_t stream) { // n <= cap elements, behind what the stream holds
		hipError_t e = hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream);
		if (e == hipSuccess) e = hipEventRecord(done, stream);
		pending = e == hipSuccess;
		return e;
	}
	hipError_t wait() { // for the copy alone, not for the stream
		const hipError_t e = pending ? hipEventSynchronize(done) : hipSuccess;
		if (e == hipSuccess) pending = false;
		return e;
	}
	void release() {
		if (host) (void)hipHostFree(host);
		if (done) (void)hipEventDestroy(done);
		*this = PinnedReadback();
	}
};

// Two events around a stretch of a stream, made on first use; `timed` once the second is recorded (the owner clears it)
struct TimedSpan {
	hipEvent_t ev[2] = {nullptr, nullptr};
	bool timed = false;
	hipError_t begin(hipStream_t stream) {
		for (hipEvent_t &e : ev)
			if (hipError_t rc = e ? hipSuccess : hipEventCreate(&e)) return rc;
		return hipEventRecord(ev[0], stream);
	}
	hipError_t end(hipStream_t stream) {
		const hipError_t e = hipEventRecord(ev[1], stream);
		timed = e == hipSuccess;
		return e;
	}
	hipError_t elapsed(float *ms) const { return timed ? hipEventElapsedTime(ms, ev[0], ev[1]) : hipSuccess; } // (the stream has passed it)
	void release() {
		for (hipEvent_t e : ev)
			if (e) (void)hipEventDestroy(e);
		*this = TimedSpan();
	}
};

// Upkeep of the BVH on the device (accel_device.hip, which alone reads it): the state of the last upload, by owner
struct AccelDevice {
	// in-place refit (bvh_refit.hip; SRT_REFIT_DEVICE): the refitted models, their extents, inner blocks by level, a box per block
	DevBuf<RefitModel> refit_models;
	DevBuf<uint32_t> refit_extents, refit_sched;
	DevBuf<float> refit_boxes;
	uint64_t refit_info[4] = {0, 0, 0, 0};
	TimedSpan refit_span; // around the refit launches, when the kernel timers are on
	// a deformed model keeps its hierarchy (SRT_DEFORM_REFIT): the counts, the cost launch's inputs on the device and its sums
	// on their way back (pending until srt_accel_deform_consume)
	uint64_t deform_info[4] = {0, 0, 0, 0};
	DevBuf<RefitCostRange> deform_ranges;
	DevBuf<uint8_t> deform_weights;
	DevBuf<double> deform_sums;
	PinnedReadback<double> deform_sums_back;
	std::vector<size_t> deform_entry;  // per refitted model: its entry in the cache, its cost as built
	std::vector<double> deform_built, deform_ratio; // deform_ratio: cost now / as built once the sums are in; 0 = unknown
	std::vector<uint8_t> deform_fresh; // per cost range: a model built by that upload (its sum is its cost as built)
	double deform_worst_host = 0.0;    // the largest ratio among the models the device did not refit
	// a model's hierarchy built on the device (bvh_build.hip; SRT_BUILD_DEVICE): the built models, their extents, the sort's two
	// key / index buffers (a slot per record of the scene) and its histogram table, the counts, and the scene's sorted order
	// array on its way back (pending until srt_accel_build_consume)
	DevBuf<RefitModel> build_models;
	DevBuf<uint32_t> build_extents, build_keys[2], build_vals[2], build_table;
	DevBuf<uint32_t> build_ranges_dev; // SRT_BUILD_ORDER_MEDIAN only: per built model its first range slot, then six dwords per range (device_types.h BuildParams)
	std::vector<uint32_t> build_ranges_host; // ... and what it is uploaded from
	uint64_t build_info[4] = {0, 0, 0, 0};
	PinnedReadback<uint32_t> build_order_back;
	std::vector<size_t> build_entry;      // per built model: its entry in the cache ...
	std::vector<RefitModel> build_ranges; // ... and its records
	TimedSpan build_span; // around the build launches and the refit behind them, when the kernel timers are on
	void release() {
		refit_models.release(), refit_extents.release(), refit_sched.release(), refit_boxes.release(), refit_span.release();
		deform_ranges.release(), deform_weights.release(), deform_sums.release(), deform_sums_back.release();
		build_models.release(), build_extents.release(), build_table.release(), build_ranges_dev.release();
		for (int k = 0; k < 2; k++) build_keys[k].release(), build_vals[k].release();
		build_order_back.release(), build_span.release();
	}
};

// Exposure for the resolve (exposure.hip; srt_set_exposure): the switch and its parameters, and the device record that holds
// the histogram, the adaptation state and the scalar the exposed resolve reads (made when the feature is first enabled)
struct ExposureState {
	bool on = false;
	bool last_exposed = false; // srt_last_resolve_exposed: the last resolve of a site went through the exposed kernel
	srt_exposure_params p{};
	DevBuf<uint32_t> record;
};

// Bloom for the resolve (bloom.hip; srt_set_bloom): the switch and its parameters, the pyramid (every level's float4 texels one
// after the other, made when the feature is first enabled) and the shape of the last bloomed frame's (srt_read_bloom)
struct BloomState {
	bool on = false;
	bool last_bloomed = false; // srt_last_resolve_bloomed: the last resolve of a site went through the bloom composite
	srt_bloom_params p{};
	DevBuf<float> pyramid;
	int last_w = 0, last_h = 0, last_levels = 0;
};

// Noise metering (noise_meter.hip; srt_set_noise_meter): the switch and its parameters, the device record one metering adds into
// and its pinned copies (made when the feature is first enabled). Two copies, taken in turn: srt_render_until reads check k - 1
// while check k is in flight. `enqueued` counts the meterings; the newest one's copy is back[(enqueued - 1) & 1]
struct NoiseState {
	bool on = false;
	bool last_ran = false; // srt_last_meter_ran: the last resolving call of a site metered its frame
	srt_noise_params p{};
	DevBuf<uint32_t> record;
	PinnedReadback<uint32_t> back[2];
	uint64_t enqueued = 0;
	void release() {
		record.release();
		for (PinnedReadback<uint32_t> &b : back) b.release();
	}
};

// Selection overlay and ID pass (selection.hip; srt_set_selection, srt_render_ids): the switch, its parameters and the set as
// given; the set as a bit table sized to the scene it was made for and the outline's alpha table, both uploaded when they
// change (their host copies stay put between two srt_set_selection, which wait for the stream); the ID planes (shape,
// triangle, material: three planes of ids_w x ids_h words) with the key they were made under; the alpha plane of the last
// overlaid frame
struct SelectionKey {
	uint64_t scene_rev;
	const void *scene, *tri_materials; // the handle whose scene was walked, its per-triangle material table
	float camera_to_world[16], aspect_ratio, fov_scale;
	int32_t width, height;
};
struct SelectionState {
	bool on = false;
	bool last_applied = false, last_id_ran = false; // srt_last_resolve_selected
	srt_selection_params p{};
	std::vector<uint32_t> shapes;
	srt_tracer *scene = nullptr; // the handle srt_set_selection was called on: its scene and its last dispatch's camera
	std::vector<uint32_t> bits_host;
	DevBuf<uint32_t> bits;
	uint32_t bits_shapes = 0;    // shapes the table covers
	uint64_t bits_rev = 0;       // the scene revision it was made for
	bool bits_dirty = true;
	uint8_t table_host[SRT_SELECTION_TABLE_MAX + 3] = {};
	DevBuf<uint8_t> table;
	int radius = 0;
	bool table_dirty = true;
	DevBuf<uint32_t> ids;
	int ids_w = 0, ids_h = 0;
	bool ids_valid = false;
	SelectionKey ids_key{};
	DevBuf<uint8_t> alpha;
	int alpha_w = 0, alpha_h = 0;
	void release() { bits.release(), table.release(), ids.release(), alpha.release(); }
};

// Ambient-occlusion pass (ao.hip; srt_render_ao): the surface records (two float4 per pixel) and the count plane of the last
// pass with its frame and parameters, and the view's grey table on the device (uploaded when the sample count changes; its
// host copy stays put between two such changes, which wait for the stream)
struct AoState {
	DevBuf<float> surfaces;
	DevBuf<uint32_t> occluded;
	int w = 0, h = 0; // of the last pass; 0: none yet
	srt_ao_params p{};
	uint8_t table_host[SRT_AO_MAX_SAMPLES + 1 + 3] = {};
	DevBuf<uint8_t> table;
	uint32_t table_samples = 0; // the sample count the device table was made for; 0: none
	void release() { surfaces.release(), occluded.release(), table.release(); }
};

// Area selection (area.hip; srt_area_coverage ...): the result of the last coverage call on the device -- the 8 words of an
// srt_area_summary, then the counts -- its pinned copy, the timers' span around the last call's clear and launches, and whether
// that call had to make the ID planes (srt_last_area_id_pass). All made on first use
struct AreaState {
	DevBuf<uint32_t> out;
	PinnedReadback<uint32_t> back;
	TimedSpan span;
	bool last_id_ran = false;
	void release() { out.release(), back.release(), span.release(); }
};

struct SrtCollect;  // collect_internal.h (srt_collect.hip): RCCL communicator, gathered canvases
struct SrtPipeline; // frame_pipeline.hip: copy stream, the two frames in flight

struct srt_tracer {
	int width = 0, height = 0, device = 0;
	SrtCollect *collect = nullptr;
	SrtPipeline *pipeline = nullptr;
	hipStream_t own_stream = nullptr, stream = nullptr;
	DevBuf<float> canvas_own;
	float *canvas = nullptr;
	size_t canvas_bytes = 0; // of the buffer in use
	DevBuf<uint8_t> argb;
	DevBuf<srt_shape> shapes;
	DevBuf<BlockGroup> runs; // group headers of the packed shape blocks
	DevBuf<float> run_data;
	DevBuf<WinnerRec> winners;
	int num_runs = 0;
	size_t num_materials = 0;
	DevBuf<srt_triangle> triangles;
	DevBuf<srt_material> materials;
	DevBuf<float> wtris;
	DevBuf<uint32_t> wtri_offset;
	DevBuf<float> sky;
	DevBuf<uint32_t> bvh_blocks; // wide hierarchy, 32 dwords per block (device_types.h)
	DevBuf<uint32_t> bvh_order, bvh_dest;
	AccelPolicy policy;              // what the next srt_update_scene builds and who keeps it up (scene_prep.h; the srt_set_acceleration* setters)
	bool bvh_active = false;         // the current scene's models carry BVH roots
	uint64_t bvh_info[7] = {0, 0, 0, 0, 0, 0, 0};
	size_t bvh_num_blocks = 0;       // blocks of the current scene in bvh_blocks (srt_read_bvh_blocks)
	AccelDevice upkeep;              // refit, deform cost and build on the device (accel_device.hip)
	struct BvhCache *bvh_cache = nullptr; // hierarchies of the previous srt_update_scene (bvh_host.h BvhCacheEntry; made by scene_prep.cpp)
	DevBuf<unsigned long long> counters;
	DevBuf<unsigned long long> wave_counters; // per persistent wave, summed in srt_get_counters
	DevBuf<float> scan_queue;                 // array scan: per persistent wave (two sets, as the counters), allocated when first needed
	DevBuf<float> radiance;  // 3 floats per (pixel, sample) of the current batch
	DevBuf<float> running;   // float4 per pixel, carries the ordered sum across batches
	size_t radiance_budget = 0; // bytes; 0 = pick from free HBM at first use
	size_t radiance_budget_env = 0; // bytes from SRT_RADIANCE_BUDGET_MB as srt_create found it; 0 = not set
	int num_cus = 0;
	int last_waves_per_cu = 0, last_grid = 0;
	std::vector<hipEvent_t> ev_k; // one pair per sample batch, around srt_trace_kernel alone (reduce excluded)
	// dispatches of several sample batches: even / odd batches trace on two streams of their own so that one batch's tail
	// (its last long paths, a few lanes per wave) runs under the next batch's start; the reductions stay in order on `stream`
	hipStream_t batch_stream[2] = {nullptr, nullptr};
	bool timers_in_render = false; // srt_render / srt_render_async / srt_render_pipelined record the kernel timers' events too (srt_set_kernel_timers)
	bool queue_dirty[2] = {false, false}; // a trace launch used the work cursor and no reduction has reset it since (srt_trace)
	hipEvent_t ev_batch_traced[2] = {nullptr, nullptr}, ev_batch_reduced[2] = {nullptr, nullptr}, ev_batch_fork = nullptr;
	bool batches_overlapped = false; // the last srt_trace ran that way (srt_last_trace_kernel_ms: a span, not a sum)
	size_t ev_k_used = 0;         // events of the last srt_trace
	float last_trace_kernel_ms = 0.f, last_reduce_ms = 0.f;
	int sky_w = 0, sky_h = 0;
	srt_scene_data sd{};
	int num_models = 0;
	bool all_materials_ok = false; // no shape of the scene has a negative material index
	bool unit_materials = false;   // the device material table holds bernoulli() thresholds (srt_update_scene)
	int material_flags = 0;        // SRT_MF_* (device_types.h)
	uint32_t one_group_code = 0;   // the header of a sphere / plane scene that is ONE block group over shapes 0 .. n - 1, else 0 (scene classes)
	uint32_t plane_axes = 0;       // that group's plane form: 2 bits per plane slot (device_types.h "Axis planes")
	uint64_t scan_tris = 0; // array scan: triangles of the models a ray can be made to scan (all of them), for the launch-length bound
	bool scene_set = false;
	bool count_tris = false;
	int rank = 0, world = 1, rows_per_block = 8, owned_rows = 0;
	// edge-aware denoiser (denoise.hip; srt_set_denoise). Full frame only: never on together with world > 1.
	DenoiseSettings dn;       // what the setters of denoise.hip and temporal.hip set (denoise_plan.h)
	FilterPlan last_filter;   // the plan of the last filter (srt_last_filter_demodulated, _spatial_variance), its feedback of the last pass 1 (srt_last_filter_history_feedback)
	SetupPlan last_setup;     // the plan of the last temporal set-up (srt_last_setup_history_illumination, srt_last_setup_history_clamp)
	bool dn_filtered = false; // dn_col[dn_out] holds a filter result (srt_read_denoised)
	uint32_t dn_T = 0, dn_P = 0, dn_F = 0; // since the last clear: dispatches, sum of num_samples, feature rays per pixel
	uint64_t dn_serial = 0;                // srt_denoise_count: names what is traced (a StagingKey's serial)
	DevBuf<float> dn_nd, dn_ah, dn_mom;    // guide sums (float4 {normals, t}, float4 {albedos, hits}) and moments per pixel
	DevBuf<float> dn_guide;                // filter set-up: 2 float4 per pixel {N, Z}, {A, cov}
	DevBuf<float> dn_col;                  // two float4 images {colour, variance}, ping-pong between passes
	int dn_out = 0;                        // the image of dn_col the last pass wrote
	srt_render_data dn_cam{};              // the last dispatch's render data since the clear (its camera: temporal reprojection)
	// temporal reprojection (temporal.hip; srt_set_denoise_temporal). Two history sets, each px x 14 floats: float4
	// {colour, count}, float2 {m1, m2}, 2 float4 guide; tp_set[tp_cur] is the history, the other the frame being integrated
	DevBuf<float> tp_set[2];
	int tp_cur = 0;
	bool tp_valid = false;   // tp_set[tp_cur] holds a history
	std::optional<StagingKey> tp_staged; // srt_temporal_setup: what it made tp_set[1 - tp_cur] under; the commit swaps that set in when the key then is equal, else makes the set itself
	srt_render_data tp_cam{}; // the history frame's render data
	DevBuf<float> tp_bounds;       // the history clamp: two float4 planes {mu, sum of weights}, {sigma, taps} (allocated on the first enable; no part of the history)
	bool tp_bounds_ran = false;    // srt_temporal_bounds_kernel has written tp_bounds at least once (srt_read_denoise_history_bounds)
	std::vector<uint8_t> scene_bytes; // the last srt_update_scene's arrays and scene data (the history survives an unchanged scene)
	// object motion (temporal.hip; srt_set_denoise_object_motion): the feature pass stores a shape index per pixel into
	// om_ids[om_cur]; the commit swaps, so om_ids[1 - om_cur] belongs to the history, traced with the scene om_hist_scene
	DevBuf<uint32_t> om_ids[2];
	int om_cur = 0;
	bool om_mixed = false;     // the frame on the canvas was traced with more than one scene (or without indices): it cannot become a history
	bool om_any_moved = false; // a shape of om_table is not SRT_MOTION_STATIC (the moved set-up kernel runs)
	std::vector<uint8_t> om_hist_scene; // scene_bytes of the history frame
	std::vector<uint32_t> om_table;     // SRT_MOTION_WORDS per shape of the current scene: the next filter's current -> history maps
	DevBuf<uint32_t> om_table_dev;
	// per-triangle motion (temporal.hip; srt_set_denoise_vertex_motion): beside the shape index the feature pass stores the
	// hit triangle's index inside its model into vm_tri[om_cur], and vm_rows[om_cur] holds the frame's world vertices (9
	// floats per instance triangle, shape vm_first[s]'s first row; vm_first[n_shapes] = all rows). The commit swaps both
	// with om_cur. vm_ver[k] names the scene vm_rows[k] was written from (0: none), vm_scene_ver the current scene
	bool om_any_deformed = false; // a shape of om_table is SRT_MOTION_DEFORMED (the deform set-up kernel runs)
	DevBuf<uint32_t> vm_tri[2];
	DevBuf<float> vm_rows[2];
	std::vector<uint32_t> vm_first;
	DevBuf<uint32_t> vm_first_dev;
	uint64_t vm_scene_ver = 1, vm_ver[2] = {0, 0};
	// group denoiser (srt_group.hip srt_group_set_denoise): a member of a device group accumulates the denoiser's inputs for
	// its OWN rows, packed as its canvas rows are. gd_pack is ONE allocation of srt_planes_slot_floats() floats that one collective
	// sends: the canvas rows (bound as the canvas, the way srt_bind_canvas does), the normal_depth and albedo_hits planes
	// (float4 per pixel of the padded rows each) and the moments plane. The filter runs on the group's full-frame resolver
	// handle; dn.on stays false here, and the public per-handle rules (no denoiser on a partitioned handle) are unchanged.
	bool gd_on = false;
	int gd_feature_samples = 0;
	DevBuf<float> gd_pack;
	float *gd_prev_canvas = nullptr; // what was bound before, bound again when the group's denoiser goes off
	size_t gd_prev_bytes = 0;
	// albedo textures (srt_texture.hip; include/srt_abi.h). What the three setters were given lives on the host; the device
	// tables are (re)made by srt_texture_sync when a setter or srt_update_scene has run since (tex_dirty)
	std::vector<TexDesc> tex_images;                // srt_set_textures: the images inside tex_texels
	std::vector<srt_material_texture> tex_bindings; // srt_set_material_textures, as given
	std::vector<float> tex_uv_host;                 // srt_set_triangle_uvs
	bool tex_has_uvs = false;
	std::vector<int32_t> tex_tm_host;               // srt_set_triangle_materials
	bool tex_has_tm = false;
	std::vector<PlaneFrame> tex_frames_host; // per shape of the current scene (srt_update_scene)
	size_t tex_scene_triangles = 0;          // of the current scene
	DevBuf<float> tex_texels, tex_uvs;
	DevBuf<TexDesc> tex_descs;
	DevBuf<srt_material_texture> tex_bind_dev; // one per material of the scene
	DevBuf<PlaneFrame> tex_frames;
	DevBuf<int32_t> tex_tm;
	bool tex_dirty = false;
	bool tex_tm_active = false;      // the table has an entry >= 0 and the current scene has triangles
	bool tex_active = false;         // a material of the current scene has a texture bound, or tex_tm_active: dispatches launch the textured kernels
	bool last_trace_textured = false; // srt_last_trace_textured
	int last_trace_class = 0;         // srt_last_trace_class
	ExposureState ex_own;             // exposure.hip ...
	ExposureState *ex = &ex_own;      // ... through this: a group's full-frame resolver handle shares the first member's (srt_group.hip resolver_of)
	BloomState bl_own;                // bloom.hip ...
	BloomState *bl = &bl_own;         // ... shared the same way
	NoiseState nz_own;                // noise_meter.hip ...
	NoiseState *nz = &nz_own;         // ... shared the same way
	uint32_t last_trace_plane_form = 0; // srt_last_trace_plane_form
	SelectionState sel_own;           // selection.hip ...
	SelectionState *sel = &sel_own;   // ... shared the same way
	uint64_t scene_rev = 0;           // bumped by every successful srt_update_scene (the ID planes' key)
	srt_render_data last_rd{};        // the most recent dispatch's options (the overlay's camera) ...
	bool have_last_rd = false;        // ... once there was one
	// ray and occlusion queries (ray_query.hip, occlusion.hip): the host forms' one staging allocation, sized for the largest
	// call so far and laid out per call by query_stage.h, and the timers' span around the last query's launches
	DevBuf<uint8_t> rq_stage;
	TimedSpan rq_span;
	AoState ao; // ao.hip
	AreaState ar; // area.hip
	hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr, ev_r0 = nullptr, ev_r1 = nullptr;
	bool have_trace_ev = false, have_resolve_ev = false, have_kernel_ev = false;
	std::string err;
};

int srt_fail(srt_tracer *t, int code, const std::string &msg); // records the text for srt_last_error (t == NULL: srt_create's)
static inline int fail(srt_tracer *t, int code, const std::string &msg) { return srt_fail(t, code, msg); }
// pixels of the rows this handle owns (srt_set_partition) and of the whole frame (the denoiser's buffers)
static inline size_t owned_pixels(const srt_tracer *t) { return (size_t)t->owned_rows * (size_t)t->width; }
static inline size_t full_pixels(const srt_tracer *t) { return (size_t)t->width * (size_t)t->height; }

// group denoiser: pixels of one plane of a member's gd_pack (the padded rows every rank sends), the float offsets of its four
// planes and the floats of the whole (the moments plane is padded so that every rank's slot of the gathered buffer starts
// on 16 bytes)
static inline size_t gd_plane_pixels(int width, int height, int world, int rpb) { return (size_t)srt_partition_padded_rows(height, world, rpb) * (size_t)width; }
static inline size_t gd_slot_floats(size_t plane_pixels) { return 12 * plane_pixels + ((plane_pixels + 3) & ~(size_t)3); }
static inline float *gd_normal_depth(const srt_tracer *t) { return t->gd_pack.ptr + 4 * gd_plane_pixels(t->width, t->height, t->world, t->rows_per_block); }
static inline float *gd_albedo_hits(const srt_tracer *t) { return t->gd_pack.ptr + 8 * gd_plane_pixels(t->width, t->height, t->world, t->rows_per_block); }
static inline float *gd_moments(const srt_tracer *t) { return t->gd_pack.ptr + 12 * gd_plane_pixels(t->width, t->height, t->world, t->rows_per_block); }

#define SRT_HIP(t, call)                                                                              \
	do {                                                                                              \
		hipError_t e_ = (call);                                                                       \
		if (e_ != hipSuccess)                                                                         \
			return fail((t), SRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));         \
	} while (0)


void srt_collect_release(srt_tracer *t); /* srt_destroy: the communicator srt_comm_init made, the gathered buffers */
__attribute__((visibility("hidden"))) void srt_pipeline_release(srt_tracer *t); /* ... then the copy stream (waited for), the frames' buffers, the events */
int srt_accel_deform_consume(srt_tracer *t, BvhCache *cache); /* accel_device.hip, before the host pass: the last upload's cost sums become ratios, here and in `cache` (the handle's own, a group's first member's) */
int srt_accel_build_consume(srt_tracer *t, BvhCache *cache);  /* before the host pass: the last upload's sorted order goes to its entries of `cache` */
int srt_accel_before_prepass(srt_tracer *t, const ScenePrep &sp); /* SRT_BUILD_DEVICE: the order of the models this upload builds */
int srt_accel_behind_prepass(srt_tracer *t, const ScenePrep &sp); /* SRT_REFIT_DEVICE: new boxes, the deform cost, then the built order starts its way back */
/* srt_texture.hip: the setters' data checked against a scene that is about to be uploaded; the plane frames and triangle count of the scene being uploaded (srt_update_scene, every group member);
 * checking the setters' data against the current scene and bringing the device tables up to date (after srt_update_scene
 * and before every dispatch; sets tex_active); the tables as the textured kernels take them; freeing them */
int srt_texture_check_scene(srt_tracer *t, size_t n_triangles, size_t n_materials); /* before a scene with this many triangles and materials replaces the current one */
void srt_texture_scene(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, size_t n_triangles);
int srt_texture_sync(srt_tracer *t);
TexParams srt_texture_params(const srt_tracer *t);
void srt_texture_release(srt_tracer *t);
/* THE place a textured kernel's parameter block is made (Tex = TexTraceParams / TexFeatureParams over Base = TraceParams /
 * FeatureParams): zeroed, padding included (what a kernel is handed is compared byte for byte), then the untextured
 * kernel's parameters, then the texture tables */
template <class Tex, class Base>
static inline Tex srt_with_textures(const srt_tracer *t, const Base &base) {
	Tex x;
	memset(&x, 0, sizeof x);
	static_cast<Base &>(x) = base;
	x.tx = srt_texture_params(t);
	return x;
}
/* denoise.hip: zero the denoiser's accumulations and counts (enqueued); after a dispatch's reductions, the feature pass of
 * that dispatch (p: its TraceParams as srt_trace_fused's last batch left them -- a dispatch without samples has no batch: the
 * batch's fields, radiance and queue among them, are zero, and no feature kernel is launched; else one launch of the kernel
 * last_trace_textured and dn.object_motion choose) and the counts; the filter over the canvas into argb (device, width*height*4 bytes) */
int srt_denoise_clear(srt_tracer *t);
int srt_denoise_after_trace(srt_tracer *t, const TraceParams &p, int num_samples);
int srt_denoise_filter(srt_tracer *t, uint32_t ticks_stopped, uint8_t *argb);
/* a clear that has to make the staging set itself under the history feedback (temporal.hip srt_temporal_commit, plan_filter's feedback):
 * the filter's front -- set-up, demodulate and spatial-variance launches, pass 1 in its feedback form -- without an ARGB image;
 * the filter's images hold no filter result afterwards */
int srt_denoise_feedback_front(srt_tracer *t);
/* the counts of one dispatch of `rd` (T, P, F, the camera) added to t's: srt_denoise_after_trace's, and what a group keeps on
 * its resolver handle for the dispatch all members have just run */
void srt_denoise_count(srt_tracer *t, const srt_render_data &rd, int feature_samples);
/* group denoiser, a group's way to its members (the public srt_set_denoise refuses a partitioned handle): feature_samples > 0
 * turns the member's accumulation on (allocates gd_pack for the current partition, binds the canvas into it, zeroes all of it),
 * 0 turns it off (the canvas rows go back to the buffer bound before) */
int srt_denoise_member(srt_tracer *t, int feature_samples);
/* the bytes srt_update_scene compares two scenes by (the denoiser's history survives an unchanged scene) */
void srt_scene_bytes(std::vector<uint8_t> &bytes, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                     const srt_material *materials, size_t n_materials, const srt_scene_data *scene);
/* temporal.hip: the temporal set-up over the canvas into `col` (and argb when not NULL), *staged = what it wrote into the
 * staging set (the guide the passes filter with; {c, count} and {m1, m2} for the spatial variance estimate);
 * the commit at srt_clear_canvas (before the canvas is zeroed); dropping the history */
struct TemporalStaged {
	const float4 *guide; // 2 float4 per pixel
	const float4 *cc;    // {colour, min(n, history_limit)}
	const float2 *m;     // {m1, m2}
};
int srt_temporal_setup(srt_tracer *t, float4 *col, uint32_t *argb, TemporalStaged *staged);
int srt_temporal_commit(srt_tracer *t);
void srt_temporal_drop(srt_tracer *t);
/* srt_update_scene with object motion on (`bytes`: the new scene, scene_bytes still the previous call's; rc: the update's
 * result): keeps or drops the history and rebuilds the motion table */
int srt_motion_update_scene(srt_tracer *t, const std::vector<uint8_t> &bytes, int rc);
/* per-triangle motion, before a feature pass: the frame's world-vertex table, written when the scene has changed since */
int srt_vertex_table_sync(srt_tracer *t);
/* exposure.hip, behind a site's own resolve into `argb`: with exposure on, the metering (AUTO) and the exposed resolve of the
 * w x h float4 of `source` / divisor over the same image, on the handle's stream; with bloom on and `picture` (the rows are a
 * picture's, not the interleaved blocks a partitioned handle owns), bloom.hip's launches, whose composite takes the exposed
 * resolve's place; both off: nothing. Sets last_exposed and last_bloomed. */
int srt_exposure_apply(srt_tracer *t, const float *source, float divisor, uint32_t w, uint32_t h, bool picture, uint8_t *argb);
/* ... for the render calls, whose frame is the canvas or, with the handle's denoiser on, the filter's image (divided already) */
static inline int srt_exposure_apply_frame(srt_tracer *t, uint32_t ticks_stopped, uint8_t *argb) {
	if (t->dn.on && t->dn_filtered)
		return srt_exposure_apply(t, t->dn_col.ptr + (size_t)t->dn_out * full_pixels(t) * 4, 1.0f, (uint32_t)t->width, (uint32_t)t->height, true, argb);
	return srt_exposure_apply(t, t->canvas, (float)ticks_stopped, (uint32_t)t->width, (uint32_t)t->owned_rows, t->world == 1, argb);
}
/* noise_meter.hip, behind a picture-producing site's resolve (srt_render, srt_render_async, srt_render_pipelined): with the meter
 * on, the handle meterable and dn_T a multiple of check_every, one metering on the handle's stream; else nothing. Sets last_ran. */
int srt_noise_after_resolve(srt_tracer *t);
/* ... and the metering itself: zero the record, the kernel over the canvas and the moments (view_argb not NULL: the heat map
 * into it as well), the record's copy into the next pinned slot behind its event. The caller has checked the state. */
int srt_noise_meter_enqueue(srt_tracer *t, uint8_t *view_argb);
/* selection.hip, the last step on a site's bytes (behind srt_exposure_apply): with a selection set, `picture` and a dispatch
 * behind the handle whose scene the selection names, the ID pass when the planes' key differs, then the outline kernel over the
 * w x h words of `argb`, on the handle's stream; else nothing. Sets last_applied and last_id_ran. */
int srt_selection_apply(srt_tracer *t, uint32_t w, uint32_t h, bool picture, uint8_t *argb);
/* ... for the render calls, whose frame is the handle's rows or, with its denoiser on, the filter's full image */
static inline int srt_selection_apply_frame(srt_tracer *t, uint8_t *argb) {
	if (t->dn.on && t->dn_filtered) return srt_selection_apply(t, (uint32_t)t->width, (uint32_t)t->height, true, argb);
	return srt_selection_apply(t, (uint32_t)t->width, (uint32_t)t->owned_rows, t->world == 1, argb);
}
/* ... for area.hip: the handle's ID planes brought up to date for its own scene under rd's camera and frame, by the overlay's
 * key -- planes made under an equal key are kept and nothing is launched; *ran = whether the pass was enqueued. rd is checked
 * as srt_render_ids checks it */
int srt_selection_ids_current(srt_tracer *t, const srt_render_data *rd, bool *ran);
/* area.hip for area_through.hip, which counts by other kernels into the same result buffers (t->ar), on the handle's stream:
 * the span's start and the clear of summary (8 words) and counts (n words; one_block: one allocation, the summary first); behind
 * the counting launches srt_area_finish_kernel over counts[0 .. n_counts) (launched: there were any) and the span's end; a
 * blocking call's frame -- the handle's buffer reserved, enqueue(d_counts, d_summary), one copy back through pinned memory;
 * the triangle count of a model shape (SRT_ERR_INVALID: beyond the scene, or no model; reads the uploaded record, blocking);
 * srt_select_area's rule applied to counts that are on the host */
int srt_area_clear(srt_tracer *t, uint32_t *counts, size_t n, uint32_t *summary, bool one_block);
int srt_area_finish(srt_tracer *t, const uint32_t *counts, uint32_t n_counts, uint32_t *summary, bool launched);
template <class Enqueue>
static inline int srt_area_result_host(srt_tracer *t, uint32_t n_counts, uint32_t *counts, srt_area_summary *out, Enqueue enqueue) {
	AreaState &ar = t->ar;
	const size_t words = 8 + (size_t)n_counts;
	if (ar.out.cap < words || ar.back.cap < words) { // (a grown buffer replaces one a queued launch may still use)
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		SRT_HIP(t, ar.out.reserve(words));
	}
	SRT_HIP(t, ar.back.reserve(words));
	if (const int rc = enqueue(ar.out.ptr + 8, ar.out.ptr)) return rc; // the counts, the summary
	SRT_HIP(t, ar.back.copy(ar.out.ptr, words, t->stream));
	SRT_HIP(t, ar.back.wait());
	memcpy(out, ar.back.host, sizeof *out);
	if (n_counts) memcpy(counts, ar.back.host + 8, (size_t)n_counts * sizeof(uint32_t));
	return SRT_OK;
}
int srt_area_model_triangles(srt_tracer *t, const char *who, uint32_t shape, uint32_t *n_triangles);
int srt_area_select_counts(srt_tracer *t, const uint32_t *counts, size_t n, int mode, uint32_t min_pixels, size_t *n_selected);
/* bloom.hip: whether a site's resolve of num_pixels is bloomed (the feature on, a picture, not empty); sets last_bloomed */
bool srt_bloom_begin(srt_tracer *t, bool picture, size_t num_pixels);
/* ... and its launches on the handle's stream: the pyramid of (source / divisor) * *exposure (NULL: 1.0f) and the composite
 * over `argb` */
int srt_bloom_resolve(srt_tracer *t, const float *source, float divisor, const float *exposure, uint32_t w, uint32_t h, uint8_t *argb);
/* srt_trace whose last reduction also resolves into fused_argb (device, owned pixels x 4 bytes; NULL: plain srt_trace); with a
 * denoiser on, the feature pass and the filter (a group member on its own: the plain resolve) follow the reductions. A
 * sequence of file-local steps in srt_abi.hip; the arithmetic they share with the host unit check is trace_plan.h's */
extern "C" int srt_trace_fused(srt_tracer *t, const srt_render_data *options, uint8_t *fused_argb, uint32_t ticks_stopped);
/* srt_abi.hip: trace_params_of for a caller outside it (ray_query.hip) -- the scene buffers and camera set-up a dispatch of
 * `options` over the handle's current scene would be handed; the batch's fields stay zero */
TraceParams srt_trace_params_for_query(const srt_tracer *t, const srt_render_data *options);
/* ray_query.hip: srt_pick's ray set-up for a caller outside it (multi_hit.hip) -- srt_pick_rays_kernel over n points at xy_dev
 * into n srt_ray at rays_dev, enqueued on the handle's stream (the caller has checked `options` and set the device) */
int srt_enqueue_pick_rays(srt_tracer *t, const srt_render_data *options, const void *xy_dev, size_t n, void *rays_dev);
/* one scene for several handles: the host pass once (members[0]'s acceleration mode and hierarchy cache), the uploads of all
 * members enqueued before the first is waited for (srt_abi.hip; srt_group_update_scene). *failed_member = the member an error came from */
extern "C" int srt_update_scene_many(srt_tracer *const *members, size_t n_members, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles,
                          size_t n_triangles, const srt_material *materials, size_t n_materials, const srt_scene_data *scene, size_t *failed_member);

#endif
