// srt_abi.hip — host side of libsrt_hip.so: the C ABI of include/srt_abi.h over the kernels in kernels.hip. This is what replaces
// the boost.compute/OpenCL dispatch of the reference's Tracer (src/tracer.cpp:11-116). HIP runtime only: life cycle, scene upload,
// trace; the BVH's upkeep on the device around an upload's pre-pass and the srt_*acceleration* entry points are accel_device.hip's.
// What needs no device lives beside it: the BVH builder (bvh_host.cpp), the scene's host pass (scene_prep.cpp), the launch plan (trace_plan.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/srt_abi.h"
#include "detmath.h"
#include "device_types.h"

#include "scene_prep.h"
#include "srt_internal.h"
#include "trace_plan.h"

namespace {

thread_local std::string g_create_error;

int num_blocks(int height, int rpb) { return (height + rpb - 1) / rpb; }

int clear_canvas_impl(srt_tracer *t) {
	const int rc = srt_temporal_commit(t); // temporal.hip: the frame being cleared becomes the denoiser's history
	if (rc) return rc;
	// enqueue_fill_buffer with 0.0f over the whole canvas (src/tracer.cpp:98-101)
	SRT_HIP(t, hipMemsetAsync(t->canvas, 0, t->canvas_bytes, t->stream));
	if (t->dn.on) return srt_denoise_clear(t); // the denoiser's accumulations start again with the canvas
	return SRT_OK;
}

} // namespace

int srt_fail(srt_tracer *t, int code, const std::string &msg) {
	if (t) t->err = msg;
	else g_create_error = msg;
	return code;
}


void srt_scene_bytes(std::vector<uint8_t> &bytes, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                     const srt_material *materials, size_t n_materials, const srt_scene_data *scene) {
	const size_t nb[4] = {n_shapes * sizeof(srt_shape), n_triangles * sizeof(srt_triangle), n_materials * sizeof(srt_material), sizeof(srt_scene_data)};
	const void *src[4] = {shapes, triangles, materials, scene};
	bytes.resize(32 + nb[0] + nb[1] + nb[2] + nb[3]);
	memcpy(bytes.data(), nb, 32);
	size_t o = 32;
	for (int k = 0; k < 4; k++) {
		if (nb[k]) memcpy(bytes.data() + o, src[k], nb[k]);
		o += nb[k];
	}
}

extern "C" {

const char *srt_version(void) {
#ifdef SRT_DEV_KNOBS
	return "srt-hip 0.1 gfx950 parity (fp-contract=off, IEEE div/sqrt, detmath) [dev knobs]";
#else
	return "srt-hip 0.1 gfx950 parity (fp-contract=off, IEEE div/sqrt, detmath)";
#endif
}

const char *srt_last_error(const srt_tracer *t) { return t ? t->err.c_str() : g_create_error.c_str(); }

int srt_partition_owned_rows(int height, int rank, int world, int rpb) {
	if (height < 0 || world < 1 || rank < 0 || rank >= world || rpb < 1) return -1;
	int rows = 0;
	const int nb = num_blocks(height, rpb);
	for (int b = rank; b < nb; b += world) {
		int r = height - b * rpb;
		rows += r < rpb ? r : rpb;
	}
	return rows;
}

int srt_partition_padded_rows(int height, int world, int rpb) {
	if (height < 0 || world < 1 || rpb < 1) return -1;
	const int nb = num_blocks(height, rpb);
	return ((nb + world - 1) / world) * rpb;
}

int srt_partition_global_row(int height, int rank, int world, int rpb, int local_row) {
	if (height < 0 || world < 1 || rank < 0 || rank >= world || rpb < 1 || local_row < 0) return -1;
	const int lb = local_row / rpb;
	const int y = (lb * world + rank) * rpb + (local_row - lb * rpb);
	return y < height ? y : -1;
}

int srt_partition_unpermute(const void *gathered, void *image, int height, int world, int rpb, size_t row_bytes) {
	if (!gathered || !image || height < 0 || world < 1 || rpb < 1) return SRT_ERR_INVALID;
	const int padded = srt_partition_padded_rows(height, world, rpb);
	const char *src = static_cast<const char *>(gathered);
	char *dst = static_cast<char *>(image);
	for (int r = 0; r < world; r++) {
		for (int lr = 0; lr < padded; lr++) {
			const int y = srt_partition_global_row(height, r, world, rpb, lr);
			if (y < 0) continue;
			memcpy(dst + (size_t)y * row_bytes, src + ((size_t)r * padded + lr) * row_bytes, row_bytes);
		}
	}
	return SRT_OK;
}

// Development knobs (scheduling experiments and tests that force rare paths: SRT_WAVES_PER_CU, SRT_SCAN_PAIRS, SRT_JOB_CAP_SUBS,
// SRT_ITEMS_PER_WAVE, SRT_FORCE_BATCH, SRT_POOL_BLOCKS, SRT_NO_SCAN_POOL) are read from the environment by -DSRT_DEV_KNOBS builds only (build.py build_dev():
// lib/variants/dev/). The product library's scheduling does not depend on the caller's environment.
#ifdef SRT_DEV_KNOBS
static const char *dev_env(const char *name) { return getenv(name); }
#else
static const char *dev_env(const char *) { return nullptr; }
#endif
static int dev_int(const char *name) { // a knob that is a count: 0 = not set
	const char *env = dev_env(name);
	return env ? atoi(env) : 0;
}

int srt_create(int width, int height, int device_index, srt_tracer **out) {
	if (!out) return fail(nullptr, SRT_ERR_INVALID, "srt_create: out is NULL");
	*out = nullptr;
	if (width <= 0 || height <= 0) return fail(nullptr, SRT_ERR_INVALID, "srt_create: width and height must be positive");
	if ((uint64_t)width * (uint64_t)height >= (1ull << 31))
		return fail(nullptr, SRT_ERR_INVALID, "srt_create: width * height must stay below 2^31 pixels (the kernel's pixel id is 32-bit, as in render.cl:488)");
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0)
		return fail(nullptr, SRT_ERR_HIP, std::string("srt_create: no HIP device (") + hipGetErrorString(e) + ")");
	if (device_index < 0 || device_index >= ndev) return fail(nullptr, SRT_ERR_INVALID, "srt_create: device_index out of range");
	srt_tracer *t = new (std::nothrow) srt_tracer();
	if (!t) return fail(nullptr, SRT_ERR_INVALID, "srt_create: out of host memory");
	t->width = width;
	t->height = height;
	t->device = device_index;
	t->owned_rows = height;
	if (const char *env = getenv("SRT_RADIANCE_BUDGET_MB")) { // the one environment variable a deployment may want: read here, once
		const long long mb = atoll(env);
		if (mb > 0) t->radiance_budget_env = (size_t)mb << 20;
	}
	auto bail = [&](const char *what, hipError_t err) {
		std::string m = std::string("srt_create: ") + what + ": " + hipGetErrorString(err);
		srt_destroy(t);
		return fail(nullptr, SRT_ERR_HIP, m);
	};
	if ((e = hipSetDevice(device_index)) != hipSuccess) return bail("hipSetDevice", e);
	if ((e = hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
	{
		hipDeviceProp_t prop;
		if ((e = hipGetDeviceProperties(&prop, device_index)) != hipSuccess) return bail("hipGetDeviceProperties", e);
		t->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	}
	t->stream = t->own_stream;
	const size_t px = (size_t)width * height;
	if ((e = t->canvas_own.reserve(px * 4)) != hipSuccess) return bail("canvas alloc", e);
	t->canvas = t->canvas_own.ptr;
	t->canvas_bytes = px * 16;
	if ((e = t->argb.reserve(px * 4)) != hipSuccess) return bail("argb alloc", e);
	if ((e = t->counters.reserve(SRT_CTR_COUNT)) != hipSuccess) return bail("counter alloc", e);
	if ((e = t->wave_counters.reserve((size_t)2 * SRT_WAVE_CTR_SLOTS * SRT_WAVE_CTR_STRIDE)) != hipSuccess) return bail("counter alloc", e);
	if ((e = t->shapes.reserve(1)) != hipSuccess || (e = t->runs.reserve(1)) != hipSuccess ||
	    (e = t->run_data.reserve(32)) != hipSuccess || (e = t->winners.reserve(1)) != hipSuccess ||
	    (e = t->triangles.reserve(1)) != hipSuccess || (e = t->materials.reserve(1)) != hipSuccess ||
	    (e = t->wtris.reserve(SRT_WTRI_FLOATS + 64)) != hipSuccess || (e = t->wtri_offset.reserve(1)) != hipSuccess)
		return bail("scene alloc", e);
	if ((e = hipEventCreate(&t->ev_t0)) != hipSuccess || (e = hipEventCreate(&t->ev_t1)) != hipSuccess ||
	    (e = hipEventCreate(&t->ev_r0)) != hipSuccess || (e = hipEventCreate(&t->ev_r1)) != hipSuccess)
		return bail("hipEventCreate", e);
	if ((e = hipMemsetAsync(t->canvas, 0, t->canvas_bytes, t->stream)) != hipSuccess) return bail("canvas clear", e);
	if ((e = hipMemsetAsync(t->wave_counters.ptr, 0, (size_t)2 * SRT_WAVE_CTR_SLOTS * SRT_WAVE_CTR_STRIDE * sizeof(unsigned long long), t->stream)) != hipSuccess)
		return bail("counter clear", e);
	if ((e = hipMemsetAsync(t->counters.ptr, 0, SRT_CTR_COUNT * sizeof(unsigned long long), t->stream)) != hipSuccess)
		return bail("counter clear", e);
	if ((e = hipStreamSynchronize(t->stream)) != hipSuccess) return bail("sync", e);
	*out = t;
	return SRT_OK;
}

void srt_destroy(srt_tracer *t) {
	if (!t) return;
	(void)hipSetDevice(t->device);
	if (t->own_stream) (void)hipStreamSynchronize(t->own_stream);
	srt_collect_release(t);
	srt_pipeline_release(t);
	t->canvas_own.release();
	t->gd_pack.release();
	t->argb.release();
	t->shapes.release();
	t->runs.release();
	t->run_data.release();
	t->winners.release();
	t->triangles.release();
	t->materials.release();
	t->wtris.release();
	t->wtri_offset.release();
	t->bvh_blocks.release();
	t->bvh_order.release();
	t->bvh_dest.release();
	t->upkeep.release();
	t->sky.release();
	t->counters.release();
	t->wave_counters.release();
	t->scan_queue.release();
	t->radiance.release();
	t->running.release();
	t->dn_nd.release();
	t->dn_ah.release();
	t->dn_mom.release();
	t->dn_guide.release();
	t->dn_col.release();
	t->tp_set[0].release();
	t->tp_set[1].release();
	t->tp_bounds.release();
	t->om_ids[0].release();
	t->om_ids[1].release();
	t->om_table_dev.release();
	for (int k = 0; k < 2; k++) t->vm_tri[k].release(), t->vm_rows[k].release();
	t->vm_first_dev.release();
	t->ex_own.record.release();
	t->bl_own.pyramid.release();
	t->nz_own.release();
	t->sel_own.release();
	t->rq_stage.release();
	t->rq_span.release();
	t->ao.release();
	t->ar.release();
	srt_texture_release(t);
	if (t->ev_t0) (void)hipEventDestroy(t->ev_t0);
	if (t->ev_t1) (void)hipEventDestroy(t->ev_t1);
	if (t->ev_r0) (void)hipEventDestroy(t->ev_r0);
	if (t->ev_r1) (void)hipEventDestroy(t->ev_r1);
	for (hipEvent_t ev : t->ev_k) (void)hipEventDestroy(ev);
	for (int k = 0; k < 2; k++) {
		if (t->ev_batch_traced[k]) (void)hipEventDestroy(t->ev_batch_traced[k]);
		if (t->ev_batch_reduced[k]) (void)hipEventDestroy(t->ev_batch_reduced[k]);
		if (t->batch_stream[k]) (void)hipStreamDestroy(t->batch_stream[k]);
	}
	if (t->ev_batch_fork) (void)hipEventDestroy(t->ev_batch_fork);
	if (t->own_stream) (void)hipStreamDestroy(t->own_stream);
	delete t->bvh_cache;
	delete t;
}

int srt_set_skybox(srt_tracer *t, const float *rgba, int width, int height) {
	if (!t) return SRT_ERR_INVALID;
	if (!rgba || width <= 0 || height <= 0) return fail(t, SRT_ERR_INVALID, "srt_set_skybox: bad image");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t n = (size_t)width * height * 4;
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // kernels may still read the old image
	SRT_HIP(t, t->sky.reserve(n));
	SRT_HIP(t, hipMemcpyAsync(t->sky.ptr, rgba, n * sizeof(float), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	t->sky_w = width;
	t->sky_h = height;
	srt_temporal_drop(t); // the denoiser's history saw the old sky
	return SRT_OK;
}

static int update_scene_impl(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                             const srt_material *materials, size_t n_materials, const srt_scene_data *scene);

int srt_update_scene(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles,
                     size_t n_triangles, const srt_material *materials, size_t n_materials,
                     const srt_scene_data *scene) {
	// the host pass allocates (std::vector): no C++ exception may cross the C ABI
	try {
		// the denoiser's history (temporal.hip) survives only a call with the same bytes as the previous one: the front-end
		// calls this after every clear, and without object motion vectors a moved or edited object starts from scratch
		std::vector<uint8_t> bytes;
		if (t && scene) srt_scene_bytes(bytes, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
		const int rc = update_scene_impl(t, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
		if (t && t->dn.object_motion) { // temporal.hip: object motion compares with the history's scene and keeps what only moved
			const int mrc = srt_motion_update_scene(t, bytes, rc);
			if (rc == SRT_OK && mrc != SRT_OK) {
				t->scene_bytes.swap(bytes);
				return mrc;
			}
		} else if (t && (rc != SRT_OK || bytes.empty() || bytes != t->scene_bytes)) srt_temporal_drop(t);
		if (t) t->scene_bytes.swap(bytes);
		return rc;
	} catch (const std::bad_alloc &) {
		if (t) t->err.clear(); // the message itself must not allocate much: a short literal fits the small-string buffer
		return t ? fail(t, SRT_ERR_INVALID, "out of host memory") : SRT_ERR_INVALID;
	} catch (...) {
		return SRT_ERR_INVALID;
	}
}

// device pass, first half: wait for the handle's previous launches, (re)allocate, enqueue every upload and the pre-pass on its stream
static int upload_scene_begin(srt_tracer *t, const ScenePrep &sp, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles,
                              size_t n_triangles, size_t n_materials) {
	const std::vector<BlockGroup> &groups = sp.groups;
	const std::vector<float> &data = sp.data;
	const std::vector<WinnerRec> &winners = sp.winners;
	const std::vector<uint32_t> &offs = sp.offs, &bvh_blocks = sp.bvh_blocks, &bvh_order = sp.bvh_order, &bvh_dest = sp.bvh_dest;
	const std::vector<srt_material> &dev_mats = sp.dev_mats;
	const bool use_bvh = sp.use_bvh;
	const uint64_t total_wtris = sp.total_wtris, max_tris = sp.max_tris;
	const int num_models = sp.num_models;
	if (const int trc = srt_texture_check_scene(t, n_triangles, n_materials)) return trc; // (before anything of the current scene is replaced)
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // previous launches may still read the old scene
	srt_texture_scene(t, shapes, n_shapes, n_triangles);
	SRT_HIP(t, t->shapes.reserve(n_shapes));
	SRT_HIP(t, t->runs.reserve(groups.size()));
	SRT_HIP(t, t->run_data.reserve(data.size()));
	SRT_HIP(t, t->winners.reserve(n_shapes));
	SRT_HIP(t, t->wtri_offset.reserve(n_shapes));
	SRT_HIP(t, t->triangles.reserve(n_triangles));
	SRT_HIP(t, t->materials.reserve(n_materials));
	if (use_bvh) {
		SRT_HIP(t, t->bvh_blocks.reserve(bvh_blocks.size()));
		SRT_HIP(t, t->bvh_order.reserve(bvh_order.size()));
		SRT_HIP(t, t->bvh_dest.reserve(bvh_dest.size()));
		if (!bvh_blocks.empty()) // inner blocks complete, leaf blocks zero: srt_prepass_kernel writes their triangles
			SRT_HIP(t, hipMemcpyAsync(t->bvh_blocks.ptr, bvh_blocks.data(), bvh_blocks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
		if (!bvh_order.empty()) {
			SRT_HIP(t, hipMemcpyAsync(t->bvh_order.ptr, bvh_order.data(), bvh_order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
			SRT_HIP(t, hipMemcpyAsync(t->bvh_dest.ptr, bvh_dest.data(), bvh_dest.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
		}
	} else {
		SRT_HIP(t, t->wtris.reserve((size_t)total_wtris * SRT_WTRI_FLOATS + 64)); // + slack for the loop's look-ahead pair
	}
	if (n_shapes) {
		SRT_HIP(t, hipMemcpyAsync(t->shapes.ptr, shapes, n_shapes * sizeof(srt_shape), hipMemcpyHostToDevice, t->stream));
		SRT_HIP(t, hipMemcpyAsync(t->winners.ptr, winners.data(), n_shapes * sizeof(WinnerRec), hipMemcpyHostToDevice, t->stream));
		SRT_HIP(t, hipMemcpyAsync(t->wtri_offset.ptr, offs.data(), n_shapes * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
	}
	if (!groups.empty())
		SRT_HIP(t, hipMemcpyAsync(t->runs.ptr, groups.data(), groups.size() * sizeof(BlockGroup), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipMemcpyAsync(t->run_data.ptr, data.data(), data.size() * sizeof(float), hipMemcpyHostToDevice, t->stream));
	if (n_triangles)
		SRT_HIP(t, hipMemcpyAsync(t->triangles.ptr, triangles, n_triangles * sizeof(srt_triangle), hipMemcpyHostToDevice, t->stream));
	if (n_materials)
		SRT_HIP(t, hipMemcpyAsync(t->materials.ptr, dev_mats.data(), n_materials * sizeof(srt_material), hipMemcpyHostToDevice, t->stream));

	if (const int brc = srt_accel_before_prepass(t, sp)) return brc; // accel_device.hip: SRT_BUILD_DEVICE sorts the order the pre-pass reads
	if (num_models > 0 && total_wtris > 0) {
		if (!use_bvh) SRT_HIP(t, hipMemsetAsync(t->wtris.ptr, 0, ((size_t)total_wtris * SRT_WTRI_FLOATS + 64) * sizeof(float), t->stream));
		// blockIdx.y = shape index; launch in slabs of 65535 shapes
		for (size_t base = 0; base < n_shapes; base += 65535) {
			PrepassParams pp;
			pp.shapes = t->shapes.ptr + base;
			pp.triangles = t->triangles.ptr;
			pp.wtri_offset = t->wtri_offset.ptr + base;
			pp.wtris = use_bvh ? reinterpret_cast<float *>(t->bvh_blocks.ptr) : t->wtris.ptr;
			pp.order = use_bvh ? t->bvh_order.ptr : nullptr;
			pp.dest = use_bvh ? t->bvh_dest.ptr : nullptr;
			size_t cnt = n_shapes - base;
			pp.num_shapes = (int32_t)(cnt > 65535 ? 65535 : cnt);
			pp.num_triangles = (uint32_t)n_triangles;
			srt_launch_prepass(pp, max_tris, t->stream);
		}
		SRT_HIP(t, hipGetLastError());
	}
	return srt_accel_behind_prepass(t, sp); // SRT_REFIT_DEVICE refits what the pre-pass wrote; the built order starts its way back
}

// device pass, second half: the uploads have arrived (the host arrays are free again), the handle describes the new scene
static int upload_scene_end(srt_tracer *t, const ScenePrep &sp, size_t n_shapes, size_t n_materials, const srt_scene_data *scene) {
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	t->sd = *scene;
	t->sd.num_shapes = (int32_t)n_shapes; // src/tracer.cpp:94
	t->num_models = sp.num_models;
	t->scan_tris = sp.use_bvh ? 0 : sp.total_wtris;
	t->bvh_active = sp.use_bvh && sp.num_models > 0;
	t->bvh_num_blocks = sp.use_bvh ? sp.bvh_blocks.size() / 32 : 0;
	for (int k = 0; k < 7; k++) t->bvh_info[k] = sp.bvh_info[k];
	t->all_materials_ok = sp.all_materials_ok;
	t->unit_materials = sp.unit_materials;
	t->material_flags = sp.material_flags;
	t->one_group_code = sp.one_group_code;
	t->plane_axes = sp.plane_axes;
	t->num_runs = (int)sp.groups.size();
	t->num_materials = n_materials;
	t->scene_set = true;
	t->scene_rev++; // selection.hip: ID planes of the previous scene are stale
	return srt_texture_sync(t); // albedo textures: bindings and UVs are checked against the new scene
}

// the host pass (scene_prep.cpp) with `t`'s acceleration mode and hierarchy cache (a group: its first member's)
static int prepare_scene_of(srt_tracer *t, ScenePrep &sp, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                            const srt_material *materials, size_t n_materials, const srt_scene_data *scene) {
	std::string err;
	if (const int crc = srt_accel_deform_consume(t, t->bvh_cache)) return crc; // the rebuild rule looks at the last known cost ratios
	if (const int brc = srt_accel_build_consume(t, t->bvh_cache)) return brc;  // every entry's order is the sorted one
	const int rc = prepare_scene(t->policy, t->bvh_cache, srt_scan_suspend_min(), err, sp, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
	return rc == SRT_OK ? SRT_OK : fail(t, rc, err);
}

static int update_scene_impl(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                             const srt_material *materials, size_t n_materials, const srt_scene_data *scene) {
	if (!t) return SRT_ERR_INVALID;
	ScenePrep sp;
	int rc = prepare_scene_of(t, sp, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
	if (rc == SRT_OK) rc = upload_scene_begin(t, sp, shapes, n_shapes, triangles, n_triangles, n_materials);
	if (rc == SRT_OK) rc = upload_scene_end(t, sp, n_shapes, n_materials, scene);
	return rc;
}

// One scene for N handles (srt_group_update_scene): prepared once with members[0]'s acceleration mode and hierarchy cache, uploaded to
// all of them -- every device's copies and pre-pass are enqueued before the first is waited for. On an error the members that
// were not reached keep their previous scene.
int srt_update_scene_many(srt_tracer *const *members, size_t n_members, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles,
                          size_t n_triangles, const srt_material *materials, size_t n_materials, const srt_scene_data *scene, size_t *failed_member) {
	if (failed_member) *failed_member = 0;
	if (!members || n_members == 0 || !members[0]) return SRT_ERR_INVALID;
	try {
		ScenePrep sp;
		int rc = prepare_scene_of(members[0], sp, shapes, n_shapes, triangles, n_triangles, materials, n_materials, scene);
		if (rc != SRT_OK) return rc;
		size_t begun = 0;
		for (; begun < n_members && rc == SRT_OK; begun++) {
			if (failed_member) *failed_member = begun;
			members[begun]->policy = members[0]->policy; // (the prepared scene is in this form)
			rc = upload_scene_begin(members[begun], sp, shapes, n_shapes, triangles, n_triangles, n_materials);
		}
		if (rc != SRT_OK) { // what was enqueued on the members before the failing one still reads the host arrays: let it finish
			for (size_t i = 0; i + 1 < begun; i++) (void)upload_scene_end(members[i], sp, n_shapes, n_materials, scene);
			return rc;
		}
		for (size_t i = 0; i < n_members; i++) {
			if (failed_member) *failed_member = i;
			const int r = upload_scene_end(members[i], sp, n_shapes, n_materials, scene);
			if (r != SRT_OK && rc == SRT_OK) rc = r;
		}
		return rc;
	} catch (const std::bad_alloc &) {
		return fail(members[0], SRT_ERR_INVALID, "out of host memory");
	} catch (...) {
		return SRT_ERR_INVALID;
	}
}

int srt_clear_canvas(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	return clear_canvas_impl(t);
}

// THE scene-class predicate: which instantiation of the sphere / plane trace kernel a dispatch of `options` over the handle's
// scene starts (device_types.h SRT_SCENE_CLASS_LIST; 0 = the general kernel). Host data only: what srt_update_scene found
// of the scene, and the options of this dispatch. A class needs all of: no models, one block group over all shapes, the scene
// records staged in LDS, every shape with a material, material probabilities as thresholds, bounces, no show_normals, no
// textures, no triangle counting, and a build that holds the classes (kernels.hip SRT_SCENE_CLASSES: sky ring of 64, no instruments).
static int scene_class(const srt_tracer *t, const srt_render_data *options, bool textured) {
	if (!srt_trace_has_scene_classes()) return SRT_SCENE_CLASS_GENERAL;
	if (!t->scene_set || t->num_models != 0 || t->num_runs != 1 || t->one_group_code == 0) return SRT_SCENE_CLASS_GENERAL;
	if (srt_scene_lds_bytes((size_t)t->sd.num_shapes, t->num_materials, 0, 1) == 0) return SRT_SCENE_CLASS_GENERAL;
	if (!t->all_materials_ok || !t->unit_materials) return SRT_SCENE_CLASS_GENERAL;
	if (options->num_bounces <= 0 || options->show_normals || textured || t->count_tris) return SRT_SCENE_CLASS_GENERAL;
	const bool no_spec = (t->material_flags & (SRT_MF_NO_SPECULAR | SRT_MF_PLAIN_COLORS)) == (SRT_MF_NO_SPECULAR | SRT_MF_PLAIN_COLORS);
#define SRT_SCENE_CLASS_MATCH(number, code, class_no_spec) \
	if (t->one_group_code == (code) && no_spec == class_no_spec) return number;
	SRT_SCENE_CLASS_LIST(SRT_SCENE_CLASS_MATCH)
#undef SRT_SCENE_CLASS_MATCH
	return SRT_SCENE_CLASS_GENERAL;
}

// Which twin of a class a launch runs: the scene's plane form when the class has an axis twin for exactly that pattern
// (device_types.h SRT_SCENE_AXIS_LIST), else 0, the class's own kernel. The class is decided first and by scene_class() alone.
static uint32_t plane_form_of(const srt_tracer *t, int scene_class) {
#define SRT_SCENE_AXIS_MATCH(number, code, class_no_spec, axes) \
	if (scene_class == number && t->plane_axes == (axes)) return axes;
	SRT_SCENE_AXIS_LIST(SRT_SCENE_AXIS_MATCH)
#undef SRT_SCENE_AXIS_MATCH
	return 0u;
}

int srt_last_trace_class(const srt_tracer *t, int *scene_class_out) {
	if (!t || !scene_class_out) return SRT_ERR_INVALID;
	*scene_class_out = t->last_trace_class;
	return SRT_OK;
}

int srt_last_trace_plane_form(const srt_tracer *t, int *plane_form_out) {
	if (!t || !plane_form_out) return SRT_ERR_INVALID;
	*plane_form_out = (int)t->last_trace_plane_form;
	return SRT_OK;
}

int srt_trace(srt_tracer *t, const srt_render_data *options) { return srt_trace_fused(t, options, nullptr, 0u); }

// ---- the steps of a dispatch (srt_trace_fused below runs them in this order) ------------------------------------------------

// What the steps hand to each other, on srt_trace_fused's stack (value-initialised there). The two parameter blocks travel beside
// it: the TraceParams (trace_params_of; launch_batch fills the batch's fields in place) and the ReduceParams (reduce_params_of).
struct Dispatch {
	bool textured, timed, denoise;
	size_t pixels; // owned
	int ns;        // options->num_samples
	uint8_t *fused_argb;
	uint32_t batch, n_batches; // reserve_radiance, with radiance_stride
	size_t radiance_stride;
	int slots;              // resident waves of the device for this launch configuration (wave_slots)
	bool scan_queue;        // reserve_scan_stacks: array scan, the launches get scan stacks, scan_set_floats per set
	size_t scan_set_floats;
	uint32_t pool_blocks;
};

// num_pixels of `canvas` through the tone map into `argb`, on the handle's stream
static int launch_resolve(srt_tracer *t, const float *canvas, uint32_t num_pixels, uint32_t ticks_stopped, uint8_t *argb) {
	ResolveParams rp;
	rp.canvas = canvas;
	rp.argb = argb;
	rp.num_steps = ticks_stopped;
	rp.num_pixels = num_pixels;
	srt_launch_resolve(rp, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

// The TraceParams that the handle and the options decide: everything but the batch's buffers, cursor, samples and chunks
// (launch_batch). No side effects.
static TraceParams trace_params_of(const srt_tracer *t, const srt_render_data *options, bool textured) {
	TraceParams p;
	memset(&p, 0, sizeof p);
	p.rd = *options;
	if (t->scene_set) {
		p.sd = t->sd;
	} else {
		memset(&p.sd, 0, sizeof p.sd); // kernel arg 1 never set: behave as the empty scene
	}
	p.runs = t->runs.ptr;
	p.run_data = t->run_data.ptr;
	p.winners = t->winners.ptr;
	p.num_runs = t->scene_set ? t->num_runs : 0;
	p.num_materials = t->scene_set ? (int32_t)t->num_materials : 0;
	p.shapes = t->shapes.ptr;
	p.triangles = t->triangles.ptr;
	p.materials = t->materials.ptr;
	p.wtris = t->wtris.ptr;
	p.sky = t->sky.ptr;
	p.canvas = t->canvas;
	p.counters = t->counters.ptr;
	p.wave_counters = t->wave_counters.ptr;
	p.sky_w = t->sky_w;
	p.sky_h = t->sky_h;
	p.f_width = (float)options->width;
	p.f_height = (float)options->height;
	p.inv_f_width = 1.0f / p.f_width; // IEEE quotients: the kernel's camera rays divide by multiplying with them (device_math.h div_by_rcp)
	p.inv_f_height = 1.0f / p.f_height;
	srt_magic_u31(options->width > 0 ? (uint32_t)options->width : 1u, &p.width_magic, &p.width_shift);
	srt_magic_u31(t->rows_per_block > 0 ? (uint32_t)t->rows_per_block : 1u, &p.rpb_magic, &p.rpb_shift);
	p.all_materials_ok = t->scene_set && t->all_materials_ok ? 1 : 0;
	p.unit_materials = t->scene_set && t->unit_materials ? 1 : 0;
	p.material_flags = t->scene_set ? t->material_flags : 0;
	{
		const int sc = scene_class(t, options, textured);
		p.scene_class = srt_kernel_key(sc, plane_form_of(t, sc));
	}
	p.f_sky_w = (float)t->sky_w;
	p.f_sky_h = (float)t->sky_h;
	p.sun_focus_int = dm_pow_small_int(p.sd.sun_focus);
	p.num_models = t->num_models;
	p.use_bvh = t->bvh_active ? 1 : 0;
	p.bvh_blocks = reinterpret_cast<const float *>(t->bvh_blocks.ptr);
	p.rank = t->rank;
	p.world = t->world;
	p.rows_per_block = t->rows_per_block;
	p.owned_rows = t->owned_rows;
	return p;
}

// the ReduceParams of a dispatch but for the batch's fields (launch_batch) and the moments / argb union (launch_reduce)
static ReduceParams reduce_params_of(const srt_tracer *t, const Dispatch &d, uint32_t ticks_stopped) {
	ReduceParams rp;
	rp.radiance = t->radiance.ptr;
	rp.running = t->running.ptr;
	rp.canvas = t->canvas;
	rp.counters = t->counters.ptr;
	rp.num_pixels = (uint32_t)d.pixels;
	rp.num_samples = d.ns;
	rp.queue_reset = nullptr;
	rp.argb = nullptr;
	rp.num_steps = ticks_stopped;
	return rp;
}

// With the denoiser on, the reductions also collect the per-pixel moments and the render calls resolve through the filter
// after the feature pass (denoise_tail), so no reduction resolves.
// A member of a group whose denoiser is on (gd_on) does the same for its own rows; the group's resolver handle filters.
static void launch_reduce(srt_tracer *t, ReduceParams &rp, bool denoise, uint8_t *argb) {
	if (denoise) {
		rp.moments = t->gd_on ? gd_moments(t) : t->dn_mom.ptr;
		srt_launch_reduce_moments(rp, t->stream);
	} else {
		rp.argb = argb;
		srt_launch_reduce(rp, t->stream);
	}
}

// ---- batches of samples: radiance[pixel][sample] must fit the HBM budget ----------
// Chooses the budget (first use), plans the batch and allocates the radiance buffers -- two when there are several batches,
// and `running` with them --, falling back to smaller batches if the device cannot give that much right now. Fills d.batch
// (samples per batch), d.n_batches and d.radiance_stride.
static int reserve_radiance(srt_tracer *t, Dispatch &d) {
	const size_t pixels = d.pixels;
	const int ns = d.ns;
	if (t->radiance_budget == 0) {
		size_t free_b = 0, total_b = 0;
		SRT_HIP(t, hipMemGetInfo(&free_b, &total_b));
		size_t budget = free_b / 2; // leave half of what is free to the caller
		const size_t cap = (size_t)96 << 30;
		if (budget > cap) budget = cap;
		if (t->radiance_budget_env) budget = t->radiance_budget_env; // SRT_RADIANCE_BUDGET_MB, read once by srt_create
		t->radiance_budget = budget;
	}
	const char *env_pairs = dev_env("SRT_SCAN_PAIRS");
	uint32_t batch = plan_batch(pixels, ns, t->radiance_budget, t->scan_tris, env_pairs ? atof(env_pairs) : 0.0, dev_int("SRT_FORCE_BATCH"));
	// allocate; if the device cannot give that much right now, fall back to smaller batches
	while (batch) {
		const size_t buffers = batch < (uint32_t)ns ? 2 : 1;
		hipError_t e = t->radiance.reserve(buffers * plan_radiance_stride(pixels, batch)); // each buffer a whole number of 16-byte units
		if (e == hipSuccess) break;
		(void)hipGetLastError(); // clear the sticky out-of-memory state
		if (e != hipErrorOutOfMemory || batch == 1)
			return fail(t, SRT_ERR_HIP, std::string("srt_trace: radiance buffer: ") + hipGetErrorString(e));
		batch = plan_batch_halved(batch);
		t->radiance_budget = pixels * 12 * (size_t)batch;
	}
	d.batch = batch;
	d.n_batches = plan_num_batches(ns, batch);
	d.radiance_stride = plan_radiance_stride(pixels, batch);
	if (d.n_batches > 1) SRT_HIP(t, t->running.reserve(pixels * 4));
	return SRT_OK;
}

// resident waves of the device for this dispatch's kernel: one counter line per persistent wave
static int wave_slots(srt_tracer *t, const TraceParams &p, bool textured) {
	int per_cu = textured ? srt_trace_tex_resident_waves_per_cu(srt_with_textures<TexTraceParams>(t, p), t->count_tris) : srt_trace_resident_waves_per_cu(p, t->count_tris);
	if (const char *env = dev_env("SRT_WAVES_PER_CU")) {
		const int v = atoi(env);
		if (v > 0 && v < per_cu) per_cu = v;
	}
	t->last_waves_per_cu = per_cu;
	const int slots = t->num_cus * per_cu;
	return slots > SRT_WAVE_CTR_SLOTS ? SRT_WAVE_CTR_SLOTS : slots;
}

// Array scan: one block of scan / park stacks per persistent wave the largest launch of this dispatch starts (46 KB each),
// the launch-end ray pool's records (84 MB), and a second set of both only when sample batches overlap: 320 MB for a
// one-launch frame on 256 CUs, 640 MB for an overlapped one. If the device cannot give that, the
// dispatch runs without the pool (every wave scans its own remainder: slower tails, same canvas) before it fails.
// Fills d.scan_queue, d.scan_set_floats and d.pool_blocks.
static int reserve_scan_stacks(srt_tracer *t, Dispatch &d) {
	d.scan_queue = t->num_models > 0 && !t->bvh_active;
	const size_t scan_waves = plan_scan_waves(d.slots, d.pixels, d.batch);
	d.pool_blocks = d.scan_queue && !dev_env("SRT_NO_SCAN_POOL") ? (uint32_t)SRT_POOL_BLOCKS : 0u;
	if (const char *env = dev_env("SRT_POOL_BLOCKS")) { // tests: a pool that overflows
		const int v = atoi(env);
		if (v >= 0 && (uint32_t)v < d.pool_blocks) d.pool_blocks = (uint32_t)v;
	}
	if (d.scan_queue) {
		const size_t sets = d.n_batches > 1 ? 2 : 1;
		hipError_t e = t->scan_queue.reserve(sets * SRT_SCAN_SET_FLOATS(scan_waves, d.pool_blocks != 0u));
		if (e == hipErrorOutOfMemory && d.pool_blocks != 0u) {
			(void)hipGetLastError();
			d.pool_blocks = 0u;
			e = t->scan_queue.reserve(sets * SRT_SCAN_SET_FLOATS(scan_waves, false));
		}
		if (e != hipSuccess) {
			(void)hipGetLastError();
			return fail(t, SRT_ERR_HIP, std::string("srt_trace: scan stacks: ") + hipGetErrorString(e));
		}
	}
	d.scan_set_floats = SRT_SCAN_SET_FLOATS(scan_waves, d.pool_blocks != 0u);
	return SRT_OK;
}

// one pair of timer events per sample batch (srt_last_trace_kernel_ms)
static int reserve_timer_events(srt_tracer *t, uint32_t n_batches) {
	while (t->ev_k.size() < 2 * (size_t)n_batches) { // std::vector growth is the only throwing step: srt_trace's callers catch nothing
		hipEvent_t ev = nullptr;
		SRT_HIP(t, hipEventCreate(&ev));
		try {
			t->ev_k.push_back(ev);
		} catch (...) {
			(void)hipEventDestroy(ev);
			return fail(t, SRT_ERR_INVALID, "out of host memory");
		}
	}
	return SRT_OK;
}

// Several sample batches: even and odd batches trace on two streams of their own, each into its own radiance buffer,
// work cursor and set of per-wave counter lines, so that the tail of a batch (its last long paths, a few lanes per wave
// and most waves gone: half of a launch of the 10^5-triangle array scan) runs under the next batch instead of leaving
// the GPU idle. The ordered reductions stay on the caller's stream, in batch order; a batch's trace waits for the
// reduction that last read its buffer (launch_batch). Here: the streams and events, made when first needed, and the fork.
static int fork_batch_streams(srt_tracer *t) {
	for (int k = 0; k < 2; k++) {
		if (!t->batch_stream[k]) {
			// The two streams must not share a hardware queue, or the batches they carry run one after the other: the runtime
			// deals its few queues out to streams as they are created, and in a process that holds other streams (bench.py:
			// torch's, the headline handle's) both of these landed on one -- configs[4] 5.5 s instead of 4.3 s. Streams of
			// different priority never share a queue, so the odd batches' stream is created one level above the even ones'.
			int pr_low = 0, pr_high = 0;
			(void)hipDeviceGetStreamPriorityRange(&pr_low, &pr_high); // (numerically lower = higher priority)
			const int pr = (k == 1 && pr_high < pr_low) ? pr_low - 1 : pr_low;
			SRT_HIP(t, hipStreamCreateWithPriority(&t->batch_stream[k], hipStreamNonBlocking, pr));
		}
		if (!t->ev_batch_traced[k]) SRT_HIP(t, hipEventCreateWithFlags(&t->ev_batch_traced[k], hipEventDisableTiming));
		if (!t->ev_batch_reduced[k]) SRT_HIP(t, hipEventCreateWithFlags(&t->ev_batch_reduced[k], hipEventDisableTiming));
	}
	if (!t->ev_batch_fork) SRT_HIP(t, hipEventCreateWithFlags(&t->ev_batch_fork, hipEventDisableTiming));
	SRT_HIP(t, hipEventRecord(t->ev_batch_fork, t->stream)); // everything the caller's stream holds so far (scene upload, clear, ...)
	for (int k = 0; k < 2; k++) SRT_HIP(t, hipStreamWaitEvent(t->batch_stream[k], t->ev_batch_fork, 0));
	return SRT_OK;
}

// Batch b of the dispatch: its trace launch on the batch's stream, its ordered reduction on the handle's.
static int launch_batch(srt_tracer *t, const Dispatch &d, uint32_t b, TraceParams &p, ReduceParams &rp) {
	const bool overlap = d.n_batches > 1;
	const BatchSlice bs = plan_batch_slice(b, d.n_batches, d.pixels, d.ns, d.batch);
	const int par = bs.parity;
	hipStream_t ts = overlap ? t->batch_stream[par] : t->stream;
	p.radiance = t->radiance.ptr + (size_t)par * d.radiance_stride;
	p.queue = t->counters.ptr + (par ? SRT_CTR_QUEUE2 : SRT_CTR_QUEUE);
	p.wave_counters = t->wave_counters.ptr + (size_t)par * SRT_WAVE_CTR_SLOTS * SRT_WAVE_CTR_STRIDE;
	p.scan_queue = d.scan_queue ? t->scan_queue.ptr + (size_t)par * d.scan_set_floats : nullptr;
	p.pool_blocks = d.pool_blocks;
	if (overlap && b >= 2) SRT_HIP(t, hipStreamWaitEvent(ts, t->ev_batch_reduced[par], 0)); // batch b - 2 has been summed up
	p.batch_samples = bs.samples;
	p.first_sample = bs.first_sample;
	p.total_items = bs.total_items;
	const LaunchPlan lp = plan_launch(p.total_items, bs.samples, (unsigned long long)srt_sub_job_items(t->num_models > 0, t->bvh_active), t->num_cus, d.slots,
	                                  t->num_models > 0, t->bvh_active, dev_int("SRT_ITEMS_PER_WAVE"), dev_int("SRT_JOB_CAP_SUBS"));
	p.nbs_magic16 = lp.nbs_magic16;
	p.job_items = lp.job_items;
	// the work cursor is zero: the reduction behind the launch that used it last has reset it (srt_reduce_kernel). Only a launch
	// whose reduction was never enqueued (an error in between) leaves it dirty.
	if (t->queue_dirty[par]) SRT_HIP(t, hipMemsetAsync(p.queue, 0, sizeof(unsigned long long), ts));
	t->queue_dirty[par] = true;
	if (p.pool_blocks) SRT_HIP(t, hipMemsetAsync(p.scan_queue, 0, (size_t)SRT_POOL_CTL_WORDS * sizeof(uint32_t), ts));
	if (d.timed) SRT_HIP(t, hipEventRecord(t->ev_k[2 * b], ts));
	t->last_grid = lp.num_waves;
	if (d.textured) srt_launch_trace_tex(srt_with_textures<TexTraceParams>(t, p), t->count_tris, lp.num_waves, ts);
	else srt_launch_trace(p, t->count_tris, lp.num_waves, ts);
	SRT_HIP(t, hipGetLastError());
	if (d.timed) SRT_HIP(t, hipEventRecord(t->ev_k[2 * b + 1], ts));
	if (overlap) {
		SRT_HIP(t, hipEventRecord(t->ev_batch_traced[par], ts));
		SRT_HIP(t, hipStreamWaitEvent(t->stream, t->ev_batch_traced[par], 0));
	}
	t->ev_k_used = 2 * (size_t)(b + 1);
	rp.radiance = p.radiance;
	rp.batch_samples = bs.samples;
	rp.first_batch = (b == 0);
	rp.last_batch = (b == d.n_batches - 1);
	rp.queue_reset = p.queue;
	launch_reduce(t, rp, d.denoise, rp.last_batch ? d.fused_argb : nullptr);
	SRT_HIP(t, hipGetLastError());
	t->queue_dirty[par] = false; // (no pixels: neither launch ran, the cursor is untouched)
	if (overlap) SRT_HIP(t, hipEventRecord(t->ev_batch_reduced[par], t->stream));
	return SRT_OK;
}

// behind the reductions of a dispatch with a denoiser on: the feature pass, and for the render calls the filter
static int denoise_tail(srt_tracer *t, const Dispatch &d, const TraceParams &p, uint32_t ticks_stopped) {
	int rc = srt_denoise_after_trace(t, p, d.ns);
	if (rc == SRT_OK && d.fused_argb && t->dn.on) rc = srt_denoise_filter(t, ticks_stopped, d.fused_argb);
	if (rc) return rc;
	// a group member rendered on its own: its rows unfiltered (the group's resolver filters whole frames)
	if (d.fused_argb && !t->dn.on) return launch_resolve(t, t->canvas, (uint32_t)d.pixels, ticks_stopped, d.fused_argb);
	return SRT_OK;
}

// srt_trace; with fused_argb != NULL the last reduction also resolves every pixel it has just accumulated into fused_argb
// (owned pixels x 4 bytes, device memory) with the divisor ticks_stopped: what srt_resolve would do in a launch of its own
int srt_trace_fused(srt_tracer *t, const srt_render_data *options, uint8_t *fused_argb, uint32_t ticks_stopped) {
	if (!t) return SRT_ERR_INVALID;
	if (!options) return fail(t, SRT_ERR_INVALID, "srt_trace: options is NULL");
	if (options->width != t->width || options->height != t->height)
		return fail(t, SRT_ERR_INVALID, "srt_trace: options width/height differ from the handle's (no resize, tracer.hpp:61-66)");
	if (t->sky_w <= 0) return fail(t, SRT_ERR_STATE, "srt_trace: no skybox set (srt_set_skybox)");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int trc = srt_texture_sync(t)) return trc;
	t->last_rd = *options, t->have_last_rd = true; // selection.hip: the overlay's camera
	Dispatch d{};
	d.textured = t->tex_active && !options->show_normals; // (show_normals ignores textures: the untextured kernels)
	t->last_trace_textured = d.textured;
	// The kernel timers (srt_last_kernel_ms, srt_last_trace_kernel_ms) are four event records per dispatch: 10-17 us of a 150 us
	// interactive frame. srt_trace always takes them; the render calls only when asked to (srt_set_kernel_timers).
	d.timed = !fused_argb || t->timers_in_render;
	d.denoise = t->dn.on || t->gd_on;
	d.pixels = owned_pixels(t);
	d.ns = options->num_samples;
	d.fused_argb = fused_argb;
	TraceParams p = trace_params_of(t, options, d.textured);
	t->last_trace_class = srt_key_class(p.scene_class);
	t->last_trace_plane_form = srt_key_plane_form(p.scene_class);
	if (const int rc = reserve_radiance(t, d)) return rc;
	d.slots = wave_slots(t, p, d.textured);
	if (const int rc = reserve_scan_stacks(t, d)) return rc;
	ReduceParams rp = reduce_params_of(t, d, ticks_stopped);
	if (const int rc = reserve_timer_events(t, d.n_batches)) return rc;
	t->ev_k_used = 0;
	if (d.timed) SRT_HIP(t, hipEventRecord(t->ev_t0, t->stream));
	if (d.n_batches == 0) {
		// num_samples <= 0: no paths; the reduction still applies colour = 0 / num_samples (render.cl:520-522)
		rp.batch_samples = 0;
		rp.first_batch = rp.last_batch = 1;
		launch_reduce(t, rp, d.denoise, fused_argb);
	}
	t->batches_overlapped = d.n_batches > 1;
	if (t->batches_overlapped)
		if (const int rc = fork_batch_streams(t)) return rc;
	for (uint32_t b = 0; b < d.n_batches; b++)
		if (const int rc = launch_batch(t, d, b, p, rp)) return rc;
	if (d.denoise)
		if (const int rc = denoise_tail(t, d, p, ticks_stopped)) return rc;
	if (d.timed) SRT_HIP(t, hipEventRecord(t->ev_t1, t->stream));
	t->have_trace_ev = d.timed;
	t->have_kernel_ev = d.timed && d.n_batches > 0;
	return SRT_OK;
}

// srt_resolve / srt_resolve_external: launch_resolve between the resolve timer's events; `expose`: with the handle's exposure
// or bloom on, their launches (exposure.hip, bloom.hip) behind it, inside the same span: the image is the handle's own rows
static int resolve_impl(srt_tracer *t, const float *canvas, uint32_t num_pixels, uint32_t ticks_stopped, uint8_t *argb, bool expose) {
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipEventRecord(t->ev_r0, t->stream));
	if (const int rc = launch_resolve(t, canvas, num_pixels, ticks_stopped, argb)) return rc;
	if (expose)
		if (const int rc = srt_exposure_apply(t, canvas, (float)ticks_stopped, (uint32_t)t->width, (uint32_t)t->owned_rows, t->world == 1, argb)) return rc;
	if (expose)
		if (const int rc = srt_selection_apply(t, (uint32_t)t->width, (uint32_t)t->owned_rows, t->world == 1, argb)) return rc; // selection.hip: likewise
	SRT_HIP(t, hipEventRecord(t->ev_r1, t->stream));
	t->have_resolve_ev = true;
	return SRT_OK;
}

int srt_resolve(srt_tracer *t, uint32_t ticks_stopped) {
	if (!t) return SRT_ERR_INVALID;
	return resolve_impl(t, t->canvas, (uint32_t)owned_pixels(t), ticks_stopped, t->argb.ptr, true);
}

int srt_resolve_external(srt_tracer *t, const void *device_canvas, uint32_t num_pixels, uint32_t ticks_stopped,
                         void *device_argb) {
	if (!t) return SRT_ERR_INVALID;
	if (!device_canvas || !device_argb) return fail(t, SRT_ERR_INVALID, "srt_resolve_external: NULL buffer");
	return resolve_impl(t, static_cast<const float *>(device_canvas), num_pixels, ticks_stopped, static_cast<uint8_t *>(device_argb), false);
}

int srt_synchronize(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_render(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!argb_out) return fail(t, SRT_ERR_INVALID, "srt_render: argb_out is NULL");
	const int rc = srt_render_async(t, options, ticks_stopped, argb_out);
	if (rc) return rc;
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // blocking read-back, as queue.enqueue_read_buffer (src/tracer.cpp:115)
	return SRT_OK;
}

int srt_render_async(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!argb_out) return fail(t, SRT_ERR_INVALID, "srt_render_async: argb_out is NULL");
	int rc = srt_trace_fused(t, options, t->argb.ptr, ticks_stopped); // trace, ordered reduction and resolve: the last two in one launch
	if (rc) return rc;
	t->have_resolve_ev = false;
	if (const int erc = srt_exposure_apply_frame(t, ticks_stopped, t->argb.ptr)) return erc; // exposure.hip: nothing while the feature is off
	if (const int src = srt_selection_apply_frame(t, t->argb.ptr)) return src;               // selection.hip: likewise
	SRT_HIP(t, hipMemcpyAsync(argb_out, t->argb.ptr, owned_pixels(t) * 4, hipMemcpyDeviceToHost, t->stream));
	if (const int nrc = srt_noise_after_resolve(t)) return nrc; // noise_meter.hip: nothing while the feature is off
	return SRT_OK; // argb_out is valid after srt_synchronize()
}

int srt_read_canvas(srt_tracer *t, float *rgba_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!rgba_out) return fail(t, SRT_ERR_INVALID, "srt_read_canvas: NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemcpyAsync(rgba_out, t->canvas, owned_pixels(t) * 16, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_read_argb(srt_tracer *t, uint8_t *argb_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!argb_out) return fail(t, SRT_ERR_INVALID, "srt_read_argb: NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemcpyAsync(argb_out, t->argb.ptr, owned_pixels(t) * 4, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

// both sets of per-wave counter lines (device_types.h) read back into `w`, and the SRT_CTR_COUNT shared counters into `shared`
// when not NULL; returns once they have arrived
static int read_wave_counters(srt_tracer *t, std::vector<unsigned long long> &w, unsigned long long *shared) {
	try {
		w.resize((size_t)2 * SRT_WAVE_CTR_SLOTS * SRT_WAVE_CTR_STRIDE);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
	if (shared) SRT_HIP(t, hipMemcpyAsync(shared, t->counters.ptr, SRT_CTR_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipMemcpyAsync(w.data(), t->wave_counters.ptr, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_get_counters(srt_tracer *t, srt_counters *out) {
	if (!t) return SRT_ERR_INVALID;
	if (!out) return fail(t, SRT_ERR_INVALID, "srt_get_counters: NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	unsigned long long h[SRT_CTR_COUNT];
	std::vector<unsigned long long> w;
	if (const int rc = read_wave_counters(t, w, h)) return rc;
	unsigned long long sum[5] = {0, 0, 0, 0, 0};
	for (size_t i = 0; i < (size_t)2 * SRT_WAVE_CTR_SLOTS; i++)
		for (int k = 0; k < 5; k++) sum[k] += w[i * SRT_WAVE_CTR_STRIDE + k];
	out->rays = sum[0];
	out->sky = sum[1];
	out->paths = sum[2];
	out->tri_tests = sum[3];
	out->tri_pass_u = sum[4];
	out->nan_pixels = h[SRT_CTR_NAN];
	out->watchdog = h[SRT_CTR_WATCHDOG];
	return SRT_OK;
}

int srt_reset_counters(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemsetAsync(t->counters.ptr, 0, SRT_CTR_COUNT * sizeof(unsigned long long), t->stream));
	SRT_HIP(t, hipMemsetAsync(t->wave_counters.ptr, 0, (size_t)2 * SRT_WAVE_CTR_SLOTS * SRT_WAVE_CTR_STRIDE * sizeof(unsigned long long), t->stream));
	return SRT_OK;
}

int srt_last_kernel_ms(srt_tracer *t, float *trace_ms, float *resolve_ms) {
	if (!t) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if (trace_ms) {
		*trace_ms = 0.f;
		if (t->have_trace_ev) SRT_HIP(t, hipEventElapsedTime(trace_ms, t->ev_t0, t->ev_t1));
	}
	if (resolve_ms) {
		*resolve_ms = 0.f;
		if (t->have_resolve_ev) SRT_HIP(t, hipEventElapsedTime(resolve_ms, t->ev_r0, t->ev_r1));
	}
	return SRT_OK;
}

int srt_set_kernel_timers(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	t->timers_in_render = enable != 0;
	return SRT_OK;
}

int srt_set_radiance_budget(srt_tracer *t, size_t bytes) {
	if (!t) return SRT_ERR_INVALID;
	t->radiance_budget = bytes; // 0 = choose from free HBM at the next srt_trace
	return SRT_OK;
}

int srt_last_trace_kernel_ms(srt_tracer *t, float *kernel_ms) {
	if (!t) return SRT_ERR_INVALID;
	if (!kernel_ms) return fail(t, SRT_ERR_INVALID, "srt_last_trace_kernel_ms: NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	*kernel_ms = 0.f;
	if (t->have_kernel_ev && t->batches_overlapped && t->ev_k_used >= 4) {
		// overlapping launches: from the first batch's start to the later of the last two ends (the reductions of the earlier
		// batches run inside that span)
		for (size_t i = t->ev_k_used - 4; i + 1 < t->ev_k_used; i += 2) {
			float ms = 0.f;
			SRT_HIP(t, hipEventElapsedTime(&ms, t->ev_k[0], t->ev_k[i + 1]));
			if (ms > *kernel_ms) *kernel_ms = ms;
		}
	} else if (t->have_kernel_ev) {
		for (size_t i = 0; i + 1 < t->ev_k_used; i += 2) { // one pair per sample batch: the reductions between them are not counted
			float ms = 0.f;
			SRT_HIP(t, hipEventElapsedTime(&ms, t->ev_k[i], t->ev_k[i + 1]));
			*kernel_ms += ms;
		}
	}
	return SRT_OK;
}

int srt_last_trace_launches(const srt_tracer *t, int *launches, int *overlapped) {
	if (!t) return SRT_ERR_INVALID;
	if (launches) *launches = (int)(t->ev_k_used / 2);
	if (overlapped) *overlapped = t->batches_overlapped ? 1 : 0;
	return SRT_OK;
}

int srt_device_buffers(srt_tracer *t, void **canvas, size_t *canvas_bytes, void **argb, size_t *argb_bytes) {
	if (!t) return SRT_ERR_INVALID;
	if (canvas) *canvas = t->canvas;
	if (canvas_bytes) *canvas_bytes = t->canvas_bytes;
	if (argb) *argb = t->argb.ptr;
	if (argb_bytes) *argb_bytes = t->argb.cap;
	return SRT_OK;
}

int srt_bind_canvas(srt_tracer *t, void *device_canvas, size_t bytes) {
	if (!t) return SRT_ERR_INVALID;
	if (t->gd_on) return fail(t, SRT_ERR_STATE, "srt_bind_canvas: the handle's group has its denoiser on: the canvas lives in the member's gather buffer (srt_group_set_denoise(g, NULL) first)");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if (!device_canvas) {
		t->canvas = t->canvas_own.ptr;
		t->canvas_bytes = t->canvas_own.cap * sizeof(float);
		return SRT_OK;
	}
	if (bytes < owned_pixels(t) * 16) return fail(t, SRT_ERR_INVALID, "srt_bind_canvas: buffer smaller than owned_rows*width*16");
	t->canvas = static_cast<float *>(device_canvas);
	t->canvas_bytes = bytes;
	return SRT_OK;
}

int srt_bind_stream(srt_tracer *t, void *hip_stream) {
	if (!t) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	t->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : t->own_stream;
	return SRT_OK;
}

int srt_set_partition(srt_tracer *t, int rank, int world, int rows_per_block) {
	if (!t) return SRT_ERR_INVALID;
	if (world < 1 || rank < 0 || rank >= world || rows_per_block < 1)
		return fail(t, SRT_ERR_INVALID, "srt_set_partition: need 0 <= rank < world and rows_per_block >= 1");
	if (t->gd_on) return fail(t, SRT_ERR_STATE, "srt_set_partition: the handle's group has its denoiser on (srt_group_set_denoise(g, NULL) first)");
	if (world > 1 && t->dn.temporal) return fail(t, SRT_ERR_STATE, "srt_set_partition: temporal reprojection works on the full frame only (srt_set_denoise_temporal(t, NULL) first)");
	if (world > 1 && t->dn.on) return fail(t, SRT_ERR_STATE, "srt_set_partition: the denoiser works on the full frame only (srt_set_denoise(t, NULL) first)");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	const int padded = srt_partition_padded_rows(t->height, world, rows_per_block);
	const size_t need = (size_t)padded * t->width * 4; // floats; padded >= owned
	if (t->canvas == t->canvas_own.ptr) {
		SRT_HIP(t, t->canvas_own.reserve(need));
		t->canvas = t->canvas_own.ptr;
		t->canvas_bytes = t->canvas_own.cap * sizeof(float);
	} else if (t->canvas_bytes < need * sizeof(float)) {
		return fail(t, SRT_ERR_INVALID, "srt_set_partition: bound canvas too small for padded_rows*width*16");
	}
	SRT_HIP(t, t->argb.reserve((size_t)padded * t->width * 4));
	t->rank = rank;
	t->world = world;
	t->rows_per_block = rows_per_block;
	t->owned_rows = srt_partition_owned_rows(t->height, rank, world, rows_per_block);
	SRT_HIP(t, hipMemsetAsync(t->argb.ptr, 0, t->argb.cap, t->stream));
	return clear_canvas_impl(t);
}

int srt_selftest_math(srt_tracer *t, uint32_t stride, uint64_t out[16]) {
	if (!t) return SRT_ERR_INVALID;
	if (!out || stride == 0) return fail(t, SRT_ERR_INVALID, "srt_selftest_math: bad arguments");
	SRT_HIP(t, hipSetDevice(t->device));
	unsigned long long *d = nullptr;
	SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&d), 16 * sizeof(unsigned long long)));
	hipError_t e = hipMemsetAsync(d, 0, 16 * sizeof(unsigned long long), t->stream);
	if (e == hipSuccess) {
		srt_launch_selftest(d, stride, t->stream);
		e = hipGetLastError();
	}
	unsigned long long h[16] = {0};
	if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(t, SRT_ERR_HIP, std::string("srt_selftest_math: ") + hipGetErrorString(e));
	for (int i = 0; i < 16; i++) out[i] = h[i];
	return SRT_OK;
}

int srt_selftest_rare_lanes(srt_tracer *t, int what, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, uint64_t *mismatches) {
	if (!t) return SRT_ERR_INVALID;
	if (!in || !out_new || !out_ref || !mismatches || what < 0 || what > 1 || waves == 0 || waves > 65536u)
		return fail(t, SRT_ERR_INVALID, "srt_selftest_rare_lanes: bad arguments");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t lanes = (size_t)waves * 64u, in_bytes = lanes * 8u * sizeof(uint32_t), out_bytes = lanes * 4u * sizeof(uint32_t);
	char *d = nullptr; // [in | out_new | out_ref | count]
	SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&d), in_bytes + 2 * out_bytes + sizeof(unsigned long long)));
	uint32_t *d_in = reinterpret_cast<uint32_t *>(d), *d_new = reinterpret_cast<uint32_t *>(d + in_bytes), *d_ref = reinterpret_cast<uint32_t *>(d + in_bytes + out_bytes);
	unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(d + in_bytes + 2 * out_bytes), h_bad = 0;
	hipError_t e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, t->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_new, 0, 2 * out_bytes + sizeof(unsigned long long), t->stream);
	if (e == hipSuccess) {
		srt_launch_selftest_rare(what, d_in, waves, d_new, d_ref, d_bad, t->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out_new, d_new, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(out_ref, d_ref, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(t, SRT_ERR_HIP, std::string("srt_selftest_rare_lanes: ") + hipGetErrorString(e));
	*mismatches = h_bad;
	return SRT_OK;
}

int srt_selftest_plane_forms(srt_tracer *t, int what, const float planes[32], const float cam_org[3], const uint32_t *in, uint32_t waves, uint32_t *out_new,
                             uint32_t *out_ref, uint32_t *fast, uint64_t *mismatches) {
	if (!t) return SRT_ERR_INVALID;
	if (!planes || !cam_org || !in || !out_new || !out_ref || !fast || !mismatches || what < 0 || what > 1 || waves == 0 || waves > 65536u)
		return fail(t, SRT_ERR_INVALID, "srt_selftest_plane_forms: bad arguments");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t lanes = (size_t)waves * 64u, in_bytes = lanes * 8u * sizeof(uint32_t), out_bytes = lanes * 2u * sizeof(uint32_t), fast_bytes = (size_t)waves * sizeof(uint32_t);
	char *d = nullptr; // [in | out_new | out_ref | count | fast]
	SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&d), in_bytes + 2 * out_bytes + sizeof(unsigned long long) + fast_bytes));
	uint32_t *d_in = reinterpret_cast<uint32_t *>(d), *d_new = reinterpret_cast<uint32_t *>(d + in_bytes), *d_ref = reinterpret_cast<uint32_t *>(d + in_bytes + out_bytes);
	unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(d + in_bytes + 2 * out_bytes), h_bad = 0;
	uint32_t *d_fast = reinterpret_cast<uint32_t *>(d + in_bytes + 2 * out_bytes + sizeof(unsigned long long));
	hipError_t e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, t->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_new, 0, 2 * out_bytes + sizeof(unsigned long long) + fast_bytes, t->stream);
	if (e == hipSuccess) {
		srt_launch_selftest_plane_forms(what, planes, cam_org, d_in, waves, d_new, d_ref, d_fast, d_bad, t->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out_new, d_new, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(out_ref, d_ref, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(fast, d_fast, fast_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(t, SRT_ERR_HIP, std::string("srt_selftest_plane_forms: ") + hipGetErrorString(e));
	*mismatches = h_bad;
	return SRT_OK;
}

int srt_selftest_diffuse_bounce(srt_tracer *t, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, uint32_t *fast, uint64_t *mismatches) {
	if (!t) return SRT_ERR_INVALID;
	if (!in || !out_new || !out_ref || !fast || !mismatches || waves == 0 || waves > 65536u) return fail(t, SRT_ERR_INVALID, "srt_selftest_diffuse_bounce: bad arguments");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t lanes = (size_t)waves * 64u, in_bytes = lanes * 20u * sizeof(uint32_t), out_bytes = lanes * 8u * sizeof(uint32_t), fast_bytes = (size_t)waves * sizeof(uint32_t);
	char *d = nullptr; // [in | out_new | out_ref | count | fast]
	SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&d), in_bytes + 2 * out_bytes + sizeof(unsigned long long) + fast_bytes));
	uint32_t *d_in = reinterpret_cast<uint32_t *>(d), *d_new = reinterpret_cast<uint32_t *>(d + in_bytes), *d_ref = reinterpret_cast<uint32_t *>(d + in_bytes + out_bytes);
	unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(d + in_bytes + 2 * out_bytes), h_bad = 0;
	uint32_t *d_fast = reinterpret_cast<uint32_t *>(d + in_bytes + 2 * out_bytes + sizeof(unsigned long long));
	hipError_t e = hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, t->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_new, 0, 2 * out_bytes + sizeof(unsigned long long) + fast_bytes, t->stream);
	if (e == hipSuccess) {
		srt_launch_selftest_diffuse_bounce(d_in, waves, d_new, d_ref, d_fast, d_bad, t->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out_new, d_new, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(out_ref, d_ref, out_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(fast, d_fast, fast_bytes, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(t, SRT_ERR_HIP, std::string("srt_selftest_diffuse_bounce: ") + hipGetErrorString(e));
	*mismatches = h_bad;
	return SRT_OK;
}

/* diagnostics: sums of the eight per-wave counter slots since the last reset (slot 5 = the scene-class kernels' EXTEND phases of
 * fresh camera rays only << 36 | the rays in those phases, 6 = wave iterations, 7 = SHADE phases; out[10], out[11] = an axis
 * twin's EXTEND phases and those among them that failed its guard, out[12], out[13] = a NO_SPEC class's SHADE phases that ran no
 * per-lane bounce and those that failed the diffuse-wave guard, in the slots the -DSRT_PHASE_CLOCK builds keep clocks in) */
int srt_debug_counters(srt_tracer *t, uint64_t out[18]) {
	if (!t || !out) return SRT_ERR_INVALID;
	SRT_HIP(t, hipSetDevice(t->device));
	std::vector<unsigned long long> w;
	if (const int rc = read_wave_counters(t, w, nullptr)) return rc;
	for (int k = 0; k < 18; k++) out[k] = 0;
	for (size_t i = 0; i < (size_t)2 * SRT_WAVE_CTR_SLOTS; i++) {
		for (int k = 0; k < 8; k++) out[k] += w[i * SRT_WAVE_CTR_STRIDE + k];
		for (int k = 8; k < 16; k++) out[k + 2] += w[i * SRT_WAVE_CTR_STRIDE + k]; // phase clocks of -DSRT_PHASE_CLOCK builds
	}
	out[8] = (uint64_t)t->last_waves_per_cu;
	out[9] = (uint64_t)t->last_grid;
	return SRT_OK;
}

/* -DSRT_REGION_COUNT builds: per region of the trace kernel (trace_regions.h SRT_REGION_LIST, in that order) how often a wave
 * ran it and with how many lanes, summed over the waves since the last reset. *written = 0 in the product build. */
int srt_debug_region_counters(srt_tracer *t, uint64_t *out, int capacity, int *written) {
	if (!t || !out || !written || capacity < 0) return SRT_ERR_INVALID;
	*written = 0;
#ifdef SRT_REGION_COUNT
	SRT_HIP(t, hipSetDevice(t->device));
	std::vector<unsigned long long> w;
	if (const int rc = read_wave_counters(t, w, nullptr)) return rc;
	const int n = capacity < 2 * SRT_REGION_MAX ? capacity : 2 * SRT_REGION_MAX;
	for (int k = 0; k < n; k++) out[k] = 0;
	for (size_t i = 0; i < (size_t)2 * SRT_WAVE_CTR_SLOTS; i++)
		for (int k = 0; k < n; k++) out[k] += w[i * SRT_WAVE_CTR_STRIDE + 16 + k];
	*written = n;
#endif
	return SRT_OK;
}

/* test hook: build with triangle counters (instrumented kernel variant) */
int srt_set_count_triangles(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	t->count_tris = enable != 0;
	return SRT_OK;
}

} // extern "C"

// ray_query.hip's way to trace_params_of: a query is handed the scene exactly as a dispatch is (never a textured one: a query
// samples no texture)
TraceParams srt_trace_params_for_query(const srt_tracer *t, const srt_render_data *options) { return trace_params_of(t, options, false); }
