// ray_query.hip -- ray queries behind the ABI (include/srt_abi.h "ray queries"): the closest hit of caller rays in the handle's
// scene, and picking. A translation unit of its own: the kernels here are new, every kernel the library launched before keeps
// its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_ray_query_kernel<HAS_MODELS, USE_BVH>: one lane per ray, one wave per workgroup, the lane's BVH stack in scratch -- the
//    feature kernels' launch shape (kernels.hip srt_features_kernel) and their closest-hit loop (features_body.inc): the same
//    test_block over p.runs with the tests of device_intersect.h, so the same closest hit as the trace's EXTEND, then
//    winner_normal of device_shading.h. What differs: the ray comes from memory (two 128-bit loads) instead of the camera, a
//    validity test stands in front of the loop, tmin starts from the ray's tmax, and the result is a record (two 128-bit
//    stores) instead of a sum into guide planes.
//  * srt_pick_rays_kernel: the rays of picked image points, the statements of the trace's CAMERA phase with the caller's x, y
//    in place of pixel + jitter.
// The scene arrives as the TraceParams a dispatch would be handed (srt_abi.hip trace_params_of), beside it the per-triangle
// material table when the scene has one.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_shading.h"
#include "srt_internal.h"

struct RayQueryParams {
	TraceParams tp;               /* the scene buffers, as a dispatch's (rd: unused by the cast) */
	const float4 *rays;           /* n srt_ray */
	float4 *hits;                 /* n srt_ray_hit */
	const int32_t *tri_materials; /* per-triangle materials of the scene's triangle array, or NULL */
	uint32_t n;
	uint32_t flags; /* SRT_RAYS_* */
};
struct PickParams {
	TraceParams tp;   /* rd: the camera and frame size; f_width .. inv_f_height as a dispatch of rd has them */
	const float2 *xy; /* n points */
	float4 *rays;     /* n srt_ray */
	uint32_t n;
};

namespace {
__device__ __forceinline__ bool finite_bits(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite3(f3 a) { return finite_bits(a.x) && finite_bits(a.y) && finite_bits(a.z); }
} // namespace

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_ray_query_kernel(const RayQueryParams qp) {
	const TraceParams &p = qp.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= qp.n) return; // lanes past n in the last workgroup load and store nothing
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	const float4 r0 = qp.rays[2u * q], r1 = qp.rays[2u * q + 1u];
	const f3 org = mk(r0.x, r0.y, r0.z);
	f3 dir = mk(r1.x, r1.y, r1.z);
	const float tmax = r0.w;
	// ---- hostile rays: decided here, device-resident rays never pass the host ----
	bool valid = finite3(org) && finite3(dir) && tmax == tmax;
	if (!(qp.flags & SRT_RAYS_UNIT_DIRECTIONS)) {
		// detmath's division-free rsqrt keeps normalize(0) = 0, gives a large finite value where the squared length underflows and
		// no number where it overflows: what comes out is a direction only if it has unit length (NaN compares false)
		dir = normalize3(dir);
		const float len2 = dot3(dir, dir);
		valid = valid && len2 > 0.25f && len2 < 4.0f;
	}
	valid = valid && finite3(dir) && !(dir.x == 0.0f && dir.y == 0.0f && dir.z == 0.0f);
	// ---- closest_intersection: srt_trace_kernel EXTEND (test_block), as features_body.inc; tmin starts from tmax ----
	float tmin = DM_INF_F;
	int best = -1;
	uint32_t best_tri = 0;
	if (valid && tmax > 0.0f) { // (tmax <= 0: nothing is closer than it)
		BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		uint32_t n_tri = 0, n_tri_u = 0;
		tmin = tmax;
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
				if (((code >> 2) & 7u) <= 2u) test_spheres<2>(b, org, dir, base, tmin, best);
				else test_spheres<4>(b, org, dir, base, tmin, best);
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
				test_planes2(b, (code >> 2) & 7u, org, dir, base, tmin, best);
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				if (test_aabb(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], org, inv, tmin)) {
					if (USE_BVH) walk_bvh<false>(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, f2u(b.v[3]), org, dir, base, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
					else test_triangles<false>(p.wtris, f2u(b.v[3]), f2u(b.v[7]), org, dir, base, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
				}
				if (((code >> 2) & 7u) > 1u && test_aabb(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], org, inv, tmin)) {
					if (USE_BVH) walk_bvh<false>(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, f2u(b.v[11]), org, dir, base + 1, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
					else test_triangles<false>(p.wtris, f2u(b.v[11]), f2u(b.v[15]), org, dir, base + 1, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
				}
			}
		};
		for (int g = 0; g < p.num_runs; g++) {
			float gh[4];
			ld_uniform<4, 16>(reinterpret_cast<const float *>(p.runs + g), gh);
			const uint32_t code = f2u(gh[0]);
			const float *__restrict__ gd = p.run_data + 48 * g;
			test_block(ld_blk16(gd), code & 255u, (int)f2u(gh[1]));
			if ((code >> 8) & 255u) test_block(ld_blk16(gd + 16), (code >> 8) & 255u, (int)f2u(gh[2]));
			if ((code >> 16) & 255u) test_block(ld_blk16(gd + 32), (code >> 16) & 255u, (int)f2u(gh[3]));
		}
	}
	// ---- the record ----
	float4 h0, h1;
	h0.x = DM_INF_F, h0.y = dm_u2f(SRT_HIT_NONE), h0.z = dm_u2f(SRT_HIT_NONE), h0.w = dm_u2f(0xffffffffu); // material -1
	h1.x = 0.0f, h1.y = 0.0f, h1.z = 0.0f, h1.w = dm_u2f(valid ? 0u : SRT_HIT_INVALID_RAY);
	if (best >= 0) {
		const WinnerRec *__restrict__ wr = p.winners + best;
		int material = wr->material; // a shape without a material is reported (a picker selects it); the trace's sky rule is not applied
		uint32_t tri = SRT_HIT_NONE;
		if (HAS_MODELS && wr->type != SRT_SHAPE_SPHERE && wr->type != SRT_SHAPE_PLANE) {
			tri = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
			if (qp.tri_materials && material >= 0) { // (uniform over the launch) the material the trace shades the hit with
				const int tm = qp.tri_materials[p.shapes[best].shape.model.triangle_index + tri];
				material = tm >= 0 ? tm : material;
			}
		}
		f3 nrm = winner_normal<HAS_MODELS, USE_BVH>(p, best, best_tri, org + dir * tmin);
		const bool front = dot3(nrm, dir) < 0.0f;
		nrm = nrm * (front ? 1.0f : -1.0f);
		h0.x = tmin, h0.y = dm_u2f((uint32_t)best), h0.z = dm_u2f(tri), h0.w = dm_u2f((uint32_t)material);
		h1.x = nrm.x, h1.y = nrm.y, h1.z = nrm.z, h1.w = dm_u2f(SRT_HIT_HIT | (front ? SRT_HIT_FRONT : 0u));
	}
	qp.hits[2u * q] = h0;
	qp.hits[2u * q + 1u] = h1;
}

// The rays of picked image points: srt_trace_kernel CAMERA (as features_body.inc states it) with the caller's x, y
__global__ __launch_bounds__(64) void srt_pick_rays_kernel(const PickParams pp) {
	const TraceParams &p = pp.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= pp.n) return;
	const float2 xy = pp.xy[q];
	const f3 c0 = mk(p.rd.camera_to_world[0].x, p.rd.camera_to_world[0].y, p.rd.camera_to_world[0].z);
	const f3 c1 = mk(p.rd.camera_to_world[1].x, p.rd.camera_to_world[1].y, p.rd.camera_to_world[1].z);
	const f3 c2 = mk(p.rd.camera_to_world[2].x, p.rd.camera_to_world[2].y, p.rd.camera_to_world[2].z);
	const f3 cam = mk(p.rd.camera_to_world[3].x, p.rd.camera_to_world[3].y, p.rd.camera_to_world[3].z);
	const float ndc_x = div_by_rcp(xy.x, p.f_width, p.inv_f_width);
	const float ndc_y = div_by_rcp(xy.y, p.f_height, p.inv_f_height);
	const float sx = ((2.f * ndc_x - 1.f) * p.rd.aspect_ratio) * p.rd.fov_scale;
	const float sy = (1.f - 2.f * ndc_y) * p.rd.fov_scale;
	const f3 dir = normalize3(mat_cols_by_vec(c0, c1, c2, cam, mk(sx, sy, -1.0f), 0.0f));
	float4 r0, r1;
	r0.x = cam.x, r0.y = cam.y, r0.z = cam.z, r0.w = DM_INF_F;
	r1.x = dir.x, r1.y = dir.y, r1.z = dir.z, r1.w = 0.0f;
	pp.rays[2u * q] = r0;
	pp.rays[2u * q + 1u] = r1;
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

// the cast's kernel, picked as srt_launch_features picks its own
void launch_ray_query(const RayQueryParams &qp, hipStream_t stream) {
	typedef void (*QueryKernel)(const RayQueryParams);
	const bool models = qp.tp.num_models > 0, bvh = qp.tp.use_bvh != 0;
	const QueryKernel k = !models ? srt_ray_query_kernel<false, false> : bvh ? srt_ray_query_kernel<true, true> : srt_ray_query_kernel<true, false>;
	hipLaunchKernelGGL(k, dim3((qp.n + 63u) / 64u), dim3(64), 0, stream, qp);
}

// a render data that only sizes trace_params_of's camera fields (the cast reads none of them)
srt_render_data no_camera() {
	srt_render_data rd;
	memset(&rd, 0, sizeof rd);
	rd.width = rd.height = 1;
	return rd;
}

int check_count(srt_tracer *t, const char *who, size_t n, uint32_t flags) {
	if (flags & ~SRT_RAYS_UNIT_DIRECTIONS) return fail(t, SRT_ERR_INVALID, std::string(who) + ": unknown flag bits");
	if (n >= ((size_t)1 << 31)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": n must stay below 2^31 rays");
	return SRT_OK;
}

// the cast over device arrays, enqueued on the handle's stream (the caller has checked the arguments and set the device)
int enqueue_cast(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *hits_dev) {
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table as the next dispatch would see it
	const srt_render_data rd = no_camera();
	RayQueryParams qp;
	memset(&qp, 0, sizeof qp);
	qp.tp = srt_trace_params_for_query(t, &rd);
	qp.rays = static_cast<const float4 *>(rays_dev);
	qp.hits = static_cast<float4 *>(hits_dev);
	qp.tri_materials = srt_texture_params(t).tri_materials;
	qp.n = (uint32_t)n;
	qp.flags = flags;
	launch_ray_query(qp, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

// the staging allocation: n rays, n hits, n points
int reserve_stage(srt_tracer *t, size_t n) {
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // (a grown buffer replaces one a queued launch may still use)
	SRT_HIP(t, t->rq_stage.reserve(n * 72));
	return SRT_OK;
}
uint8_t *stage_rays(const srt_tracer *t) { return t->rq_stage.ptr; }
uint8_t *stage_hits(const srt_tracer *t, size_t n) { return t->rq_stage.ptr + 32 * n; }
uint8_t *stage_xy(const srt_tracer *t, size_t n) { return t->rq_stage.ptr + 64 * n; }

int span_begin(srt_tracer *t) {
	t->rq_span.timed = false;
	if (t->timers_in_render) SRT_HIP(t, t->rq_span.begin(t->stream));
	return SRT_OK;
}
int span_end(srt_tracer *t) {
	if (t->timers_in_render) SRT_HIP(t, t->rq_span.end(t->stream));
	return SRT_OK;
}

} // namespace

extern "C" {

int srt_ray_query_sizes(size_t out[2]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_ray);
	out[1] = sizeof(srt_ray_hit);
	return SRT_OK;
}

int srt_cast_rays_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *hits_dev) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = check_count(t, "srt_cast_rays_device", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays_dev || !hits_dev) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_device: NULL array");
	if (((uintptr_t)rays_dev | (uintptr_t)hits_dev) & 15u) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_device: arrays must be aligned to 16 bytes");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = span_begin(t)) return rc;
	if (const int rc = enqueue_cast(t, rays_dev, n, flags, hits_dev)) return rc;
	return span_end(t);
}

int srt_cast_rays(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = check_count(t, "srt_cast_rays", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays || !hits) return fail(t, SRT_ERR_INVALID, "srt_cast_rays: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = reserve_stage(t, n)) return rc;
	SRT_HIP(t, hipMemcpyAsync(stage_rays(t), rays, n * sizeof(srt_ray), hipMemcpyHostToDevice, t->stream));
	if (const int rc = span_begin(t)) return rc;
	if (const int rc = enqueue_cast(t, stage_rays(t), n, flags, stage_hits(t, n))) return rc;
	if (const int rc = span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(hits, stage_hits(t, n), n * sizeof(srt_ray_hit), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_pick(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = check_count(t, "srt_pick", n, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!options || !xy || !hits) return fail(t, SRT_ERR_INVALID, "srt_pick: NULL argument");
	if (options->width <= 0 || options->height <= 0) return fail(t, SRT_ERR_INVALID, "srt_pick: options->width and height must be positive");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = reserve_stage(t, n)) return rc;
	SRT_HIP(t, hipMemcpyAsync(stage_xy(t, n), xy, n * 2 * sizeof(float), hipMemcpyHostToDevice, t->stream));
	if (const int rc = span_begin(t)) return rc;
	PickParams pp;
	memset(&pp, 0, sizeof pp);
	pp.tp = srt_trace_params_for_query(t, options);
	pp.xy = reinterpret_cast<const float2 *>(stage_xy(t, n));
	pp.rays = reinterpret_cast<float4 *>(stage_rays(t));
	pp.n = (uint32_t)n;
	hipLaunchKernelGGL(srt_pick_rays_kernel, dim3((pp.n + 63u) / 64u), dim3(64), 0, t->stream, pp);
	SRT_HIP(t, hipGetLastError());
	if (const int rc = enqueue_cast(t, stage_rays(t), n, SRT_RAYS_UNIT_DIRECTIONS, stage_hits(t, n))) return rc;
	if (const int rc = span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(hits, stage_hits(t, n), n * sizeof(srt_ray_hit), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_last_ray_query_ms(srt_tracer *t, float *ms) {
	if (!t) return SRT_ERR_INVALID;
	if (!ms) return fail(t, SRT_ERR_INVALID, "srt_last_ray_query_ms: NULL");
	*ms = 0.f;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	SRT_HIP(t, t->rq_span.elapsed(ms));
	return SRT_OK;
}

} // extern "C"
