// ray_query.hip -- ray queries behind the ABI (include/srt_abi.h "ray queries"): the closest hit of caller rays in the handle's
// scene, and picking. A translation unit of its own: the kernels here are new, every kernel the library launched before keeps
// its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_ray_query_kernel<HAS_MODELS, USE_BVH>: one lane per ray, one wave per workgroup, the lane's BVH stack in scratch -- the
//    feature kernels' launch shape (kernels.hip srt_features_kernel) and their closest-hit walk, which is closest_hit.inc for
//    both (and for selection.hip's ID pass): test_block over p.runs with the tests of device_intersect.h, so the same closest
//    hit as the trace's EXTEND, then winner_normal of device_shading.h. What differs: the ray comes from memory (two 128-bit
//    loads) instead of the camera, the validity test of ray_valid.inc (shared with occlusion.hip and the ID pass) stands in
//    front of the walk, tmin starts from the ray's tmax, and the result is a record (two 128-bit stores) instead of a sum into
//    guide planes.
//  * srt_pick_rays_kernel: the rays of picked image points, device_math.h camera_ray (shared with the ID pass): the trace's
//    CAMERA phase with the caller's x, y in place of pixel + jitter.
// The two .inc files are text because the same statements as __device__ functions compile to other instruction streams
// (DESIGN.md 28, 29). The scene arrives as the TraceParams a dispatch would be handed (srt_abi.hip trace_params_of), beside it
// the per-triangle material table when the scene has one. The host side's scaffold -- count check, timed span, kernel pick and
// launch, the staging allocation's layout -- is query_host.h, shared with occlusion.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_shading.h"
#include "query_host.h"

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
	const uint32_t flags = qp.flags;
#include "ray_valid.inc"
	// ---- closest_intersection: tmin starts from tmax ----
	float tmin = DM_INF_F;
	int best = -1;
	uint32_t best_tri = 0;
	if (valid && tmax > 0.0f) { // (tmax <= 0: nothing is closer than it)
		BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		uint32_t n_tri = 0, n_tri_u = 0;
		tmin = tmax;
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
#include "closest_hit.inc"
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

// The rays of picked image points
__global__ __launch_bounds__(64) void srt_pick_rays_kernel(const PickParams pp) {
	const TraceParams &p = pp.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= pp.n) return;
	f3 cam, dir;
	camera_ray(p, pp.xy[q], cam, dir);
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

// the cast over device arrays, enqueued on the handle's stream (the caller has checked the arguments and set the device)
int enqueue_cast(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *hits_dev) {
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table as the next dispatch would see it
	RayQueryParams qp;
	memset(&qp, 0, sizeof qp);
	qp.tp = query_scene_params(t);
	qp.rays = static_cast<const float4 *>(rays_dev);
	qp.hits = static_cast<float4 *>(hits_dev);
	qp.tri_materials = srt_texture_params(t).tri_materials;
	qp.n = (uint32_t)n;
	qp.flags = flags;
	query_launch(SRT_QUERY_KERNEL(srt_ray_query_kernel, qp.tp), qp, qp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

} // namespace

int srt_enqueue_pick_rays(srt_tracer *t, const srt_render_data *options, const void *xy_dev, size_t n, void *rays_dev) {
	PickParams pp;
	memset(&pp, 0, sizeof pp);
	pp.tp = srt_trace_params_for_query(t, options);
	pp.xy = static_cast<const float2 *>(xy_dev);
	pp.rays = static_cast<float4 *>(rays_dev);
	pp.n = (uint32_t)n;
	query_launch(srt_pick_rays_kernel, pp, pp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

extern "C" {

int srt_ray_query_sizes(size_t out[2]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_ray);
	out[1] = sizeof(srt_ray_hit);
	return SRT_OK;
}

int srt_cast_rays_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *hits_dev) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_cast_rays_device", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays_dev || !hits_dev) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_device: NULL array");
	if (((uintptr_t)rays_dev | (uintptr_t)hits_dev) & 15u) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_device: arrays must be aligned to 16 bytes");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_cast(t, rays_dev, n, flags, hits_dev)) return rc;
	return query_span_end(t);
}

int srt_cast_rays(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_cast_rays", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays || !hits) return fail(t, SRT_ERR_INVALID, "srt_cast_rays: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.rays, rays, n * sizeof(srt_ray), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_cast(t, stage + st.rays, n, flags, stage + st.hits)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(hits, stage + st.hits, n * sizeof(srt_ray_hit), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_pick(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_pick", n, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!options || !xy || !hits) return fail(t, SRT_ERR_INVALID, "srt_pick: NULL argument");
	if (options->width <= 0 || options->height <= 0) return fail(t, SRT_ERR_INVALID, "srt_pick: options->width and height must be positive");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.xy, xy, n * 2 * sizeof(float), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = srt_enqueue_pick_rays(t, options, stage + st.xy, n, stage + st.rays)) return rc;
	if (const int rc = enqueue_cast(t, stage + st.rays, n, SRT_RAYS_UNIT_DIRECTIONS, stage + st.hits)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(hits, stage + st.hits, n * sizeof(srt_ray_hit), hipMemcpyDeviceToHost, t->stream));
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
