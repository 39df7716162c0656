// nearest.hip -- nearest-surface queries behind the ABI (include/srt_abi.h "nearest-surface queries"): for caller points, the
// closest point of the handle's scene, its distance and what it lies on. A translation unit of its own: the kernels here are
// new, every kernel the library launched before keeps its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_nearest_kernel<HAS_MODELS, USE_BVH>: one lane per query, one wave per workgroup, the lane's BVH stack in scratch -- the
//    cast's launch shape (ray_query.hip), picked and launched through query_host.h. The query comes in as one 128-bit load, the
//    answer goes out as two 128-bit stores; lanes past n leave before either.
//  * The shapes are walked over p.runs as closest_hit.inc walks them, and that file is NOT included: the block test differs in
//    substance. A ray cannot hit a block's filler records, but a point can be near them (a filler sphere sits at the origin, a
//    filler plane has a zero normal), so the block's shape count from the group code bounds every loop; a sphere's radius is
//    read from its winner record (the block holds r * r, and the contract is over |radius|); a model is left out by the squared
//    distance to its record's box instead of a slab test, and its triangles go through device_nearest.h's scan or walk.
//  * The distance functions are nearest_math.h, which the host exports at the bottom compile too.
// The answer is a minimum over primitives with ties to the lower index: shapes are visited in array order and replaced only by a
// strictly smaller distance, triangles of one model by a smaller distance or, at the same one, a lower index.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_nearest.h"
#include "query_host.h"

struct NearestParams {
	TraceParams tp;               /* the scene buffers, as a dispatch's (rd: unused) */
	const float4 *queries;        /* n srt_point_query */
	float4 *out;                  /* n srt_nearest */
	const int32_t *tri_materials; /* per-triangle materials of the scene's triangle array, or NULL */
	uint32_t n;
	uint32_t skip; /* the shape left out, SRT_HIT_NONE: none */
};

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_nearest_kernel(const NearestParams np) {
	const TraceParams &p = np.tp;
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	if (i >= np.n) return; // lanes past n in the last workgroup load and store nothing
	const float4 in = np.queries[i];
	const f3 q = mk(in.x, in.y, in.z);
	const float maxd = in.w;
	const bool valid = finite3(q) && maxd == maxd;
	NearestBest best;
	best.d = maxd, best.shape = -1, best.rec = SRT_HIT_NONE, best.px = best.py = best.pz = 0.0f, best.flags = 0u;
	if (valid && maxd > 0.0f) { // (max_distance <= 0: nothing is closer than it)
		BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		const uint32_t skip = np.skip;
		const float qmax = __builtin_fmaxf(__builtin_fmaxf(dm_fabs(q.x), dm_fabs(q.y)), dm_fabs(q.z));
		// model record m of block b (8 dwords at b.v[o]): {min, first world triangle or root, max, count}
		auto test_model = [&](const Blk16 &b, int o, int idx) {
			const float d2 = nearest_box_d2(nearest_gap(b.v[o] - q.x, b.v[o + 4] - q.x), nearest_gap(b.v[o + 1] - q.y, b.v[o + 5] - q.y),
			                                nearest_gap(b.v[o + 2] - q.z, b.v[o + 6] - q.z));
			// the largest |coordinate| of the box (wave-uniform) and of the point: what the rounding errors of a closest point are
			// relative to (device_nearest.h PRUNING)
			const float bmax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(dm_fabs(b.v[o]), dm_fabs(b.v[o + 1])), __builtin_fmaxf(dm_fabs(b.v[o + 2]), dm_fabs(b.v[o + 4]))),
			                                   __builtin_fmaxf(dm_fabs(b.v[o + 5]), dm_fabs(b.v[o + 6])));
			const float slack = (bmax + qmax) * 0x1p-17f;
			if (d2 > nearest_reach2(best.d, slack)) return; // strictly beyond: a box at the best distance is still searched
			if (USE_BVH) nearest_walk(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, f2u(b.v[o + 3]), q, idx, slack, best);
			else nearest_scan(p.wtris, f2u(b.v[o + 3]), f2u(b.v[o + 7]), q, idx, best);
		};
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u, count = (code >> 2) & 7u; // count: the block's shapes; the rest are fillers, never candidates
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
#pragma unroll
				for (int k = 0; k < 4; k++) {
					if ((uint32_t)k >= count || (uint32_t)(base + k) == skip) continue; // (wave-uniform)
					float radius[1];
					ld_uniform<1, 4>(reinterpret_cast<const float *>(p.winners + (base + k)) + 5, radius); // WinnerRec.w
					const nm_result r = nm_sphere(b.v[4 * k], b.v[4 * k + 1], b.v[4 * k + 2], radius[0], q.x, q.y, q.z);
					if (r.distance < best.d) nearest_take(best, r, base + k, SRT_HIT_NONE);
				}
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
#pragma unroll
				for (int k = 0; k < 2; k++) {
					if ((uint32_t)k >= count || (uint32_t)(base + k) == skip) continue;
					const nm_result r = nm_plane(b.v[8 * k], b.v[8 * k + 1], b.v[8 * k + 2], b.v[8 * k + 4], b.v[8 * k + 5], b.v[8 * k + 6], q.x, q.y, q.z);
					if (r.distance < best.d) nearest_take(best, r, base + k, SRT_HIT_NONE);
				}
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				if (count > 0u && (uint32_t)base != skip) test_model(b, 0, base);
				if (count > 1u && (uint32_t)(base + 1) != skip) test_model(b, 8, base + 1);
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
	float4 o0, o1;
	o0.x = DM_INF_F, o0.y = dm_u2f(SRT_HIT_NONE), o0.z = dm_u2f(SRT_HIT_NONE), o0.w = dm_u2f(0xffffffffu); // material -1
	o1.x = 0.0f, o1.y = 0.0f, o1.z = 0.0f, o1.w = dm_u2f(valid ? 0u : SRT_NEAREST_INVALID);
	if (best.shape >= 0) {
		const WinnerRec *__restrict__ wr = p.winners + best.shape;
		int material = wr->material; // a shape without a material is reported, as the cast reports it
		uint32_t tri = SRT_HIT_NONE;
		if (HAS_MODELS && best.rec != SRT_HIT_NONE) {
			tri = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best.rec) : best.rec;
			if (np.tri_materials && material >= 0) { // (uniform over the launch) the cast's rule
				const int tm = np.tri_materials[p.shapes[best.shape].shape.model.triangle_index + tri];
				material = tm >= 0 ? tm : material;
			}
		}
		o0.x = best.d, o0.y = dm_u2f((uint32_t)best.shape), o0.z = dm_u2f(tri), o0.w = dm_u2f((uint32_t)material);
		o1.x = best.px, o1.y = best.py, o1.z = best.pz, o1.w = dm_u2f(SRT_NEAREST_FOUND | best.flags);
	}
	np.out[2u * i] = o0;
	np.out[2u * i + 1u] = o1;
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

int nearest_check(srt_tracer *t, const char *who, size_t n) {
	if (n >= ((size_t)1 << 31)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": n must stay below 2^31 queries");
	return SRT_OK;
}
int nearest_check_skip(srt_tracer *t, const char *who, uint32_t skip_shape) {
	const uint32_t shapes = t->scene_set ? (uint32_t)t->sd.num_shapes : 0u;
	if (skip_shape != SRT_HIT_NONE && skip_shape >= shapes) return fail(t, SRT_ERR_INVALID, std::string(who) + ": skip_shape is not a shape of the scene");
	return SRT_OK;
}

// the query over device arrays, enqueued on the handle's stream (the caller has checked the arguments and set the device)
int enqueue_nearest(srt_tracer *t, const void *queries_dev, size_t n, uint32_t skip_shape, void *out_dev) {
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table as the next dispatch would see it
	NearestParams np;
	memset(&np, 0, sizeof np);
	np.tp = query_scene_params(t);
	np.queries = static_cast<const float4 *>(queries_dev);
	np.out = static_cast<float4 *>(out_dev);
	np.tri_materials = srt_texture_params(t).tri_materials;
	np.n = (uint32_t)n;
	np.skip = skip_shape;
	query_launch(SRT_QUERY_KERNEL(srt_nearest_kernel, np.tp), np, np.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

void nearest_store(const nm_result &r, float *distance, float point[3], uint32_t *flags) {
	*distance = r.distance;
	point[0] = r.px, point[1] = r.py, point[2] = r.pz;
	*flags = r.flags;
}

} // namespace

static_assert(NM_BACK == SRT_NEAREST_BACK && NM_FEATURE_SHIFT == SRT_NEAREST_FEATURE_SHIFT, "nearest_math.h's bits are the record's");

extern "C" {

int srt_nearest_sizes(size_t out[2]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_point_query);
	out[1] = sizeof(srt_nearest);
	return SRT_OK;
}

int srt_nearest_triangle_host(const float wtri[9], const float q[3], float *distance, float point[3], uint32_t *flags) {
	if (!wtri || !q || !distance || !point || !flags) return SRT_ERR_INVALID;
	nearest_store(nm_triangle(wtri[0], wtri[1], wtri[2], wtri[3], wtri[4], wtri[5], wtri[6], wtri[7], wtri[8], q[0], q[1], q[2]), distance, point, flags);
	return SRT_OK;
}

int srt_nearest_sphere_host(const float centre[3], float radius, const float q[3], float *distance, float point[3], uint32_t *flags) {
	if (!centre || !q || !distance || !point || !flags) return SRT_ERR_INVALID;
	nearest_store(nm_sphere(centre[0], centre[1], centre[2], radius, q[0], q[1], q[2]), distance, point, flags);
	return SRT_OK;
}

int srt_nearest_plane_host(const float position[3], const float normal[3], const float q[3], float *distance, float point[3], uint32_t *flags) {
	if (!position || !normal || !q || !distance || !point || !flags) return SRT_ERR_INVALID;
	nearest_store(nm_plane(position[0], position[1], position[2], normal[0], normal[1], normal[2], q[0], q[1], q[2]), distance, point, flags);
	return SRT_OK;
}

int srt_nearest_points_device(srt_tracer *t, const void *queries_dev, size_t n, uint32_t skip_shape, void *out_dev) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = nearest_check(t, "srt_nearest_points_device", n)) return rc;
	if (n == 0) return SRT_OK;
	if (!queries_dev || !out_dev) return fail(t, SRT_ERR_INVALID, "srt_nearest_points_device: NULL array");
	if (((uintptr_t)queries_dev | (uintptr_t)out_dev) & 15u) return fail(t, SRT_ERR_INVALID, "srt_nearest_points_device: arrays must be aligned to 16 bytes");
	if (const int rc = nearest_check_skip(t, "srt_nearest_points_device", skip_shape)) return rc;
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_nearest(t, queries_dev, n, skip_shape, out_dev)) return rc;
	return query_span_end(t);
}

int srt_nearest_points(srt_tracer *t, const srt_point_query *queries, size_t n, uint32_t skip_shape, srt_nearest *out) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = nearest_check(t, "srt_nearest_points", n)) return rc;
	if (n == 0) return SRT_OK;
	if (!queries || !out) return fail(t, SRT_ERR_INVALID, "srt_nearest_points: NULL array");
	if (const int rc = nearest_check_skip(t, "srt_nearest_points", skip_shape)) return rc;
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	const NearestStage ns = nearest_stage(n);
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + ns.points, queries, n * sizeof(srt_point_query), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_nearest(t, stage + ns.points, n, skip_shape, stage + ns.nearest)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(out, stage + ns.nearest, n * sizeof(srt_nearest), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

} // extern "C"
