// multi_hit.hip -- multi-hit ray queries behind the ABI (include/srt_abi.h "multi-hit ray queries"): the first k candidates
// along each caller ray, in order. A translation unit of its own: the kernels here are new, every kernel the library launched
// before keeps its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_multi_hit{2,4,8}_kernel<HAS_MODELS, USE_BVH>: the cast's launch shape (one lane per ray, one wave per workgroup, the
//    lane's BVH stack in scratch), its ray loads and its validity test (ray_valid.inc), then the same runs and blocks. What
//    differs is what a lane keeps: not one minimum but a sorted list of up to CAP = 2, 4 or 8 entries in registers
//    (device_multihit.h; the caller's k is rounded up to a capacity), fed by per-primitive forms of the sphere and plane tests
//    and by the triangle scan and hierarchy walk without an early exit. A model's box is tested against the caller's tmax, a
//    constant, which is what makes the answer a set over primitives. After the walk the surviving entries become records by
//    the cast's own statements (winner_normal, the per-triangle material rule).
//  * srt_pick_through reuses ray_query.hip's srt_pick_rays_kernel for its rays (srt_enqueue_pick_rays).
// The host side's scaffold is query_host.h, the staging layout query_stage.h's multi_stage.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_shading.h"
#include "device_multihit.h"
#include "query_host.h"

struct MultiHitParams {
	TraceParams tp;               /* the scene buffers, as a dispatch's (rd: unused) */
	const float4 *rays;           /* n srt_ray */
	float4 *hits;                 /* n * k srt_ray_hit */
	uint32_t *counts;             /* n words, or NULL */
	const int32_t *tri_materials; /* per-triangle materials of the scene's triangle array, or NULL */
	uint32_t n;
	uint32_t k;     /* 1 .. CAP of the instantiation */
	uint32_t flags; /* SRT_RAYS_* */
};

template <bool HAS_MODELS, bool USE_BVH, int CAP>
__device__ __forceinline__ void multi_hit_body(const MultiHitParams &mp) {
	const TraceParams &p = mp.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= mp.n) return; // lanes past n in the last workgroup load and store nothing
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	const float4 r0 = mp.rays[2u * q], r1 = mp.rays[2u * q + 1u];
	const f3 org = mk(r0.x, r0.y, r0.z);
	f3 dir = mk(r1.x, r1.y, r1.z);
	const float tmax = r0.w;
	const uint32_t flags = mp.flags, k = mp.k;
	const bool count_all = (flags & SRT_RAYS_COUNT_ALL) != 0u;
#include "ray_valid.inc"
	HitList<CAP> L;
	list_clear(L);
	if (valid && tmax > 0.0f) { // (tmax <= 0: nothing is closer than it)
		AnyStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		const float4 *const blocks = reinterpret_cast<const float4 *>(p.bvh_blocks);
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_model = [&](float lx, float ly, float lz, float hx, float hy, float hz, uint32_t ref, uint32_t count, int idx) {
			// the model's box against the constant limit: which models count does not depend on what was found before
			if (test_aabb(lx, ly, lz, hx, hy, hz, org, inv, tmax)) {
				if (USE_BVH) walk_bvh_multi<CAP>(blocks, bvh_stack, ref, org, dir, (uint32_t)idx, k, tmax, count_all, L SRT_RC_ARG);
				else scan_triangles_multi<CAP>(p.wtris, ref, count, org, dir, (uint32_t)idx, k, tmax, L SRT_RC_ARG);
			}
		};
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u, cnt = (code >> 2) & 7u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
#pragma unroll
				for (int i = 0; i < 4; i++) {
					float t;
					if ((uint32_t)i < cnt && sphere_hit_t(b.v + 4 * i, org, dir, t)) list_offer<CAP, USE_BVH>(L, blocks, k, tmax, t, (uint32_t)(base + i), SRT_HIT_NONE);
				}
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
#pragma unroll
				for (int i = 0; i < 2; i++) {
					float t;
					if ((uint32_t)i < cnt && plane_hit_t(b.v + 8 * i, org, dir, t)) list_offer<CAP, USE_BVH>(L, blocks, k, tmax, t, (uint32_t)(base + i), SRT_HIT_NONE);
				}
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				test_model(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], f2u(b.v[3]), f2u(b.v[7]), base);
				if (cnt > 1u) test_model(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], f2u(b.v[11]), f2u(b.v[15]), base + 1);
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
	// ---- the records: the cast's statements on each surviving entry, the miss record in the other slots ----
	float4 *const out = mp.hits + 2u * (size_t)q * k;
	for (uint32_t j = 0; j < k; j++) { // (wave-uniform)
		float t;
		uint32_t shape, ref;
		list_get(L, j, t, shape, ref);
		float4 h0, h1;
		h0.x = DM_INF_F, h0.y = dm_u2f(SRT_HIT_NONE), h0.z = dm_u2f(SRT_HIT_NONE), h0.w = dm_u2f(0xffffffffu); // material -1
		h1.x = 0.0f, h1.y = 0.0f, h1.z = 0.0f, h1.w = dm_u2f(valid ? 0u : SRT_HIT_INVALID_RAY);
		if (shape != SRT_HIT_NONE) {
			const int best = (int)shape;
			const WinnerRec *__restrict__ wr = p.winners + best;
			int material = wr->material; // a shape without a material is reported, as the cast reports it
			uint32_t tri = SRT_HIT_NONE;
			if (HAS_MODELS && wr->type != SRT_SHAPE_SPHERE && wr->type != SRT_SHAPE_PLANE) {
				tri = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), ref) : ref;
				if (mp.tri_materials && material >= 0) { // (uniform over the launch) the material the trace shades the hit with
					const int tm = mp.tri_materials[p.shapes[best].shape.model.triangle_index + tri];
					material = tm >= 0 ? tm : material;
				}
			}
			f3 nrm = winner_normal<HAS_MODELS, USE_BVH>(p, best, ref, org + dir * t);
			const bool front = dot3(nrm, dir) < 0.0f;
			nrm = nrm * (front ? 1.0f : -1.0f);
			h0.x = t, h0.y = dm_u2f(shape), h0.z = dm_u2f(tri), h0.w = dm_u2f((uint32_t)material);
			h1.x = nrm.x, h1.y = nrm.y, h1.z = nrm.z, h1.w = dm_u2f(SRT_HIT_HIT | (front ? SRT_HIT_FRONT : 0u));
		}
		out[2u * j] = h0;
		out[2u * j + 1u] = h1;
	}
	if (mp.counts) mp.counts[q] = count_all ? L.total : (L.total < k ? L.total : k);
}

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_multi_hit2_kernel(const MultiHitParams mp) {
	multi_hit_body<HAS_MODELS, USE_BVH, 2>(mp);
}
template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_multi_hit4_kernel(const MultiHitParams mp) {
	multi_hit_body<HAS_MODELS, USE_BVH, 4>(mp);
}
template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_multi_hit8_kernel(const MultiHitParams mp) {
	multi_hit_body<HAS_MODELS, USE_BVH, 8>(mp);
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

int multi_check(srt_tracer *t, const char *who, size_t n, uint32_t k, uint32_t flags) {
	if (srt_multi_hit_check_host(k, flags)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": k must be 1 .. 8 and flags known bits");
	return query_check_count(t, who, n, flags & SRT_RAYS_UNIT_DIRECTIONS);
}

// the query over device arrays, enqueued on the handle's stream (the caller has checked the arguments and set the device)
int enqueue_multi(srt_tracer *t, const void *rays_dev, size_t n, uint32_t k, uint32_t flags, void *hits_dev, void *counts_dev) {
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table as the next dispatch would see it
	MultiHitParams mp;
	memset(&mp, 0, sizeof mp);
	mp.tp = query_scene_params(t);
	mp.rays = static_cast<const float4 *>(rays_dev);
	mp.hits = static_cast<float4 *>(hits_dev);
	mp.counts = static_cast<uint32_t *>(counts_dev);
	mp.tri_materials = srt_texture_params(t).tri_materials;
	mp.n = (uint32_t)n;
	mp.k = k;
	mp.flags = flags;
	// the caller's k rounded up to a list capacity
	if (k <= 2u) query_launch(SRT_QUERY_KERNEL(srt_multi_hit2_kernel, mp.tp), mp, mp.n, t->stream);
	else if (k <= 4u) query_launch(SRT_QUERY_KERNEL(srt_multi_hit4_kernel, mp.tp), mp, mp.n, t->stream);
	else query_launch(SRT_QUERY_KERNEL(srt_multi_hit8_kernel, mp.tp), mp, mp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

// the host forms' tail: the records and, if asked for, the counts back from the staging allocation
int read_back(srt_tracer *t, const MultiStage &st, size_t n, uint32_t k, srt_ray_hit *hits, uint32_t *counts) {
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(hits, stage + st.hits, n * k * sizeof(srt_ray_hit), hipMemcpyDeviceToHost, t->stream));
	if (counts) SRT_HIP(t, hipMemcpyAsync(counts, stage + st.counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int reserve_multi(srt_tracer *t, size_t n, uint32_t k, MultiStage *st) {
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // (a grown buffer replaces one a queued launch may still use)
	*st = multi_stage(n, k);
	SRT_HIP(t, t->rq_stage.reserve(st->total));
	return SRT_OK;
}

} // namespace

extern "C" {

int srt_multi_hit_check_host(uint32_t k, uint32_t flags) {
	if (k < 1u || k > SRT_MULTI_HIT_MAX) return SRT_ERR_INVALID;
	if (flags & ~(SRT_RAYS_UNIT_DIRECTIONS | SRT_RAYS_COUNT_ALL)) return SRT_ERR_INVALID;
	return SRT_OK;
}

int srt_multi_hit_sizes(size_t out[3]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_ray);
	out[1] = sizeof(srt_ray_hit);
	out[2] = SRT_MULTI_HIT_MAX;
	return SRT_OK;
}

int srt_cast_rays_multi_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t k, uint32_t flags, void *hits_dev, void *counts_dev) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = multi_check(t, "srt_cast_rays_multi_device", n, k, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays_dev || !hits_dev) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_multi_device: NULL array");
	if ((((uintptr_t)rays_dev | (uintptr_t)hits_dev) & 15u) || ((uintptr_t)counts_dev & 3u))
		return fail(t, SRT_ERR_INVALID, "srt_cast_rays_multi_device: rays and hits must be aligned to 16 bytes, counts to 4");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_multi(t, rays_dev, n, k, flags, hits_dev, counts_dev)) return rc;
	return query_span_end(t);
}

int srt_cast_rays_multi(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t k, uint32_t flags, srt_ray_hit *hits, uint32_t *counts) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = multi_check(t, "srt_cast_rays_multi", n, k, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays || !hits) return fail(t, SRT_ERR_INVALID, "srt_cast_rays_multi: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	MultiStage st;
	if (const int rc = reserve_multi(t, n, k, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.rays, rays, n * sizeof(srt_ray), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_multi(t, stage + st.rays, n, k, flags, stage + st.hits, stage + st.counts)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	return read_back(t, st, n, k, hits, counts);
}

int srt_pick_through(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, uint32_t k, srt_ray_hit *hits, uint32_t *counts) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = multi_check(t, "srt_pick_through", n, k, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!options || !xy || !hits) return fail(t, SRT_ERR_INVALID, "srt_pick_through: NULL argument");
	if (options->width <= 0 || options->height <= 0) return fail(t, SRT_ERR_INVALID, "srt_pick_through: options->width and height must be positive");
	SRT_HIP(t, hipSetDevice(t->device));
	MultiStage st;
	if (const int rc = reserve_multi(t, n, k, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.xy, xy, n * 2 * sizeof(float), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = srt_enqueue_pick_rays(t, options, stage + st.xy, n, stage + st.rays)) return rc;
	if (const int rc = enqueue_multi(t, stage + st.rays, n, k, SRT_RAYS_UNIT_DIRECTIONS, stage + st.hits, stage + st.counts)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	return read_back(t, st, n, k, hits, counts);
}

} // extern "C"
