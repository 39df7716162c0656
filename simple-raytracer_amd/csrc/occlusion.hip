// occlusion.hip -- occlusion queries behind the ABI (include/srt_abi.h "occlusion queries"): is anything in the handle's scene
// closer than tmax along each caller ray, or between the two ends of each segment. The yes/no form of ray_query.hip's cast: bit
// q of the answer is set exactly when the cast of ray q would set SRT_HIT_HIT. A translation unit of its own: the kernels here
// are new, every kernel the library launched before keeps its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_occlusion_kernel<HAS_MODELS, USE_BVH>: the cast's launch shape (one lane per ray, one wave per workgroup, the lane's
//    BVH stack in scratch), its ray loads and its validity test (ray_valid.inc, one text for both), then the same runs and
//    blocks through the same sphere and plane tests with tmin = tmax -- a lane is occluded as soon as `best >= 0` -- and the
//    any-hit triangle scan and walk of device_anyhit.h. The block test is this kernel's own, not closest_hit.inc: a model is
//    tested against the constant limit by the lanes that still ask. What differs from the cast: lanes past n stay to the end (inactive) because the answer is a ballot; one
//    ballot after each run leaves the run loop when no active lane is still unoccluded; no normal, no material, no record:
//    lane 0 stores the wave's 64 answers as one 64-bit word (and a second one for "invalid" when the caller wants it).
//  * srt_segment_rays_kernel: the srt_ray of a segment, from -> to less end_gap, with the functions the kernels already have.
// The host side's scaffold is query_host.h, shared with ray_query.hip: one staging allocation, one layout (query_stage.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_anyhit.h"
#include "query_host.h"

struct OcclusionParams {
	TraceParams tp;     /* the scene buffers, as a dispatch's (rd: unused) */
	const float4 *rays; /* n srt_ray */
	uint64_t *occluded; /* ceil(n / 64) words */
	uint64_t *invalid;  /* as many, or NULL */
	uint32_t n;
	uint32_t flags; /* SRT_RAYS_* */
};
struct SegmentParams {
	const float4 *segs; /* n srt_segment */
	float4 *rays;       /* n srt_ray */
	uint32_t n;
};

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_occlusion_kernel(const OcclusionParams op) {
	const TraceParams &p = op.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	const bool in = q < op.n; // lanes past n in the last workgroup load nothing and vote 0: they stay for the ballot
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
	if (in) r0 = op.rays[2u * q], r1 = op.rays[2u * q + 1u];
	const f3 org = mk(r0.x, r0.y, r0.z);
	f3 dir = mk(r1.x, r1.y, r1.z);
	const float tmax = r0.w;
	const uint32_t flags = op.flags;
#include "ray_valid.inc"
	const bool active = in && valid && tmax > 0.0f; // (tmax <= 0: nothing is closer than it)
	float tmin = tmax;
	int best = -1;
	if (active) { // (the ballots below are over the lanes in here)
		AnyStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_model = [&](float lx, float ly, float lz, float hx, float hy, float hz, uint32_t ref, uint32_t count, int idx) {
			// only the lanes that still ask: the model's box against the constant limit, then the first triangle closer than it
			if (best < 0 && test_aabb(lx, ly, lz, hx, hy, hz, org, inv, tmax)) {
				const bool occ = USE_BVH ? walk_bvh_any(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, ref, org, dir, tmax SRT_RC_ARG)
				                         : test_triangles_any(p.wtris, ref, count, org, dir, tmax SRT_RC_ARG);
				if (occ) best = idx;
			}
		};
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
				if (((code >> 2) & 7u) <= 2u) test_spheres<2>(b, org, dir, base, tmin, best);
				else test_spheres<4>(b, org, dir, base, tmin, best);
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
				test_planes2(b, (code >> 2) & 7u, org, dir, base, tmin, best);
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				test_model(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], f2u(b.v[3]), f2u(b.v[7]), base);
				if (((code >> 2) & 7u) > 1u) test_model(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], f2u(b.v[11]), f2u(b.v[15]), base + 1);
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
			if (!any64(best < 0)) break; // (wave-uniform) nobody is left to ask
		}
	}
	// ---- the answer: the wave's 64 bits, tail lanes 0 ----
	const unsigned long long occluded = ballot64(active && best >= 0), invalid = ballot64(in && !valid);
	if (threadIdx.x == 0) {
		op.occluded[blockIdx.x] = occluded;
		if (op.invalid) op.invalid[blockIdx.x] = invalid;
	}
}

// The ray of a segment: origin `from`, unit direction towards `to`, tmax = |to - from| - end_gap along that direction. A
// negative or non-finite end_gap and a non-zero `reserved` give tmax = NaN, from == to gives a zero direction, a non-finite end
// a non-finite origin or direction: invalid rays by the cast's own rule.
__global__ __launch_bounds__(64) void srt_segment_rays_kernel(const SegmentParams sp) {
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= sp.n) return;
	const float4 s0 = sp.segs[2u * q], s1 = sp.segs[2u * q + 1u];
	const f3 from = mk(s0.x, s0.y, s0.z), d = mk(s1.x - s0.x, s1.y - s0.y, s1.z - s0.z);
	const float end_gap = s0.w;
	const f3 dir = normalize3(d);
	const bool ok = end_gap >= 0.0f && finite_bits(end_gap) && s1.w == 0.0f;
	float4 r0, r1;
	r0.x = from.x, r0.y = from.y, r0.z = from.z, r0.w = ok ? dot3(d, dir) - end_gap : dm_u2f(0x7fc00000u);
	r1.x = dir.x, r1.y = dir.y, r1.z = dir.z, r1.w = 0.0f;
	sp.rays[2u * q] = r0;
	sp.rays[2u * q + 1u] = r1;
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

// the occlusion launch over device arrays, enqueued on the handle's stream (the caller has checked the arguments and set the device)
int enqueue_occlusion(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *occluded_dev, void *invalid_dev) {
	OcclusionParams op;
	memset(&op, 0, sizeof op);
	op.tp = query_scene_params(t);
	op.rays = static_cast<const float4 *>(rays_dev);
	op.occluded = static_cast<uint64_t *>(occluded_dev);
	op.invalid = static_cast<uint64_t *>(invalid_dev);
	op.n = (uint32_t)n;
	op.flags = flags;
	query_launch(SRT_QUERY_KERNEL(srt_occlusion_kernel, op.tp), op, op.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

int enqueue_segment_rays(srt_tracer *t, const void *segs_dev, size_t n, void *rays_dev) {
	SegmentParams sp;
	sp.segs = static_cast<const float4 *>(segs_dev);
	sp.rays = static_cast<float4 *>(rays_dev);
	sp.n = (uint32_t)n;
	query_launch(srt_segment_rays_kernel, sp, sp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

// the masks of the staged rays back to the host, blocking
int fetch_masks(srt_tracer *t, size_t n, const QueryStage &st, uint64_t *occluded, uint64_t *invalid) {
	const uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(occluded, stage + st.occluded, 8 * query_mask_words(n), hipMemcpyDeviceToHost, t->stream));
	if (invalid) SRT_HIP(t, hipMemcpyAsync(invalid, stage + st.invalid, 8 * query_mask_words(n), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

} // namespace

extern "C" {

int srt_occlusion_sizes(size_t out[2]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_segment);
	out[1] = sizeof(uint64_t);
	return SRT_OK;
}

int srt_occluded_rays_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *occluded_dev, void *invalid_dev) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_occluded_rays_device", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays_dev || !occluded_dev) return fail(t, SRT_ERR_INVALID, "srt_occluded_rays_device: NULL array");
	if (((uintptr_t)rays_dev & 15u) || (((uintptr_t)occluded_dev | (uintptr_t)invalid_dev) & 7u))
		return fail(t, SRT_ERR_INVALID, "srt_occluded_rays_device: rays must be aligned to 16 bytes, masks to 8");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_occlusion(t, rays_dev, n, flags, occluded_dev, invalid_dev)) return rc;
	return query_span_end(t);
}

int srt_occluded_rays(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t flags, uint64_t *occluded, uint64_t *invalid) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_occluded_rays", n, flags)) return rc;
	if (n == 0) return SRT_OK;
	if (!rays || !occluded) return fail(t, SRT_ERR_INVALID, "srt_occluded_rays: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.rays, rays, n * sizeof(srt_ray), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_occlusion(t, stage + st.rays, n, flags, stage + st.occluded, invalid ? stage + st.invalid : nullptr)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	return fetch_masks(t, n, st, occluded, invalid);
}

int srt_occluded_segments(srt_tracer *t, const srt_segment *segs, size_t n, uint64_t *occluded, uint64_t *invalid) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_occluded_segments", n, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!segs || !occluded) return fail(t, SRT_ERR_INVALID, "srt_occluded_segments: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.segs, segs, n * sizeof(srt_segment), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_segment_rays(t, stage + st.segs, n, stage + st.rays)) return rc;
	if (const int rc = enqueue_occlusion(t, stage + st.rays, n, SRT_RAYS_UNIT_DIRECTIONS, stage + st.occluded, invalid ? stage + st.invalid : nullptr)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	return fetch_masks(t, n, st, occluded, invalid);
}

int srt_segment_rays(srt_tracer *t, const srt_segment *segs, size_t n, srt_ray *rays_out) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_segment_rays", n, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!segs || !rays_out) return fail(t, SRT_ERR_INVALID, "srt_segment_rays: NULL array");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.segs, segs, n * sizeof(srt_segment), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_segment_rays(t, stage + st.segs, n, stage + st.rays)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(rays_out, stage + st.rays, n * sizeof(srt_ray), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

} // extern "C"
