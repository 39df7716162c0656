// bvh_device.h -- what the kernels that read a model's triangles share (bvh_refit.hip, bvh_build.hip): the bit casts, std::min /
// std::max as the host's builder calls them, floats as order-preserving integers, and BvhBuilder::load's per-triangle box.
#ifndef SRT_BVH_DEVICE_H
#define SRT_BVH_DEVICE_H

#include <hip/hip_runtime.h>

#include "device_types.h"

static __device__ __forceinline__ uint32_t f2u(float f) { return __float_as_uint(f); }
static __device__ __forceinline__ float u2f(uint32_t u) { return __uint_as_float(u); }
// std::min / std::max as the host's builder calls them: the FIRST argument unless the second is strictly beyond it
static __device__ __forceinline__ float min_std(float a, float b) { return b < a ? b : a; }
static __device__ __forceinline__ float max_std(float a, float b) { return a < b ? b : a; }
static __device__ __forceinline__ bool finite_f(float f) { return (f2u(f) & 0x7f800000u) != 0x7f800000u; }

// floats as unsigned integers in the same order (-0 below +0), for atomicMin / atomicMax
static __device__ __forceinline__ uint32_t ordered(float f) {
	const uint32_t u = f2u(f);
	return (u >> 31) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float unordered(uint32_t o) { return u2f((o >> 31) ? (o & 0x7fffffffu) : ~o); }

struct Box {
	float lo[3], hi[3];
};

// BvhBuilder::load's per-triangle part: world vertices in mat_by_vec's unfused order, the box over p0, p1, p2 and the
// kernel's own p0 + (p1 - p0), p0 + (p2 - p0). false: a non-finite bound.
static __device__ __forceinline__ bool triangle_box(const srt_model *m, const srt_triangle *tr, Box &b) {
	const srt_float4 *t = m->transform;
	float p[3][3];
#pragma unroll
	for (int k = 0; k < 3; k++) {
		const srt_float3 v = tr->vertices[k].pos;
		p[k][0] = ((t[0].x * v.x + t[1].x * v.y) + t[2].x * v.z) + t[3].x * 1.0f;
		p[k][1] = ((t[0].y * v.x + t[1].y * v.y) + t[2].y * v.z) + t[3].y * 1.0f;
		p[k][2] = ((t[0].z * v.x + t[1].z * v.y) + t[2].z * v.z) + t[3].z * 1.0f;
	}
	bool finite = true;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const float q1 = p[0][a] + (p[1][a] - p[0][a]), q2 = p[0][a] + (p[2][a] - p[0][a]);
		b.lo[a] = min_std(min_std(min_std(p[0][a], p[1][a]), min_std(p[2][a], q1)), q2);
		b.hi[a] = max_std(max_std(max_std(p[0][a], p[1][a]), max_std(p[2][a], q1)), q2);
		finite = finite && finite_f(b.lo[a]) && finite_f(b.hi[a]);
	}
	return finite;
}

#endif
