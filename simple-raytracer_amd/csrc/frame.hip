// frame.hip -- the kernels around the trace launch that work per pixel or per triangle, and their launch wrappers: the
// ordered reduction of a batch's radiances (with the denoiser's moments), the pre-pass that writes world-space triangles,
// and the resolve.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "tonemap.h" // aces1, to_uchar (the resolve), lum (the moments)

// ---------------------------------------------------------------------------------
// Ordered reduction: lane = pixel, serial over the batch's samples in sample order, so
// the float sums are the reference's `color += trace(...)` sequence bit for bit no matter
// which wave traced which sample. 12 B per path in, 16 B RMW per pixel out: HBM-bound.
// ---------------------------------------------------------------------------------
// MOMENTS (denoiser, csrc/denoise.hip): also s2 = sum_k lum(radiance_k)^2 in the same order, carried across batches in
// running.w, and moments[pixel] += s2 / num_samples with the last batch; no fused resolve (the filter resolves). The canvas
// sum is the same either way.
namespace {
__device__ __forceinline__ float add_lum2(float s2, float r, float g, float b) {
	const float l = lum(r, g, b);
	return s2 + l * l;
}
} // namespace
template <bool MOMENTS>
__global__ __launch_bounds__(256) void srt_reduce_kernel(const ReduceParams p) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q == 0u && p.queue_reset) *p.queue_reset = 0ull; // the trace launch this reduction follows is over: its cursor, ready for the next one
	if (q >= p.num_pixels) return;
	f3 c = mk(0.f, 0.f, 0.f);
	float s2 = 0.f;
	float4 *run = reinterpret_cast<float4 *>(p.running) + q;
	if (!p.first_batch) {
		float4 v = *run;
		c = mk(v.x, v.y, v.z);
		if (MOMENTS) s2 = v.w;
	}
	const uint32_t n = p.batch_samples;
	const float *__restrict__ r = p.radiance + (size_t)q * n * 3u;
	uint32_t k = 0;
	if ((n & 3u) == 0u) {
		// 4 samples = 48 B = three aligned 16-byte loads; additions stay in sample order
		const float4 *__restrict__ r4 = reinterpret_cast<const float4 *>(r);
		// SRT_REDUCE_DEPTH x 4 samples per trip: every lane streams its own 12 KB run, so HBM efficiency
		// comes from bytes in flight per lane. Measured at config 2 (25.5 GB): 3 loads per trip 7.16 ms
		// (3.6 TB/s), 12 loads 4.75 ms (5.4 TB/s). The additions stay in sample order.
#ifndef SRT_REDUCE_DEPTH
#define SRT_REDUCE_DEPTH 4
#endif
		for (; k + 4 * SRT_REDUCE_DEPTH <= n; k += 4 * SRT_REDUCE_DEPTH) {
			float4 v[3 * SRT_REDUCE_DEPTH];
#pragma unroll
			for (int i = 0; i < 3 * SRT_REDUCE_DEPTH; i++) v[i] = r4[i];
			r4 += 3 * SRT_REDUCE_DEPTH;
#pragma unroll
			for (int i = 0; i < 3 * SRT_REDUCE_DEPTH; i += 3) {
				const float4 a = v[i], b = v[i + 1], d = v[i + 2];
				c = c + mk(a.x, a.y, a.z);
				if (MOMENTS) s2 = add_lum2(s2, a.x, a.y, a.z);
				c = c + mk(a.w, b.x, b.y);
				if (MOMENTS) s2 = add_lum2(s2, a.w, b.x, b.y);
				c = c + mk(b.z, b.w, d.x);
				if (MOMENTS) s2 = add_lum2(s2, b.z, b.w, d.x);
				c = c + mk(d.y, d.z, d.w);
				if (MOMENTS) s2 = add_lum2(s2, d.y, d.z, d.w);
			}
		}
		for (; k < n; k += 4) {
			const float4 a = r4[0], b = r4[1], d = r4[2];
			r4 += 3;
			c = c + mk(a.x, a.y, a.z);
			if (MOMENTS) s2 = add_lum2(s2, a.x, a.y, a.z);
			c = c + mk(a.w, b.x, b.y);
			if (MOMENTS) s2 = add_lum2(s2, a.w, b.x, b.y);
			c = c + mk(b.z, b.w, d.x);
			if (MOMENTS) s2 = add_lum2(s2, b.z, b.w, d.x);
			c = c + mk(d.y, d.z, d.w);
			if (MOMENTS) s2 = add_lum2(s2, d.y, d.z, d.w);
		}
	} else {
		for (; k < n; k++) {
			c = c + mk(r[3 * k], r[3 * k + 1], r[3 * k + 2]);
			if (MOMENTS) s2 = add_lum2(s2, r[3 * k], r[3 * k + 1], r[3 * k + 2]);
		}
	}
	if (p.last_batch) {
		c = c / (float)p.num_samples; // render.cl:520 (num_samples == 0 -> 0/0 = NaN, as the reference)
		float4 *out = reinterpret_cast<float4 *>(p.canvas) + q;
		float4 o = *out;
		o.x += c.x;
		o.y += c.y;
		o.z += c.z;
		*out = o; // render.cl:522
		if (c.x != c.x || c.y != c.y || c.z != c.z) atomicAdd(&p.counters[SRT_CTR_NAN], 1ull);
		if (!MOMENTS && p.argb) { // the resolve of this pixel (srt_resolve_kernel's expressions on the value just written), fused for srt_render
			const float n = (float)p.num_steps;
			const float r = sqrt_ieee(aces1(o.x / n)), g = sqrt_ieee(aces1(o.y / n)), b = sqrt_ieee(aces1(o.z / n));
			reinterpret_cast<uint32_t *>(p.argb)[q] = 255u | (to_uchar(r * 255.0f) << 8) | (to_uchar(g * 255.0f) << 16) | (to_uchar(b * 255.0f) << 24);
		}
		if (MOMENTS) p.moments[q] += s2 / (float)p.num_samples;
	} else {
		*run = make_float4(c.x, c.y, c.z, MOMENTS ? s2 : 0.f);
	}
}

// ---------------------------------------------------------------------------------
// Pre-pass: world-space triangles per model instance. blockIdx.y = shape.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void srt_prepass_kernel(const PrepassParams p) {
	const int si = blockIdx.y;
	if (si >= p.num_shapes) return;
	const srt_shape *sh = p.shapes + si;
	if (sh->type != SRT_SHAPE_MODEL) return;
	const srt_model *m = &sh->shape.model;
	const uint32_t n = m->num_triangles;
	const uint32_t base = p.wtri_offset[si];
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n; s += gridDim.x * blockDim.x) {
		const uint32_t j = p.order ? p.order[base + s] : s; // BVH layout: record s of the model holds its triangle order[s]
		const srt_triangle *t = p.triangles + (m->triangle_index + j);
		// render.cl:325-328 then :247-248
		f3 p0 = mat_by_vec(m->transform, ld3(t->vertices[0].pos), 1.0f);
		f3 p1 = mat_by_vec(m->transform, ld3(t->vertices[1].pos), 1.0f);
		f3 p2 = mat_by_vec(m->transform, ld3(t->vertices[2].pos), 1.0f);
		f3 e1 = p1 - p0, e2 = p2 - p0;
		// BVH layout: record base + s lives in slot (dest & 3) of leaf block (dest >> 2)
		float *w = p.order ? p.wtris + (size_t)(p.dest[base + s] >> 2) * 32u + (p.dest[base + s] & 3u) * SRT_BVH_TRI_FLOATS
		                   : p.wtris + (size_t)(base + s) * SRT_WTRI_FLOATS;
		w[0] = p0.x, w[1] = p0.y, w[2] = p0.z;
		w[3] = e1.x, w[4] = e1.y, w[5] = e1.z;
		w[6] = e2.x, w[7] = e2.y, w[8] = e2.z;
		if (p.order) p.wtris[(size_t)(p.dest[base + s] >> 2) * 32u + SRT_BVH_LEAF_J + (p.dest[base + s] & 3u)] = dm_u2f(j);
	}
}

// ---------------------------------------------------------------------------------
// Resolve: canvas / num_steps -> ACES -> sqrt -> A,R,G,B bytes (render.cl:473-481,525-535)
// 16 B in, 4 B out per pixel; HBM-bound.
// ---------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void srt_resolve_kernel(const ResolveParams p) {
	const float4 *__restrict__ canvas = reinterpret_cast<const float4 *>(p.canvas);
	uint32_t *__restrict__ out = reinterpret_cast<uint32_t *>(p.argb);
	const float n = (float)p.num_steps;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.num_pixels; i += gridDim.x * blockDim.x) {
		float4 c = canvas[i];
		float r = sqrt_ieee(aces1(c.x / n));
		float g = sqrt_ieee(aces1(c.y / n));
		float b = sqrt_ieee(aces1(c.z / n));
		// memory order A, R, G, B (little endian word)
		out[i] = 255u | (to_uchar(r * 255.0f) << 8) | (to_uchar(g * 255.0f) << 16) | (to_uchar(b * 255.0f) << 24);
	}
}

void srt_launch_reduce(const ReduceParams &p, void *stream) {
	if (p.num_pixels == 0) return;
	hipLaunchKernelGGL(srt_reduce_kernel<false>, dim3((p.num_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
}

void srt_launch_prepass(const PrepassParams &p, uint64_t max_tris_per_model, void *stream) {
	if (p.num_shapes <= 0 || max_tris_per_model == 0) return;
	unsigned gx = (unsigned)((max_tris_per_model + 255) / 256);
	if (gx > 4096) gx = 4096;
	dim3 grid(gx, (unsigned)p.num_shapes), block(256);
	hipLaunchKernelGGL(srt_prepass_kernel, grid, block, 0, (hipStream_t)stream, p);
}

void srt_launch_resolve(const ResolveParams &p, void *stream) {
	if (p.num_pixels == 0) return;
	unsigned gx = (p.num_pixels + 255) / 256;
	if (gx > 4096) gx = 4096;
	hipLaunchKernelGGL(srt_resolve_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, p);
}

void srt_launch_reduce_moments(const ReduceParams &p, void *stream) {
	if (p.num_pixels == 0) return;
	hipLaunchKernelGGL(srt_reduce_kernel<true>, dim3((p.num_pixels + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
}
