// bvh_refit.hip -- the in-place refit of moved models' hierarchies on the device (include/srt_abi.h SRT_REFIT_DEVICE): what
// BvhCacheEntry::refit_in_place (bvh_host.cpp: BvhBuilder::load + refit + quantise_body) computes on the host, bit for bit.
//   pass A  one thread per record: the triangle's unpadded world box, reduced to the model's extents over its finite triangles
//   pass B  one thread per record, the one in slot 0 works: the pad from the extents, the padded boxes of the leaf block's
//           1-3 records, their union into boxes[leaf block]
//   pass C  one launch per height level, ascending, one thread per inner block: the children's boxes from `boxes`, the block's
//           own box (their union) into `boxes`, dwords 0-9 of the block requantised (3 keeps its child count; 10, 11 stay)
// Why the bits agree: min and max are exact, so a union does not depend on how it is bracketed -- the binary hierarchy's box of
// a wide block's child is the union over the same triangles as the union over that child's own children here. (No NaN reaches
// a union: non-finite triangles get the all-embracing box. A lower bound is never -0 and an upper bound never +0, see
// step_down / step_up, so equal values have equal bits.) Everything that rounds -- the transform, the pad, the quantiser -- is
// written in the host's operation order and compiled, like the host's, with -ffp-contract=off; float division and the double
// square root are the correctly rounded ones. The kernels are launch- and latency-bound (10^5 triangles: 22k inner blocks,
// a dozen levels); nothing here waits for another workgroup: the order is the stream's.
// Behind pass C, under SRT_DEFORM_REFIT only, one more launch measures the refitted hierarchy: srt_refit_cost_kernel, below.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bvh_device.h"
#include "device_types.h"

// nextafterf(x, -INFINITY) / nextafterf(x, +INFINITY) as a step on the bit pattern. Domain: every float except NaN (the
// callers pass finite - finite, which is never NaN). +-0 step to the smallest denormal of the direction's sign; a step
// off +-FLT_MAX gives the infinity, which then stays; stepping UP from the smallest negative denormal gives -0 and DOWN
// from the smallest positive one +0, as glibc's does.
static __device__ __forceinline__ float step_down(float x) {
	const uint32_t u = f2u(x);
	if ((u & 0x7fffffffu) == 0u) return u2f(0x80000001u);
	if (u == 0xff800000u) return x;
	return u2f((u >> 31) ? u + 1u : u - 1u);
}
static __device__ __forceinline__ float step_up(float x) {
	const uint32_t u = f2u(x);
	if ((u & 0x7fffffffu) == 0u) return u2f(0x00000001u);
	if (u == 0x7f800000u) return x;
	return u2f((u >> 31) ? u - 1u : u + 1u);
}

// ---- pass A -------------------------------------------------------------------------------------------------------------
// blockIdx.y = refitted model. The extents are a minimum and a maximum over finite values: any order gives the same value
// (the sign of a zero aside, which the pad's squares do not see), so a wave reduction and one atomic per wave and bound do.
__global__ __launch_bounds__(256) void srt_refit_extents_kernel(const RefitParams p) {
	const RefitModel rm = p.models[blockIdx.y];
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < rm.num_records; s += gridDim.x * blockDim.x) {
		const uint32_t j = p.order[rm.first_record + s];
		Box b;
		if (!triangle_box(m, p.triangles + (m->triangle_index + j), b)) continue;
#pragma unroll
		for (int a = 0; a < 3; a++) lo[a] = fminf(lo[a], b.lo[a]), hi[a] = fmaxf(hi[a], b.hi[a]);
	}
#pragma unroll
	for (int a = 0; a < 3; a++)
		for (int off = 32; off > 0; off >>= 1) lo[a] = fminf(lo[a], __shfl_xor(lo[a], off)), hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
	if ((threadIdx.x & 63u) == 0u && lo[0] <= hi[0]) { // (a wave without a finite triangle has nothing to add)
		uint32_t *ext = p.extents + 6u * blockIdx.y;
#pragma unroll
		for (int a = 0; a < 3; a++) atomicMin(ext + a, ordered(lo[a])), atomicMax(ext + 3 + a, ordered(hi[a]));
	}
}

// load()'s pad: 2^-12 of the diagonal of the model's extents, in double, the axes without a finite triangle left out
static __device__ __forceinline__ float model_pad(const uint32_t *ext) {
	double d2 = 0.0;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const float mlo = unordered(ext[a]), mhi = unordered(ext[3 + a]);
		if (mhi >= mlo) d2 += ((double)mhi - (double)mlo) * ((double)mhi - (double)mlo);
	}
	const double r = __builtin_sqrt(d2) * (1.0 / 4096.0); // (the correctly rounded double square root)
	return (float)((double)FLT_MAX < r ? (double)FLT_MAX : r);
}

// ---- pass B -------------------------------------------------------------------------------------------------------------
// A leaf block's records are consecutive and sit in its slots 0, 1, 2 in that order (fold_node): the thread of the record in
// slot 0 takes the records behind it for as long as they are in the same block.
__global__ __launch_bounds__(256) void srt_refit_leaves_kernel(const RefitParams p) {
	const RefitModel rm = p.models[blockIdx.y];
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	const float pad = model_pad(p.extents + 6u * blockIdx.y);
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < rm.num_records; s += gridDim.x * blockDim.x) {
		const uint32_t d = p.dest[rm.first_record + s];
		if (d & 3u) continue;
		const uint32_t blk = d >> 2;
		float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
		for (uint32_t k = 0; k < (uint32_t)SRT_BVH_LEAF_MAX && s + k < rm.num_records; k++) {
			if ((p.dest[rm.first_record + s + k] >> 2) != blk) break;
			const uint32_t j = p.order[rm.first_record + s + k];
			Box b;
			if (!triangle_box(m, p.triangles + (m->triangle_index + j), b)) // hostile input: a box every ray enters
				for (int a = 0; a < 3; a++) b.lo[a] = -FLT_MAX, b.hi[a] = FLT_MAX;
#pragma unroll
			for (int a = 0; a < 3; a++) {
				if (b.lo[a] != -FLT_MAX) { // widen by the pad plus two ulps; stays finite
					b.lo[a] = max_std(-FLT_MAX, step_down(step_down(b.lo[a] - pad)));
					b.hi[a] = min_std(FLT_MAX, step_up(step_up(b.hi[a] + pad)));
				}
				lo[a] = min_std(lo[a], b.lo[a]), hi[a] = max_std(hi[a], b.hi[a]);
			}
		}
		float *out = p.boxes + 6u * (size_t)blk;
#pragma unroll
		for (int a = 0; a < 3; a++) out[a] = lo[a], out[3 + a] = hi[a];
	}
}

// ---- pass C -------------------------------------------------------------------------------------------------------------
// frexp's exponent of x >= 0 on the bits: x = m * 2^ex with m in [0.5, 1); 0 for x == 0, as the C library's
static __device__ __forceinline__ int frexp_exponent(float x) {
	const uint32_t u = f2u(x), ef = (u >> 23) & 255u, man = u & 0x007fffffu;
	if (ef == 0u) return man ? (31 - __clz((int)man)) - 148 : 0; // a denormal man * 2^-149, highest bit h: 0.1.. * 2^(h - 148)
	return (int)ef - 126;
}

// quantise_body (bvh_host.cpp), one axis: the children's bounds lo[k], hi[k], k < nk -> origin, biased exponent, lo and hi bytes
static __device__ __forceinline__ void quantise_axis(const float *lo, const float *hi, uint32_t nk, float &origin_out, uint32_t &expo, uint32_t &wlo, uint32_t &whi, float &top_out, float &min_out) {
	float origin = FLT_MAX, top = -FLT_MAX;
#pragma unroll
	for (uint32_t k = 0; k < 4; k++)
		if (k < nk) origin = min_std(origin, lo[k]), top = max_std(top, hi[k]);
	min_out = origin, top_out = top;
	if (!(origin == origin)) origin = -FLT_MAX;
	int e = -126;
	const float extent = top - origin;
	if (extent > 0.0f) {
		const int ex = frexp_exponent(extent / 255.0f); // (an IEEE quotient: build.py keeps the correctly rounded division)
		e = finite_f(extent) ? ex : 126;
	}
	wlo = 0u, whi = 0u; // bytes of an earlier, coarser-to-be round stay where a round stops short, as the host's arrays do
	for (;; e++) {
		if (e < -126) e = -126;
		if (e > 127) e = 127;
		const float scale = u2f((uint32_t)(e + 127) << 23);
		const double inv_scale = __longlong_as_double((long long)(1023 - e) << 52); // 2^-e, exact
		bool fits = true;
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			if (k >= nk || !fits) continue;
			const double fl = ((double)lo[k] - (double)origin) * inv_scale;
			int ql = fl >= 255.0 ? 255 : (fl > 0.0 ? (int)fl : 0);
			while (ql > 0 && !(__builtin_fmaf((float)ql, scale, origin) <= lo[k])) ql--;
			const double fh = ((double)hi[k] - (double)origin) * inv_scale;
			int qh = fh > 255.0 ? 256 : (fh > 0.0 ? (int)fh + ((double)(int)fh < fh ? 1 : 0) : 0);
			if (!(fh == fh)) qh = 256;
			while (qh <= 255 && !(__builtin_fmaf((float)qh, scale, origin) >= hi[k])) qh++;
			if (qh > 255) fits = false;
			wlo = (wlo & ~(255u << (8 * k))) | ((uint32_t)ql << (8 * k));
			whi = (whi & ~(255u << (8 * k))) | ((uint32_t)(qh & 255) << (8 * k));
		}
		if (fits || e == 127) {
			if (!fits) whi = 0xffffffffu;
			expo = (uint32_t)(e + 127);
			break;
		}
	}
	// empty slots: lo above hi (the walk counts the slots)
	const uint32_t used = nk >= 4u ? 0xffffffffu : ((1u << (8 * nk)) - 1u);
	wlo = (wlo & used) | ~used;
	whi = whi & used;
	origin_out = origin;
}

__global__ __launch_bounds__(256) void srt_refit_level_kernel(const RefitParams p, uint32_t first, uint32_t count) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= count) return;
	const uint32_t blk = p.sched[first + i];
	uint32_t *b = p.blocks + 32u * (size_t)blk;
	const uint32_t nk = b[3] >> 24, child0 = b[SRT_BVH_FIRST_DWORD];
	float lo[3][4], hi[3][4];
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		const float *c = p.boxes + 6u * (size_t)(child0 + (k < nk ? k : 0u)); // (an empty slot re-reads child 0; never used)
#pragma unroll
		for (int a = 0; a < 3; a++) lo[a][k] = c[a], hi[a][k] = c[3 + a];
	}
	float *own = p.boxes + 6u * (size_t)blk;
	uint32_t expo[3];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		float origin, top, low;
		uint32_t wlo, whi;
		quantise_axis(lo[a], hi[a], nk, origin, expo[a], wlo, whi, top, low);
		own[a] = low, own[3 + a] = top;
		b[a] = f2u(origin), b[4 + a] = wlo, b[7 + a] = whi;
	}
	b[3] = expo[0] | (expo[1] << 8) | (expo[2] << 16) | (nk << 24);
}

// ---- the cost of the refitted hierarchy (include/srt_abi.h SRT_DEFORM_REFIT) ----------------------------------------------------
// BvhBuilder::half_area_d (bvh_host.h), operation for operation: -ffp-contract=off keeps the products and sums apart
static __device__ __forceinline__ double half_area_d(const float *box) {
	const double dx = (double)box[3] - (double)box[0], dy = (double)box[4] - (double)box[1], dz = (double)box[5] - (double)box[2];
	return dx * dy + dy * dz + dz * dx;
}

// blockIdx.y = refitted model, a grid-stride loop over its blocks: after pass C `boxes` holds every one's padded box, `weights`
// what the box counts for (an inner block's children, a leaf block's triangles). Every term is what BvhBuilder::wide_cost forms
// on the host; the order of the sum is not (lanes, waves, atomics), which a sum of non-negative doubles forgives to one
// rounding per term. One wave: a butterfly over its 64 lanes, one atomic add. The root is the model's first block; whoever
// meets it stores its H beside the sum. Nothing is read outside [first_block, first_block + num_blocks).
__global__ __launch_bounds__(256) void srt_refit_cost_kernel(const float *__restrict__ boxes, const uint8_t *__restrict__ weights, const RefitCostRange *__restrict__ ranges, double *sums) {
	const RefitCostRange r = ranges[blockIdx.y];
	double sum = 0.0;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < r.num_blocks; i += gridDim.x * blockDim.x) {
		const size_t b = (size_t)r.first_block + i;
		const double h = half_area_d(boxes + 6u * b);
		sum += h * (double)weights[b];
		if (i == 0u) sums[2u * blockIdx.y + 1u] = h;
	}
	for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
	if ((threadIdx.x & 63u) == 0u && sum != 0.0) atomicAdd(sums + 2u * blockIdx.y, sum); // (NaN != 0: a non-finite term arrives)
}

int srt_launch_refit_cost(const float *boxes, const uint8_t *weights, const RefitCostRange *ranges, double *sums, uint32_t num_models, uint32_t max_blocks, void *stream) {
	int launches = 0;
	const uint32_t want = max_blocks ? (max_blocks + 255u) / 256u : 1u;
	const uint32_t gx = want > 64u ? 64u : want; // (64 workgroups of 256 stride over the largest models: 256 atomics per model at the most)
	for (uint32_t base = 0; base < num_models; base += 65535u) {
		const uint32_t cnt = num_models - base > 65535u ? 65535u : num_models - base;
		hipLaunchKernelGGL(srt_refit_cost_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, boxes, weights, ranges + base, sums + 2u * (size_t)base);
		launches++;
	}
	return launches;
}

// blockIdx.y = model: slabs of 65535
template <class K>
static int launch_per_record(K kernel, const RefitParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	int launches = 0;
	const uint32_t gx = max_records ? (max_records + 255u) / 256u : 1u;
	for (uint32_t base = 0; base < num_models; base += 65535u) {
		RefitParams q = p;
		q.models += base, q.extents += 6u * (size_t)base;
		const uint32_t cnt = num_models - base > 65535u ? 65535u : num_models - base;
		hipLaunchKernelGGL(kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q);
		launches++;
	}
	return launches;
}

int srt_launch_refit_extents(const RefitParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	return launch_per_record(srt_refit_extents_kernel, p, num_models, max_records, stream);
}
int srt_launch_refit_leaves(const RefitParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	return launch_per_record(srt_refit_leaves_kernel, p, num_models, max_records, stream);
}
int srt_launch_refit_level(const RefitParams &p, uint32_t first, uint32_t count, void *stream) {
	if (count == 0u) return 0;
	hipLaunchKernelGGL(srt_refit_level_kernel, dim3((count + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, p, first, count);
	return 1;
}
