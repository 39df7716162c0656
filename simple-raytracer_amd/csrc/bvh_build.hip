// bvh_build.hip -- a model's hierarchy built on the device (include/srt_abi.h SRT_BUILD_DEVICE): the ORDER of its triangles. The
// topology is the host's balanced one, a function of the count alone (bvh_host.cpp balanced_topology), and every box is the
// refit's (bvh_refit.hip). What is computed here is what BvhBuilder::morton_order gives on the host, bit for bit:
//   keys     one thread per record, after the extents pass over the identity order: the triangle's unpadded box, its centroid,
//            the 30-bit Morton code between the model's extents (a non-finite triangle: 0x40000000)
//   sort     a stable least-significant-digit radix sort of the records by code, 8 bits a pass, four passes, starting from the
//            identity order -- which makes the result the order by (code, index). Per pass three launches:
//              histogram  one workgroup per tile of SRT_BUILD_TILE records: the tile's digit counts, in LDS, into the table
//              scan       one workgroup per model: the exclusive prefix over the table, digit-major (digit d of tile t comes
//                         behind every smaller digit and behind digit d of the tiles before t)
//              scatter    one workgroup per tile, four rounds of 256 records: a record's rank among the equal digits of its
//                         wave by eight ballots, the waves before it from LDS counters, the rounds before it from the running
//                         offsets that start at the table's entry
//            The last pass writes the triangle indices into the scene's order array.
// blockIdx.y = model. Why the codes agree with the host's: the transform, the centroid and the quantisation are written in the
// host's operation order and compiled with -ffp-contract=off, the division is the correctly rounded one; the extents are a
// minimum and a maximum, whose value does not depend on the order (the sign of a zero can, and no code depends on it: c - mlo
// and mhi - mlo have the same value for either zero, and a zero difference gives cell 0 either way).
// Launch- and latency-bound like the refit (10^5 triangles: 98 tiles, a table of 25k counters); nothing waits for another
// workgroup, the order is the stream's. LDS: 1 KB (histogram), 5 KB (scatter); register use is small, occupancy is not a
// concern at these grid sizes. The one-workgroup scan is the serial part: 256 x tiles counters, 1,024 per step.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "bvh_device.h"
#include "device_types.h"

static_assert(SRT_BUILD_TILE % 256u == 0u, "a tile is a whole number of rounds of 256 records");

// BvhBuilder::morton_code (bvh_host.cpp), operation for operation
static __device__ __forceinline__ uint32_t morton_code(const float *c, const float *mlo, const float *mhi) {
	uint32_t q[3];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		q[a] = 0u;
		const float ext = mhi[a] - mlo[a];
		if (!(ext > 0.0f) || !finite_f(ext)) continue;
		const float f = (c[a] - mlo[a]) * (1024.0f / ext);
		q[a] = f >= 1023.0f ? 1023u : (f > 0.0f ? (uint32_t)(int)f : 0u);
	}
	uint32_t code = 0u;
#pragma unroll
	for (int i = 0; i < 10; i++) code |= (((q[0] >> i) & 1u) << (3 * i + 2)) | (((q[1] >> i) & 1u) << (3 * i + 1)) | (((q[2] >> i) & 1u) << (3 * i));
	return code;
}

__global__ __launch_bounds__(256) void srt_build_keys_kernel(const BuildParams p) {
	const RefitModel rm = p.models[blockIdx.y];
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	const uint32_t *ext = p.extents + 6u * blockIdx.y;
	float mlo[3], mhi[3];
#pragma unroll
	for (int a = 0; a < 3; a++) mlo[a] = unordered(ext[a]), mhi[a] = unordered(ext[3 + a]);
	for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < rm.num_records; s += gridDim.x * blockDim.x) {
		Box b; // record s holds triangle s: the sort starts from the identity order
		uint32_t code = 0x40000000u;
		if (triangle_box(m, p.triangles + (m->triangle_index + s), b)) {
			float c[3];
#pragma unroll
			for (int a = 0; a < 3; a++) c[a] = 0.5f * b.lo[a] + 0.5f * b.hi[a];
			code = morton_code(c, mlo, mhi);
		}
		p.keys[0][rm.first_record + s] = code;
	}
}

// ---- the sort ---------------------------------------------------------------------------------------------------------------
// A model's table: counter (digit d, tile t) at table[256 * first_tile + d * tiles + t].

__global__ __launch_bounds__(256) void srt_build_hist_kernel(const BuildParams p, const uint32_t *__restrict__ keys, uint32_t shift) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t tiles = SRT_BUILD_TILES(rm.num_records), tile = blockIdx.x;
	if (tile >= tiles) return; // (the whole workgroup: the grid is the largest model's)
	__shared__ uint32_t hist[256];
	hist[threadIdx.x] = 0u;
	__syncthreads();
	for (uint32_t r = 0; r < SRT_BUILD_TILE / 256u; r++) {
		const uint32_t s = tile * SRT_BUILD_TILE + r * 256u + threadIdx.x;
		if (s < rm.num_records) atomicAdd(&hist[(keys[rm.first_record + s] >> shift) & 255u], 1u);
	}
	__syncthreads();
	p.table[256u * (size_t)rm.first_tile + (size_t)threadIdx.x * tiles + tile] = hist[threadIdx.x];
}

// the exclusive prefix of `v` over the workgroup's 256 threads, and in `total` the sum over all of them
static __device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total) {
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t x = v;
	for (uint32_t off = 1; off < 64u; off <<= 1) {
		const uint32_t y = __shfl_up(x, off);
		if (lane >= off) x += y;
	}
	if (lane == 63u) wave_sums[wave] = x;
	__syncthreads();
	uint32_t before = 0u;
	total = 0u;
#pragma unroll
	for (uint32_t w = 0; w < 4u; w++) {
		const uint32_t ws = wave_sums[w];
		if (w < wave) before += ws;
		total += ws;
	}
	__syncthreads(); // (wave_sums is written again by the next step)
	return before + x - v;
}

__global__ __launch_bounds__(256) void srt_build_scan_kernel(const BuildParams p) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t n = 256u * SRT_BUILD_TILES(rm.num_records);
	uint32_t *tab = p.table + 256u * (size_t)rm.first_tile;
	__shared__ uint32_t wave_sums[4];
	uint32_t carry = 0u;
	for (uint32_t base = 0; base < n; base += 1024u) { // (n, and with it the trip count, is the workgroup's)
		const uint32_t i0 = base + 4u * threadIdx.x;
		uint32_t v[4], sum = 0u;
#pragma unroll
		for (uint32_t k = 0; k < 4u; k++) v[k] = i0 + k < n ? tab[i0 + k] : 0u, sum += v[k];
		uint32_t total;
		uint32_t at = carry + block_exclusive_scan(sum, wave_sums, total);
#pragma unroll
		for (uint32_t k = 0; k < 4u; k++) {
			if (i0 + k < n) tab[i0 + k] = at;
			at += v[k];
		}
		carry += total;
	}
}

// src_vals == NULL: the identity (the first pass)
__global__ __launch_bounds__(256) void srt_build_scatter_kernel(const BuildParams p, const uint32_t *__restrict__ src_keys, const uint32_t *__restrict__ src_vals,
                                                                uint32_t *__restrict__ dst_keys, uint32_t *__restrict__ dst_vals, uint32_t shift) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t tiles = SRT_BUILD_TILES(rm.num_records), tile = blockIdx.x;
	if (tile >= tiles) return; // (the whole workgroup)
	__shared__ uint32_t running[256]; // where the next record of each digit goes, relative to the model's first record
	__shared__ uint32_t count[4][256]; // per wave of the round: how many of each digit
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	running[threadIdx.x] = p.table[256u * (size_t)rm.first_tile + (size_t)threadIdx.x * tiles + tile];
#pragma unroll
	for (uint32_t w = 0; w < 4u; w++) count[w][threadIdx.x] = 0u;
	__syncthreads();
	for (uint32_t r = 0; r < SRT_BUILD_TILE / 256u; r++) { // (every thread takes every round: the barriers are the workgroup's)
		const uint32_t s = tile * SRT_BUILD_TILE + r * 256u + threadIdx.x;
		const bool valid = s < rm.num_records;
		const uint32_t key = valid ? src_keys[rm.first_record + s] : 0u;
		const uint32_t d = (key >> shift) & 255u;
		// the lanes of this wave with a record of the same digit
		unsigned long long same = __ballot(valid);
#pragma unroll
		for (uint32_t bit = 0; bit < 8u; bit++) {
			const bool one = (d >> bit) & 1u;
			const unsigned long long b = __ballot(one);
			same &= one ? b : ~b;
		}
		const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
		if (valid && rank == 0u) count[wave][d] = (uint32_t)__popcll(same);
		__syncthreads();
		if (valid) {
			uint32_t pos = running[d] + rank;
#pragma unroll
			for (uint32_t w = 0; w < 4u; w++)
				if (w < wave) pos += count[w][d];
			if (pos < rm.num_records) { // (always, when the table is this pass's histogram: nothing is ever written outside the model)
				dst_keys[rm.first_record + pos] = key;
				dst_vals[rm.first_record + pos] = src_vals ? src_vals[rm.first_record + s] : s;
			}
		}
		__syncthreads();
		running[threadIdx.x] += count[0][threadIdx.x] + count[1][threadIdx.x] + count[2][threadIdx.x] + count[3][threadIdx.x];
#pragma unroll
		for (uint32_t w = 0; w < 4u; w++) count[w][threadIdx.x] = 0u;
		__syncthreads();
	}
}

// blockIdx.y = model: slabs of 65535 (the models' table offsets are absolute)
template <class Launch>
static int per_slab(const BuildParams &p, uint32_t num_models, Launch launch) {
	int launches = 0;
	for (uint32_t base = 0; base < num_models; base += 65535u) {
		BuildParams q = p;
		q.models += base, q.extents += 6u * (size_t)base;
		launch(q, num_models - base > 65535u ? 65535u : num_models - base);
		launches++;
	}
	return launches;
}

int srt_launch_build_keys(const BuildParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	const uint32_t gx = max_records ? (max_records + 255u) / 256u : 1u;
	return per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_keys_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q); });
}

int srt_launch_build_sort(const BuildParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	const uint32_t gx = max_records ? SRT_BUILD_TILES(max_records) : 1u;
	int launches = 0;
	for (uint32_t pass = 0; pass < (uint32_t)SRT_BUILD_SORT_PASSES; pass++) {
		const uint32_t shift = 8u * pass, from = pass & 1u, to = from ^ 1u;
		const uint32_t *src_vals = pass == 0u ? nullptr : p.vals[from];
		uint32_t *dst_vals = pass + 1u == (uint32_t)SRT_BUILD_SORT_PASSES ? p.order : p.vals[to];
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_hist_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, q.keys[from], shift); });
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_scan_kernel, dim3(1, cnt), dim3(256), 0, (hipStream_t)stream, q); });
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) {
			hipLaunchKernelGGL(srt_build_scatter_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, q.keys[from], src_vals, q.keys[to], dst_vals, shift);
		});
	}
	return launches;
}
