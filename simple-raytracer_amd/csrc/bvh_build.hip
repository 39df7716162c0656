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
// The MEDIAN order (include/srt_abi.h SRT_BUILD_ORDER_MEDIAN; BvhBuilder::median_order on the host, bit for bit) is at the end of
// this file: the balanced topology's ranges, top-down, each sorted stably by a 17-bit key along the widest axis of its centroids.
//   global levels  while a depth's largest range exceeds SRT_BUILD_LOCAL records: a launch for every range's centroid extents
//                  (wave shuffles, then LDS, then at most twelve atomics per workgroup and range: a tile touches two ranges), a
//                  launch for the composite keys (range << 17 | key), and the sort above over ceil((17 + depth) / 8) digits
//   local finish   one launch, one workgroup per range of the first depth whose ranges all fit: centroids, a permutation and
//                  the keys in LDS (30 KB), all remaining depths there -- extents by LDS atomics, keys, and a record's rank
//                  inside its sub-range by counting the smaller (key, position) composites, which are unique
// Models of one update differ in depth: a workgroup of a model that takes no part in a level returns whole. A model of more
// than SRT_BUILD_LOCAL << 15 triangles (a sixteenth global level: the composite key has 32 bits) keeps the Morton order.
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
// The models a launch is for: those of more than `above` and at most `upto` records (the Morton order: all of them; a global
// level of the median order: those whose ranges at that depth are still too large for the local launch).
struct SortTake {
	uint32_t above, upto;
	__device__ __forceinline__ bool operator()(uint32_t n) const { return n > above && n <= upto; }
};

__global__ __launch_bounds__(256) void srt_build_hist_kernel(const BuildParams p, const uint32_t *__restrict__ keys, uint32_t shift, const SortTake take) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t tiles = SRT_BUILD_TILES(rm.num_records), tile = blockIdx.x;
	if (tile >= tiles || !take(rm.num_records)) return; // (the whole workgroup: the grid is the largest model's)
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

__global__ __launch_bounds__(256) void srt_build_scan_kernel(const BuildParams p, const SortTake take) {
	const RefitModel rm = p.models[blockIdx.y];
	if (!take(rm.num_records)) return; // (the whole workgroup)
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
                                                                uint32_t *__restrict__ dst_keys, uint32_t *__restrict__ dst_vals, uint32_t shift, const SortTake take) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t tiles = SRT_BUILD_TILES(rm.num_records), tile = blockIdx.x;
	if (tile >= tiles || !take(rm.num_records)) return; // (the whole workgroup)
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
		if (q.range_first) q.range_first += base;
		launch(q, num_models - base > 65535u ? 65535u : num_models - base);
		launches++;
	}
	return launches;
}

int srt_launch_build_keys(const BuildParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	const uint32_t gx = max_records ? (max_records + 255u) / 256u : 1u;
	return per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_keys_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q); });
}

// `passes` stable passes over the low 8 * passes bits of keys[cur], for the models `take` takes: keys[cur] / vals[cur] -> the other
// side and back, `cur` ends on the side that holds the result. identity: vals[cur] is not there yet, record s holds triangle s.
// last_vals: where the last pass writes the indices instead (the scene's order array).
static int sort_passes(const BuildParams &p, uint32_t num_models, uint32_t gx, void *stream, uint32_t passes, uint32_t &cur, bool identity, uint32_t *last_vals, const SortTake take) {
	int launches = 0;
	for (uint32_t pass = 0; pass < passes; pass++) {
		const uint32_t shift = 8u * pass, from = cur, to = cur ^ 1u;
		const uint32_t *src_vals = identity && pass == 0u ? nullptr : p.vals[from];
		uint32_t *dst_vals = last_vals && pass + 1u == passes ? last_vals : p.vals[to];
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_hist_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, q.keys[from], shift, take); });
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_scan_kernel, dim3(1, cnt), dim3(256), 0, (hipStream_t)stream, q, take); });
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) {
			hipLaunchKernelGGL(srt_build_scatter_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, q.keys[from], src_vals, q.keys[to], dst_vals, shift, take);
		});
		cur = to;
	}
	return launches;
}

int srt_launch_build_sort(const BuildParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	uint32_t cur = 0u;
	return sort_passes(p, num_models, max_records ? SRT_BUILD_TILES(max_records) : 1u, stream, (uint32_t)SRT_BUILD_SORT_PASSES, cur, true, p.order, SortTake{0u, 0xffffffffu});
}

// ---- the median-split order -------------------------------------------------------------------------------------------------
static_assert(SRT_BUILD_LOCAL == 4u * 256u, "the local launch: 256 threads, four records each");
static_assert(SRT_BUILD_LOCAL >= SRT_BUILD_TILE, "a tile of a global level touches at most two ranges: every range there has at least SRT_BUILD_LOCAL records");

struct MedianRange {
	uint32_t b, e, idx;
};
// the range of depth `depth` that holds record s of n: `depth` halvings at b + n / 2 (bvh_host.cpp balanced_into). Halving on
// below a leaf's size is harmless: nothing of at most SRT_BVH_LEAF_MAX records is ever sorted.
static __device__ __forceinline__ MedianRange median_range(uint32_t n, uint32_t s, uint32_t depth) {
	MedianRange r = {0u, n, 0u};
	for (uint32_t d = 0; d < depth; d++) {
		const uint32_t mid = r.b + (r.e - r.b) / 2u;
		const bool right = s >= mid;
		r.b = right ? mid : r.b, r.e = right ? r.e : mid, r.idx = 2u * r.idx + (right ? 1u : 0u);
	}
	return r;
}
// ... and range `idx` of that depth
static __device__ __forceinline__ MedianRange median_range_at(uint32_t n, uint32_t idx, uint32_t depth) {
	MedianRange r = {0u, n, idx};
	for (uint32_t d = depth; d-- > 0u;) {
		const uint32_t mid = r.b + (r.e - r.b) / 2u;
		const bool right = (idx >> d) & 1u;
		r.b = right ? mid : r.b, r.e = right ? r.e : mid;
	}
	return r;
}
// global level `level` is for the models whose largest range there, ceil(n / 2^level), exceeds SRT_BUILD_LOCAL
static SortTake median_take(uint32_t level) { return SortTake{SRT_BUILD_LOCAL << level, SRT_BUILD_LOCAL << SRT_BUILD_MEDIAN_MAX_LEVELS}; }
// BvhBuilder::load's centroid; false: a non-finite triangle
struct Centroid {
	float x, y, z;
};
static __device__ __forceinline__ bool centroid_of(const srt_model *m, const srt_triangle *tr, Centroid &c) {
	Box b;
	if (!triangle_box(m, tr, b)) return false;
	c.x = 0.5f * b.lo[0] + 0.5f * b.hi[0], c.y = 0.5f * b.lo[1] + 0.5f * b.hi[1], c.z = 0.5f * b.lo[2] + 0.5f * b.hi[2];
	return true;
}
// BvhBuilder::median_key (bvh_host.cpp), operation for operation
static __device__ __forceinline__ uint32_t median_key(float c, float clo, float ext) {
	if (!(ext > 0.0f) || !finite_f(ext)) return 0u;
	const float f = (c - clo) * (65536.0f / ext);
	return f >= 65535.0f ? 65535u : (f > 0.0f ? (uint32_t)(int)f : 0u);
}
// the key of centroid c in a range with the centroid extents e[0 .. 6) (ordered integers): the host's axis rule, then the cell
static __device__ __forceinline__ uint32_t median_key_in(const Centroid c, const uint32_t *e) {
	const float lx = unordered(e[0]), ly = unordered(e[1]), lz = unordered(e[2]);
	const float ex = unordered(e[3]) - lx, ey = unordered(e[4]) - ly, ez = unordered(e[5]) - lz;
	float bc = c.x, bl = lx, be = ex;
	if (ey > be) bc = c.y, bl = ly, be = ey;
	if (ez > be) bc = c.z, bl = lz, be = ez;
	return median_key(bc, bl, be);
}
#define SRT_MEDIAN_NONFINITE 0x10000u

// vals == NULL: the identity (level 0). One workgroup per tile; its records lie in at most two ranges of the level.
__global__ __launch_bounds__(256) void srt_build_median_extents_kernel(const BuildParams p, const uint32_t *__restrict__ vals, uint32_t level, const SortTake take) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t n = rm.num_records, tile = blockIdx.x;
	if (tile >= SRT_BUILD_TILES(n) || !take(n)) return; // (the whole workgroup)
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	__shared__ uint32_t sh[12]; // two ranges: lo.xyz (minima), hi.xyz (maxima)
	if (threadIdx.x < 12u) sh[threadIdx.x] = (threadIdx.x % 6u) < 3u ? 0xffffffffu : 0u;
	__syncthreads();
	const uint32_t first = median_range(n, tile * SRT_BUILD_TILE, level).idx;
	uint32_t lo0[3], hi0[3], lo1[3], hi1[3];
#pragma unroll
	for (int a = 0; a < 3; a++) lo0[a] = lo1[a] = 0xffffffffu, hi0[a] = hi1[a] = 0u;
	for (uint32_t r = 0; r < SRT_BUILD_TILE / 256u; r++) {
		const uint32_t s = tile * SRT_BUILD_TILE + r * 256u + threadIdx.x;
		if (s >= n) continue;
		const uint32_t v = vals ? vals[rm.first_record + s] : s, j = v < n ? v : n - 1u; // (always v < n behind a sort of this model)
		Centroid c;
		if (!centroid_of(m, p.triangles + (m->triangle_index + j), c)) continue;
		const bool second = median_range(n, s, level).idx != first;
		const uint32_t oc[3] = {ordered(c.x), ordered(c.y), ordered(c.z)};
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const uint32_t o = oc[a];
			if (second) lo1[a] = min(lo1[a], o), hi1[a] = max(hi1[a], o);
			else lo0[a] = min(lo0[a], o), hi0[a] = max(hi0[a], o);
		}
	}
#pragma unroll
	for (int a = 0; a < 3; a++)
		for (uint32_t off = 32u; off > 0u; off >>= 1) {
			lo0[a] = min(lo0[a], (uint32_t)__shfl_xor((int)lo0[a], (int)off)), hi0[a] = max(hi0[a], (uint32_t)__shfl_xor((int)hi0[a], (int)off));
			lo1[a] = min(lo1[a], (uint32_t)__shfl_xor((int)lo1[a], (int)off)), hi1[a] = max(hi1[a], (uint32_t)__shfl_xor((int)hi1[a], (int)off));
		}
	if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
		for (int a = 0; a < 3; a++) {
			atomicMin(&sh[a], lo0[a]), atomicMax(&sh[3 + a], hi0[a]);
			atomicMin(&sh[6 + a], lo1[a]), atomicMax(&sh[9 + a], hi1[a]);
		}
	}
	__syncthreads();
	if (threadIdx.x < 12u) {
		const uint32_t range = first + threadIdx.x / 6u, k = threadIdx.x % 6u, v = sh[threadIdx.x];
		if (range < (1u << level)) { // (the second range of the level's last tile: there is none)
			uint32_t *slot = p.ranges + 6u * ((size_t)p.range_first[blockIdx.y] + ((1u << level) - 1u) + range);
			if (k < 3u) {
				if (v != 0xffffffffu) atomicMin(&slot[k], v);
			} else if (v != 0u) {
				atomicMax(&slot[k], v);
			}
		}
	}
}

__global__ __launch_bounds__(256) void srt_build_median_keys_kernel(const BuildParams p, const uint32_t *__restrict__ vals, uint32_t *__restrict__ keys, uint32_t level, const SortTake take) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t n = rm.num_records, tile = blockIdx.x;
	if (tile >= SRT_BUILD_TILES(n) || !take(n)) return; // (the whole workgroup)
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	const uint32_t *slots = p.ranges + 6u * ((size_t)p.range_first[blockIdx.y] + ((1u << level) - 1u));
	for (uint32_t r = 0; r < SRT_BUILD_TILE / 256u; r++) {
		const uint32_t s = tile * SRT_BUILD_TILE + r * 256u + threadIdx.x;
		if (s >= n) continue;
		const uint32_t v = vals ? vals[rm.first_record + s] : s, j = v < n ? v : n - 1u;
		const uint32_t range = median_range(n, s, level).idx; // < 2^level
		Centroid c;
		uint32_t key = SRT_MEDIAN_NONFINITE;
		if (centroid_of(m, p.triangles + (m->triangle_index + j), c)) key = median_key_in(c, slots + 6u * (size_t)range);
		keys[rm.first_record + s] = (range << SRT_BUILD_MEDIAN_KEY_BITS) | key;
	}
}

// One workgroup per range of the model's first depth whose ranges all fit SRT_BUILD_LOCAL (blockIdx.x = the range): all remaining
// depths in LDS, then the scene's order array. Every thread takes every barrier; the depth loop's trip count is the range's.
__global__ __launch_bounds__(256) void srt_build_median_local_kernel(const BuildParams p) {
	const RefitModel rm = p.models[blockIdx.y];
	const uint32_t n = rm.num_records, levels = srt_build_median_levels(n);
	if (n == 0u || levels > SRT_BUILD_MEDIAN_MAX_LEVELS || blockIdx.x >= (1u << levels)) return; // (the whole workgroup)
	const srt_model *m = &p.shapes[rm.shape].shape.model;
	// every pass of the sort changes sides: where the model's last global level left its indices
	uint32_t passes = 0u;
	for (uint32_t l = 0; l < levels; l++) passes += srt_build_median_passes(l);
	const uint32_t *src = levels ? ((passes & 1u) ? p.vals[1] : p.vals[0]) + rm.first_record : nullptr; // (NULL: no global level, the identity)
	const MedianRange rg = median_range_at(n, blockIdx.x, levels);
	const uint32_t cnt = rg.e - rg.b < SRT_BUILD_LOCAL ? rg.e - rg.b : SRT_BUILD_LOCAL; // (1 .. SRT_BUILD_LOCAL as it is)
	__shared__ float cent[3][SRT_BUILD_LOCAL]; // by slot = the record's place in the range at the start; cent[0]: NaN = not finite
	__shared__ uint32_t perm[2][SRT_BUILD_LOCAL]; // place -> slot
	__shared__ uint32_t ckey[SRT_BUILD_LOCAL];    // by place: key << 10 | place
	__shared__ uint32_t ext[6u * 256u];           // per sub-range of the depth (at most 256 of more than a leaf's records)
	for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
		const uint32_t v = src ? src[rg.b + i] : rg.b + i, j = v < n ? v : n - 1u;
		Centroid c;
		if (!centroid_of(m, p.triangles + (m->triangle_index + j), c)) c.x = u2f(0x7fc00000u), c.y = c.z = 0.0f;
		cent[0][i] = c.x, cent[1][i] = c.y, cent[2][i] = c.z;
		perm[0][i] = i;
	}
	__syncthreads();
	uint32_t cur = 0u;
	for (uint32_t d = 0; d <= 8u && ((cnt + (1u << d) - 1u) >> d) > (uint32_t)SRT_BVH_LEAF_MAX; d++) { // (cnt <= 1024: d <= 8, 2^d <= 256 sub-ranges)
		for (uint32_t k = threadIdx.x; k < (6u << d); k += 256u) ext[k] = (k % 6u) < 3u ? SRT_REFIT_EXT_LO_INIT : SRT_REFIT_EXT_HI_INIT; // (the empty box: FLT_MAX, -FLT_MAX)
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
			const MedianRange sr = median_range(cnt, i, d);
			const uint32_t slot = perm[cur][i];
			const float c0 = cent[0][slot];
			if (sr.e - sr.b <= (uint32_t)SRT_BVH_LEAF_MAX || !(c0 == c0)) continue;
			const uint32_t ox = ordered(c0), oy = ordered(cent[1][slot]), oz = ordered(cent[2][slot]);
			uint32_t *e = &ext[6u * sr.idx];
			atomicMin(&e[0], ox), atomicMin(&e[1], oy), atomicMin(&e[2], oz);
			atomicMax(&e[3], ox), atomicMax(&e[4], oy), atomicMax(&e[5], oz);
		}
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
			const MedianRange sr = median_range(cnt, i, d);
			const uint32_t slot = perm[cur][i];
			const Centroid c = {cent[0][slot], cent[1][slot], cent[2][slot]};
			uint32_t key = 0u; // (a leaf's records stay where they are)
			if (sr.e - sr.b > (uint32_t)SRT_BVH_LEAF_MAX) key = c.x == c.x ? median_key_in(c, &ext[6u * sr.idx]) : SRT_MEDIAN_NONFINITE;
			ckey[i] = (key << 10) | i;
		}
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
			const MedianRange sr = median_range(cnt, i, d);
			uint32_t to = i;
			if (sr.e - sr.b > (uint32_t)SRT_BVH_LEAF_MAX) { // the record's rank in its sub-range: the composites are unique, so this is the stable order
				const uint32_t mine = ckey[i];
				uint32_t rank = 0u;
				for (uint32_t q = sr.b; q < sr.e; q++) rank += ckey[q] < mine ? 1u : 0u;
				to = sr.b + rank; // < sr.e: a record is not smaller than itself
			}
			perm[cur ^ 1u][to] = perm[cur][i];
		}
		__syncthreads();
		cur ^= 1u;
	}
	for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
		const uint32_t slot = perm[cur][i] < cnt ? perm[cur][i] : i;
		const uint32_t v = src ? src[rg.b + slot] : rg.b + slot;
		p.order[rm.first_record + rg.b + i] = v < n ? v : n - 1u; // (rg.b + i < n: inside the model's records)
	}
}

int srt_launch_build_median(const BuildParams &p, uint32_t num_models, uint32_t max_records, void *stream) {
	const uint32_t gx = max_records ? SRT_BUILD_TILES(max_records) : 1u, levels = srt_build_median_levels(max_records);
	if (levels > SRT_BUILD_MEDIAN_MAX_LEVELS) return 0; // (the caller's to keep out)
	int launches = 0;
	uint32_t cur = 0u;
	for (uint32_t level = 0; level < levels; level++) {
		const SortTake take = median_take(level);
		const uint32_t *vals = level ? p.vals[cur] : nullptr;
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_median_extents_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, vals, level, take); });
		launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_median_keys_kernel, dim3(gx, cnt), dim3(256), 0, (hipStream_t)stream, q, vals, q.keys[cur], level, take); });
		launches += sort_passes(p, num_models, gx, stream, srt_build_median_passes(level), cur, level == 0u, nullptr, take);
	}
	launches += per_slab(p, num_models, [&](const BuildParams &q, uint32_t cnt) { hipLaunchKernelGGL(srt_build_median_local_kernel, dim3(1u << levels, cnt), dim3(256), 0, (hipStream_t)stream, q); });
	return launches;
}
