// area.hip -- area selection behind the ABI (include/srt_abi.h "area selection"): marquee and lasso coverage counted from the ID
// pass's planes, and the selection modes on top. A translation unit of its own: the kernels here are new, every kernel the
// library launched before keeps its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_area_count_kernel<LASSO, BY_TRIANGLE>: a masked histogram with as many bins as the scene has shapes (or the model has
//    triangles). The grid covers the clipped rectangle only: a wave takes 64 consecutive pixels of ONE row (its plane loads are
//    one 256-byte read, tail lanes inactive), a workgroup of 256 lanes four rows. The lasso sits in LDS as doubled vertices; the
//    wave's row is a scalar, so "the edge spans the row" (area_host.h) is a scalar branch per edge and only the cross product of
//    a spanning edge is per-lane work; a wave whose row lies outside the polygon's y-range walks no edge. Counting: the lanes
//    that share the first active lane's key are balloted and their leader adds the popcount with one atomic; after `rounds`
//    such rounds (SRT_AREA_AGG_ROUNDS) the lanes left add 1 each. ID planes are piecewise constant, so the common wave has 1 to
//    3 keys; a dense mesh under BY_TRIANGLE is the many-keys case the per-lane tail is for. EVERY key is compared with the
//    count array's length before its atomic. The summary's three sums are ballot popcounts in scalar registers, one atomic
//    each per workgroup.
//  * srt_area_finish_kernel: distinct = the counts that are not zero, hit_pixels = area_pixels - miss_pixels.
// Counts and summary are cleared by hipMemsetAsync on the handle's stream ahead of the launches.
// area_through.hip (X-ray coverage: other counting kernels, the same result) shares the clear, the finish launch, the blocking
// read-back and the selection rule through srt_internal.h (srt_area_clear ... srt_area_select_counts below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "area_host.h"
#include "srt_internal.h"

struct AreaParams {
	const uint32_t *shape, *triangle; /* the ID planes, w words per row */
	uint32_t *counts;                 /* n_counts words, zeroed */
	uint32_t *summary;                /* 8 words as srt_area_summary, zeroed */
	uint32_t n_counts, target;        /* BY_TRIANGLE: the shape whose triangles are counted */
	int32_t w;                        /* the planes' width */
	int32_t x0, y0, x1, y1;           /* the clipped rectangle, not empty */
	uint32_t col_groups;              /* ceil((x1 - x0) / 64): workgroup b takes column group b % col_groups of row group b / col_groups */
	uint32_t rounds;                  /* aggregated rounds before the per-lane atomics */
	uint32_t n_vertices;
	int32_t ylo2, yhi2;               /* the lasso's lowest and highest doubled y */
};
struct AreaLassoParams {
	AreaParams a;
	int32_t v2[2 * SRT_AREA_MAX_VERTICES]; /* the doubled vertices (kernel arguments: no upload, no lifetime) */
};
template <bool LASSO>
struct AreaArgs {
	typedef AreaParams type;
};
template <>
struct AreaArgs<true> {
	typedef AreaLassoParams type;
};
static inline __host__ __device__ const AreaParams &area_base(const AreaParams &p) { return p; }
static inline __host__ __device__ const AreaParams &area_base(const AreaLassoParams &p) { return p.a; }

template <bool LASSO, bool BY_TRIANGLE>
__global__ __launch_bounds__(256) void srt_area_count_kernel(const typename AreaArgs<LASSO>::type args) {
	const AreaParams &ap = area_base(args);
	__shared__ int32_t lasso[LASSO ? 2 * SRT_AREA_MAX_VERTICES : 2];
	__shared__ uint32_t sums[4][3];
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (a scalar the compiler can see)
	if constexpr (LASSO) {
		for (uint32_t i = threadIdx.x; i < 2u * ap.n_vertices; i += 256u) lasso[i] = args.v2[i]; // n_vertices <= SRT_AREA_MAX_VERTICES (area_check)
		__syncthreads();
	}
	const uint32_t col_group = blockIdx.x % ap.col_groups, row_group = blockIdx.x / ap.col_groups;
	const int32_t y = ap.y0 + (int32_t)(row_group * 4u + wave);           // the wave's row
	const int32_t x = ap.x0 + (int32_t)(col_group * 64u + lane);
	bool m = y < ap.y1 && x < ap.x1; // lanes past the rectangle load nothing
	uint32_t s = SRT_HIT_NONE, key = SRT_HIT_NONE;
	if (m) {
		const size_t q = (size_t)y * (size_t)ap.w + (size_t)x;
		s = ap.shape[q];
		key = BY_TRIANGLE ? ap.triangle[q] : s;
	}
	if constexpr (LASSO) {
		const int32_t cy = 2 * y + 1;
		bool in = false;
		if (cy > ap.ylo2 && cy < ap.yhi2) { // (scalar) else no edge spans the row
			const int64_t cx = 2 * (int64_t)x + 1;
			const uint32_t n = ap.n_vertices;
			int32_t ax = __builtin_amdgcn_readfirstlane(lasso[0]), ay = __builtin_amdgcn_readfirstlane(lasso[1]);
			for (uint32_t i = 0; i < n; i++) {
				const uint32_t j = i + 1u == n ? 0u : i + 1u;
				const int32_t bx = __builtin_amdgcn_readfirstlane(lasso[2u * j]), by = __builtin_amdgcn_readfirstlane(lasso[2u * j + 1u]);
				if (area_edge_spans(ay, by, cy)) // (scalar)
					in ^= area_edge_counts(ax, ay, bx, by, cx, cy);
				ax = bx, ay = by;
			}
		}
		m = m && in;
	}
	// ---- the summary: popcounts of votes, scalars ----
	const bool miss = m && s == SRT_HIT_NONE;
	bool active = (BY_TRIANGLE ? m && s == ap.target : m && !miss) && key < ap.n_counts; // a key beyond the array is dropped HERE
	const uint32_t n_area = (uint32_t)__popcll(__ballot(m)), n_miss = (uint32_t)__popcll(__ballot(miss));
	const uint32_t n_target = BY_TRIANGLE ? (uint32_t)__popcll(__ballot(active)) : 0u;
	// ---- the counts: the lanes that share the first active lane's key add once ----
	for (uint32_t r = 0; r < ap.rounds; r++) {
		const unsigned long long left = __ballot(active);
		if (left == 0ull) break;
		const int leader = __ffsll((long long)left) - 1;
		const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, leader); // < n_counts: the leader is active
		const bool same = active && key == k0;
		const uint32_t n_same = (uint32_t)__popcll(__ballot(same));
		if ((int)lane == leader) atomicAdd(ap.counts + k0, n_same);
		active = active && !same;
	}
	if (active) atomicAdd(ap.counts + key, 1u); // key < n_counts (checked above)
	if (lane == 0u) sums[wave][0] = n_area, sums[wave][1] = n_miss, sums[wave][2] = n_target;
	__syncthreads();
	if (threadIdx.x == 0u) {
		const uint32_t a = sums[0][0] + sums[1][0] + sums[2][0] + sums[3][0], b = sums[0][1] + sums[1][1] + sums[2][1] + sums[3][1];
		if (a) atomicAdd(ap.summary + 0, a);
		if (b) atomicAdd(ap.summary + 2, b);
		if (BY_TRIANGLE) {
			const uint32_t c = sums[0][2] + sums[1][2] + sums[2][2] + sums[3][2];
			if (c) atomicAdd(ap.summary + 4, c);
		}
	}
}

// behind the counting kernel on the same stream: summary[3] = the counts that are not zero, summary[1] = area - miss
__global__ __launch_bounds__(256) void srt_area_finish_kernel(const uint32_t *counts, uint32_t n, uint32_t *summary) {
	uint32_t mine = 0u;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) mine += counts[i] != 0u ? 1u : 0u;
	uint32_t wave_sum = mine; // (mine <= a few: a butterfly over the wave's 64 lanes)
	for (int d = 32; d > 0; d >>= 1) wave_sum += (uint32_t)__shfl_xor((int)wave_sum, d, 64);
	if ((threadIdx.x & 63u) == 0u && wave_sum) atomicAdd(summary + 3, wave_sum);
	if (blockIdx.x == 0u && threadIdx.x == 0u) summary[1] = summary[0] - summary[2];
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

uint32_t agg_rounds() {
#ifdef SRT_DEV_KNOBS
	if (const char *e = getenv("SRT_AREA_ROUNDS")) return (uint32_t)atoi(e); // (development builds: scripts/area_probe.py measures 0, 2, 4, 8)
#endif
	return SRT_AREA_AGG_ROUNDS;
}

template <bool LASSO, bool BY_TRIANGLE>
void launch_count(const AreaParams &ap, const int32_t *v2, uint32_t blocks, hipStream_t stream) {
	typename AreaArgs<LASSO>::type args;
	if constexpr (LASSO) {
		memset(&args, 0, sizeof args);
		args.a = ap;
		memcpy(args.v2, v2, 2 * sizeof(int32_t) * ap.n_vertices);
	} else {
		args = ap;
	}
	hipLaunchKernelGGL((srt_area_count_kernel<LASSO, BY_TRIANGLE>), dim3(blocks), dim3(256), 0, stream, args);
}

// What every coverage call does first: the block checked, the planes current (options) or held and not stale (NULL)
int area_begin(srt_tracer *t, const char *who, const srt_render_data *options, const srt_area *area, const int32_t *vertices) {
	if (area_check(area, vertices) != SRT_OK)
		return fail(t, SRT_ERR_INVALID, std::string(who) + ": the area is refused (srt_area_check_host)");
	SRT_HIP(t, hipSetDevice(t->device));
	SelectionState *s = t->sel;
	t->ar.last_id_ran = false;
	if (options) return srt_selection_ids_current(t, options, &t->ar.last_id_ran);
	if (s->ids_w == 0 || !s->ids.ptr || !s->ids_valid) return fail(t, SRT_ERR_STATE, std::string(who) + ": no ID pass on this handle yet");
	if (s->ids_key.scene != t || s->ids_key.scene_rev != t->scene_rev)
		return fail(t, SRT_ERR_STATE, std::string(who) + ": the scene has changed since the ID planes were made");
	return SRT_OK;
}

// the clear and the launches over the handle's planes into counts (n words, of which n_counts are counted) and summary (8
// words), both on the device, on the handle's stream
int enqueue_count(srt_tracer *t, const srt_area &area, const int32_t *vertices, bool by_triangle, uint32_t target, uint32_t *counts, size_t n, uint32_t n_counts,
                  uint32_t *summary, bool one_block) {
	const SelectionState *s = t->sel;
	if (const int rc = srt_area_clear(t, counts, n, summary, one_block)) return rc;
	int32_t c[4];
	area_clip(area, s->ids_w, s->ids_h, c);
	const bool launched = c[0] < c[2] && c[1] < c[3];
	if (launched) { // else: all zeros, nothing to launch
		AreaParams ap;
		memset(&ap, 0, sizeof ap);
		const size_t px = (size_t)s->ids_w * (size_t)s->ids_h;
		ap.shape = s->ids.ptr, ap.triangle = s->ids.ptr + px;
		ap.counts = counts, ap.summary = summary;
		ap.n_counts = n_counts, ap.target = target;
		ap.w = s->ids_w;
		ap.x0 = c[0], ap.y0 = c[1], ap.x1 = c[2], ap.y1 = c[3];
		ap.col_groups = (uint32_t)((c[2] - c[0] + 63) / 64);
		ap.rounds = agg_rounds();
		ap.n_vertices = area.n_vertices;
		const uint32_t blocks = ap.col_groups * (uint32_t)((c[3] - c[1] + 3) / 4); // < 2^31: the frame is below 2^31 pixels
		if (area.n_vertices) {
			int32_t v2[2 * SRT_AREA_MAX_VERTICES], yr[2];
			area_double(vertices, area.n_vertices, v2, yr);
			ap.ylo2 = yr[0], ap.yhi2 = yr[1];
			if (by_triangle) launch_count<true, true>(ap, v2, blocks, t->stream);
			else launch_count<true, false>(ap, v2, blocks, t->stream);
		} else {
			if (by_triangle) launch_count<false, true>(ap, nullptr, blocks, t->stream);
			else launch_count<false, false>(ap, nullptr, blocks, t->stream);
		}
		SRT_HIP(t, hipGetLastError());
	}
	return srt_area_finish(t, counts, n_counts, summary, launched);
}

// the blocking forms: into the handle's own buffer, back as ONE copy through pinned memory behind its event
int coverage_host(srt_tracer *t, const srt_area &area, const int32_t *vertices, bool by_triangle, uint32_t target, uint32_t n_counts, uint32_t *counts,
                  srt_area_summary *out) {
	return srt_area_result_host(t, n_counts, counts, out, [&](uint32_t *d_counts, uint32_t *d_summary) {
		return enqueue_count(t, area, vertices, by_triangle, target, d_counts, n_counts, n_counts, d_summary, true);
	});
}

uint32_t scene_shapes(const srt_tracer *t) { return t->scene_set ? (uint32_t)t->sd.num_shapes : 0u; }

std::vector<uint32_t> sorted_unique(std::vector<uint32_t> v) {
	std::sort(v.begin(), v.end());
	v.erase(std::unique(v.begin(), v.end()), v.end());
	return v;
}

} // namespace

// ---- what area_through.hip shares (srt_internal.h): the same result buffers, span, finish kernel and selection rule ----
int srt_area_clear(srt_tracer *t, uint32_t *counts, size_t n, uint32_t *summary, bool one_block) {
	t->ar.span.timed = false;
	if (t->timers_in_render) SRT_HIP(t, t->ar.span.begin(t->stream));
	if (one_block) { // summary, then the counts, in one allocation
		SRT_HIP(t, hipMemsetAsync(summary, 0, (8 + n) * sizeof(uint32_t), t->stream));
	} else {
		SRT_HIP(t, hipMemsetAsync(summary, 0, 8 * sizeof(uint32_t), t->stream));
		if (n) SRT_HIP(t, hipMemsetAsync(counts, 0, n * sizeof(uint32_t), t->stream));
	}
	return SRT_OK;
}

int srt_area_finish(srt_tracer *t, const uint32_t *counts, uint32_t n_counts, uint32_t *summary, bool launched) {
	if (launched) {
		const uint32_t finish_blocks = n_counts == 0u ? 1u : std::min<uint32_t>((n_counts + 255u) / 256u, 1024u);
		hipLaunchKernelGGL(srt_area_finish_kernel, dim3(finish_blocks), dim3(256), 0, t->stream, counts, n_counts, summary);
		SRT_HIP(t, hipGetLastError());
	}
	if (t->timers_in_render) SRT_HIP(t, t->ar.span.end(t->stream));
	return SRT_OK;
}

int srt_area_model_triangles(srt_tracer *t, const char *who, uint32_t shape, uint32_t *n_triangles) {
	if (shape >= scene_shapes(t)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": shape is not a shape of the scene");
	SRT_HIP(t, hipSetDevice(t->device));
	uint32_t head[6]; // the shape's record as uploaded: type, material, pad x 2, model.triangle_index, model.num_triangles
	SRT_HIP(t, hipMemcpyAsync(head, t->shapes.ptr + shape, sizeof head, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if ((int32_t)head[0] != SRT_SHAPE_MODEL) return fail(t, SRT_ERR_INVALID, std::string(who) + ": shape is not a model");
	*n_triangles = head[5];
	return SRT_OK;
}

int srt_area_select_counts(srt_tracer *t, const uint32_t *counts, size_t n, int mode, uint32_t min_pixels, size_t *n_selected) {
	std::vector<uint32_t> hit, next;
	const uint32_t need = min_pixels > 1u ? min_pixels : 1u;
	for (size_t i = 0; i < n; i++)
		if (counts[i] >= need) hit.push_back((uint32_t)i); // ascending
	SelectionState *s = t->sel;
	const std::vector<uint32_t> cur = s->on ? sorted_unique(s->shapes) : std::vector<uint32_t>();
	if (mode == SRT_SELECT_REPLACE) next = hit;
	else if (mode == SRT_SELECT_ADD) std::set_union(cur.begin(), cur.end(), hit.begin(), hit.end(), std::back_inserter(next));
	else if (mode == SRT_SELECT_SUBTRACT) std::set_difference(cur.begin(), cur.end(), hit.begin(), hit.end(), std::back_inserter(next));
	else std::set_symmetric_difference(cur.begin(), cur.end(), hit.begin(), hit.end(), std::back_inserter(next));
	if (n_selected) *n_selected = next.size();
	srt_selection_params p = s->p;
	if (p.enabled == 0 && p.outline_width == 0.0f) srt_selection_defaults(&p); // srt_set_selection never stored a block
	p.enabled = 1;
	return srt_set_selection(t, &p, next.empty() ? nullptr : next.data(), next.size()); // (n == 0: off, as the call documents)
}

extern "C" {

int srt_area_sizes(size_t out[2]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_area);
	out[1] = sizeof(srt_area_summary);
	return SRT_OK;
}

int srt_area_check_host(const srt_area *area, const int32_t *vertices) { return area_check(area, vertices); }

int srt_area_mask_host(const srt_area *area, const int32_t *vertices, int w, int h, uint8_t *mask, size_t cap) {
	return area_mask(area, vertices, (int32_t)w, (int32_t)h, mask, cap);
}

int srt_area_coverage(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                      srt_area_summary *out) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !out) return fail(t, SRT_ERR_INVALID, "srt_area_coverage: NULL argument");
	const uint32_t n = scene_shapes(t);
	if (cap_shapes < n || (n && !counts)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage: counts is smaller than the scene's shape count");
	try {
		if (const int rc = area_begin(t, "srt_area_coverage", options, area, vertices)) return rc;
		return coverage_host(t, *area, vertices, false, 0u, n, counts, out);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_area_triangle_coverage(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape, uint32_t *counts,
                               size_t cap_triangles, srt_area_summary *out) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !out) return fail(t, SRT_ERR_INVALID, "srt_area_triangle_coverage: NULL argument");
	if (area_check(area, vertices) != SRT_OK) return fail(t, SRT_ERR_INVALID, "srt_area_triangle_coverage: the area is refused (srt_area_check_host)");
	try {
		uint32_t n = 0;
		if (const int rc = srt_area_model_triangles(t, "srt_area_triangle_coverage", shape, &n)) return rc;
		if (cap_triangles < n || (n && !counts)) return fail(t, SRT_ERR_INVALID, "srt_area_triangle_coverage: counts is smaller than the model's triangle count");
		if (const int rc = area_begin(t, "srt_area_triangle_coverage", options, area, vertices)) return rc;
		return coverage_host(t, *area, vertices, true, shape, n, counts, out);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_area_coverage_device(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *d_counts, size_t n,
                             uint32_t *d_summary) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !d_summary) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_device: NULL argument");
	const uint32_t n_shapes = scene_shapes(t);
	if (n < n_shapes || (n && !d_counts)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_device: d_counts is smaller than the scene's shape count");
	if (n >= ((size_t)1 << 31)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_device: n must stay below 2^31");
	if (((uintptr_t)d_counts | (uintptr_t)d_summary) & 3u) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_device: arrays must be aligned to 4 bytes");
	if (const int rc = area_begin(t, "srt_area_coverage_device", options, area, vertices)) return rc;
	return enqueue_count(t, *area, vertices, false, 0u, d_counts, n, n_shapes, d_summary, false);
}

int srt_read_selection(srt_tracer *t, uint32_t *shapes, size_t cap, size_t *n) {
	if (!t) return SRT_ERR_INVALID;
	if (!n) return fail(t, SRT_ERR_INVALID, "srt_read_selection: n is NULL");
	try {
		const SelectionState *s = t->sel;
		const std::vector<uint32_t> list = s->on ? sorted_unique(s->shapes) : std::vector<uint32_t>();
		*n = list.size();
		if (!shapes) return SRT_OK;
		if (cap < list.size()) return fail(t, SRT_ERR_INVALID, "srt_read_selection: shapes is smaller than the list");
		if (!list.empty()) memcpy(shapes, list.data(), list.size() * sizeof(uint32_t));
		return SRT_OK;
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_select_area(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                    size_t *n_selected) {
	if (!t) return SRT_ERR_INVALID;
	if (mode < SRT_SELECT_REPLACE || mode > SRT_SELECT_TOGGLE) return fail(t, SRT_ERR_INVALID, "srt_select_area: mode is SRT_SELECT_REPLACE, ADD, SUBTRACT or TOGGLE");
	if (!area) return fail(t, SRT_ERR_INVALID, "srt_select_area: NULL argument");
	try {
		std::vector<uint32_t> counts(scene_shapes(t));
		srt_area_summary sum;
		if (const int rc = srt_area_coverage(t, options, area, vertices, counts.data(), counts.size(), &sum)) return rc;
		return srt_area_select_counts(t, counts.data(), counts.size(), mode, min_pixels, n_selected);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_last_area_ms(srt_tracer *t, float *ms) {
	if (!t) return SRT_ERR_INVALID;
	if (!ms) return fail(t, SRT_ERR_INVALID, "srt_last_area_ms: NULL");
	*ms = 0.f;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	SRT_HIP(t, t->ar.span.elapsed(ms));
	return SRT_OK;
}

int srt_last_area_id_pass(const srt_tracer *t, int *id_pass_ran) {
	if (!t || !id_pass_ran) return SRT_ERR_INVALID;
	*id_pass_ran = t->ar.last_id_ran ? 1 : 0;
	return SRT_OK;
}

} // extern "C"
