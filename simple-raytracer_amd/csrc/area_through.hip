// area_through.hip -- X-ray area selection behind the ABI (include/srt_abi.h "area selection, through"): which shapes, or which
// faces of one mesh, lie inside a marquee or lasso with the ones BEHIND other shapes included. No ID planes: every pixel of the
// area casts the ID pass's ray and the count is over the ray's whole candidate set ("multi-hit ray queries"). A translation unit
// of its own: the kernels here are new, every kernel the library launched before keeps its instruction stream
// (scripts/kernel_isa_digest.py).
//
//  * srt_area_through_kernel<LASSO, HAS_MODELS, USE_BVH>: area.hip's mapping -- the grid covers the clipped rectangle only, a wave
//    takes 64 consecutive pixels of ONE row, a workgroup of 256 lanes four rows, the lasso sits in LDS as doubled vertices and is
//    decided by area_host.h's two functions. A lane inside M makes its ray (device_math.h camera_ray of the pixel centre, refused
//    by ray_valid.inc) and runs the multi-hit kernel's loop over runs and blocks, which is wave-uniform; only "my ray meets this
//    primitive" is per lane. For the sphere or plane of index s the wave's count is the popcount of one ballot, added by one lane
//    with one atomic. For a model the lanes whose ray passes its box against +inf run the ANY-HIT scan or walk
//    (device_anyhit.h: existence is all that is asked), and after they reconverge the same ballot and atomic follow. No key is
//    matched and no lane adds for itself. `s < n_counts` stands in front of every atomic.
//  * srt_area_through_triangles_kernel<LASSO, USE_BVH>: the same mapping and loop, but only the target model's box is tested and
//    only its triangles are visited: the multi-hit scan and walk without a list and with the limit fixed at tmax -- no early
//    exit, every accepted triangle is one atomic on its index inside the model (under a hierarchy from bvh_tri_in_model),
//    compared with n_counts first.
//  * The summary's sums are ballot popcounts through LDS, one atomic each per workgroup, and area.hip's srt_area_finish_kernel
//    (srt_area_finish) makes distinct and hit_pixels.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_anyhit.h"
#include "device_multihit.h"
#include "area_host.h"
#include "area_through_host.h"
#include "query_host.h"

struct ThroughParams {
	TraceParams tp;            /* the scene buffers and the camera, as a dispatch's (rd: the frame; f_width .. inv_f_height) */
	uint32_t *counts;          /* n_counts words, zeroed */
	uint32_t *summary;         /* 8 words as srt_area_summary, zeroed */
	uint32_t n_counts, target; /* triangle mode: the model shape whose triangles are counted */
	int32_t x0, y0, x1, y1;    /* the clipped rectangle, not empty */
	uint32_t col_groups;       /* ceil((x1 - x0) / 64): workgroup b takes column group b % col_groups of row group b / col_groups */
	uint32_t n_vertices;
	int32_t ylo2, yhi2;        /* the lasso's lowest and highest doubled y */
};
struct ThroughLassoParams {
	ThroughParams a;
	int32_t v2[2 * SRT_AREA_MAX_VERTICES]; /* the doubled vertices (kernel arguments: no upload, no lifetime) */
};
static_assert(sizeof(ThroughLassoParams) <= 4096, "a kernel's arguments are at most 4 KiB");
template <bool LASSO>
struct ThroughArgs {
	typedef ThroughParams type;
};
template <>
struct ThroughArgs<true> {
	typedef ThroughLassoParams type;
};
static inline __host__ __device__ const ThroughParams &through_base(const ThroughParams &p) { return p; }
static inline __host__ __device__ const ThroughParams &through_base(const ThroughLassoParams &p) { return p.a; }

namespace {

// M(p) of the lane's pixel: area.hip's statements. The lasso has been copied to LDS (and the workgroup has met) by the caller.
template <bool LASSO>
__device__ __forceinline__ bool through_mask(const ThroughParams &ap, const int32_t *lasso, int32_t x, int32_t y) {
	bool m = y < ap.y1 && x < ap.x1;
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
	return m;
}

// the wave's lanes for which `hit` holds, added to counts[s] by the first of them: one atomic. s is wave-uniform.
__device__ __forceinline__ void through_add(const ThroughParams &ap, uint32_t lane, uint32_t s, bool hit) {
	const unsigned long long b = ballot64(hit);
	if (b != 0ull && s < ap.n_counts && (int)lane == __ffsll((long long)b) - 1) atomicAdd(ap.counts + s, (uint32_t)__popcll(b));
}

// the summary: three popcounts per wave through LDS, one atomic each per workgroup (every lane of the workgroup gets here)
template <bool TARGET>
__device__ __forceinline__ void through_summary(const ThroughParams &ap, uint32_t (*sums)[2], uint32_t lane, uint32_t wave, bool m, bool miss) {
	const uint32_t n_area = (uint32_t)__popcll(ballot64(m)), n_miss = (uint32_t)__popcll(ballot64(miss));
	if (lane == 0u) sums[wave][0] = n_area, sums[wave][1] = n_miss;
	__syncthreads();
	if (threadIdx.x == 0u) {
		const uint32_t a = sums[0][0] + sums[1][0] + sums[2][0] + sums[3][0], b = sums[0][1] + sums[1][1] + sums[2][1] + sums[3][1];
		if (a) atomicAdd(ap.summary + 0, a);
		if (b) atomicAdd(ap.summary + 2, b);
		if (TARGET && a - b) atomicAdd(ap.summary + 4, a - b); // pixels with a candidate on the target, not the sum of the counts
	}
}

// scan_triangles_multi without a list: every triangle of the model accepted with t < tmax is handed to `each` with its index in
// the model. true when there was one.
template <class Each>
__device__ __forceinline__ bool scan_triangles_each(const float *__restrict__ wtris, uint32_t first, uint32_t count, f3 org, f3 dir, float tmax, Each each SRT_RC_PARAM) {
	const float *__restrict__ blk = wtris + (size_t)first * SRT_WTRI_FLOATS;
	const uint32_t npair = ((count + 3u) >> 2) << 1; // pairs, always even (the padding triangles are zero: they fail R1)
	uint32_t unused = 0u;
	bool any = false;
	auto pair = [&](const Tri2 &t, uint32_t j) {
		float t0 = 0.0f, t1 = 0.0f;
		const bool h0 = moller_trumbore<false>(t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], t.v[6], t.v[7], t.v[8], org, dir, true, t0, unused SRT_RC_ARG);
		const bool h1 = moller_trumbore<false>(t.v[9], t.v[10], t.v[11], t.v[12], t.v[13], t.v[14], t.v[15], t.v[16], t.v[17], org, dir, true, t1, unused SRT_RC_ARG);
		if (h0 && t0 < tmax) any = true, each(j);
		if (h1 && t1 < tmax) any = true, each(j + 1u);
	};
	Tri2 a = ld_tri2(blk);
	for (uint32_t b = 0; b < npair; b += 2) {
		const Tri2 c = ld_tri2(blk + 18u * (b + 1u)); // in flight while `a` is tested
		pair(a, 2u * b);
		a = ld_tri2(blk + 18u * (b + 2u)); // (one pair of slack is allocated past the end)
		pair(c, 2u * b + 2u);
	}
	return any;
}

// walk_bvh_multi without a list: the same blocks, box arithmetic, slack and stack discipline with the far side of every box
// clamped by the constant tmax (the walk under SRT_RAYS_COUNT_ALL); every triangle accepted with t < tmax is handed to `each`
// with its leaf record. true when there was one.
template <class Each>
__device__ __forceinline__ bool walk_bvh_each(const float4 *__restrict__ blocks, AnyStackEntry *__restrict__ stack, uint32_t root, f3 org, f3 dir, float tmax,
                                              Each each SRT_RC_PARAM) {
	if (root == SRT_BVH_NONE) return false;
	f3 inv;
	inv.x = dm_fabs(dir.x) >= 0x1p-100f ? 1.0f / dir.x : __builtin_copysignf(0x1p100f, dir.x);
	inv.y = dm_fabs(dir.y) >= 0x1p-100f ? 1.0f / dir.y : __builtin_copysignf(0x1p100f, dir.y);
	inv.z = dm_fabs(dir.z) >= 0x1p-100f ? 1.0f / dir.z : __builtin_copysignf(0x1p100f, dir.z);
	const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
	uint32_t unused = 0u;
	bool any = false;
	uint32_t cur = ((root & SRT_BVH_INDEX_MASK) << 5) | SRT_BVH_TAG(root, 0u);
	// the youngest waiting entry in registers, stack[0 .. sp) the older ones, under them the sentinel (as walk_bvh_any)
	uint32_t sp = 0u;
	uint32_t top = SRT_BVH_NONE;
	stack[0] = SRT_BVH_NONE;
	while (cur != SRT_BVH_NONE) {
		uint32_t next = SRT_BVH_NONE;
		const uint32_t at = (cur >> 5) << 7;
		const float4 q0 = bvh_quarter(blocks, at, 0u), q1 = bvh_quarter(blocks, at, 16u), q2 = bvh_quarter(blocks, at, 32u);
		if (cur & SRT_BVH_TAG_LEAF) {
			const uint32_t cnt = (cur >> 2) & 3u, rec0 = (cur >> 5) << 2;
			const float4 q3 = bvh_quarter(blocks, at, 48u), q4 = bvh_quarter(blocks, at, 64u);
#if SRT_BVH_LEAF_MAX > 2
			const float4 q5 = bvh_quarter(blocks, at, 80u), q6 = bvh_quarter(blocks, at, 96u);
#else
			const float4 q5 = q3, q6 = q3;
#endif
			auto tri = [&](float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, uint32_t slot) {
				float t = 0.0f;
				if (moller_trumbore<false>(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, org, dir, true, t, unused SRT_RC_ARG) && t < tmax) any = true, each(rec0 + slot);
			};
			tri(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, 0u);
			if (cnt > 1u) tri(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, 1u);
			if (cnt > 2u) tri(q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, 2u);
		} else {
			const uint32_t ex = f2u(q0.w), nk = ex >> 24;
			const float gx = dm_u2f((ex & 255u) << 23), gy = dm_u2f(((ex >> 8) & 255u) << 23), gz = dm_u2f(((ex >> 16) & 255u) << 23);
			const float cx = q0.x - org.x, cy = q0.y - org.y, cz = q0.z - org.z;
			const uint32_t nxw = sx ? f2u(q1.w) : f2u(q1.x), fxw = sx ? f2u(q1.x) : f2u(q1.w);
			const uint32_t nyw = sy ? f2u(q2.x) : f2u(q1.y), fyw = sy ? f2u(q1.y) : f2u(q2.x);
			const uint32_t nzw = sz ? f2u(q2.y) : f2u(q1.z), fzw = sz ? f2u(q1.z) : f2u(q2.y);
			const uint32_t tags = f2u(q2.z), first = f2u(q2.w);
			auto entry = [&](int c, bool there) -> bool {
				auto at_byte = [c](uint32_t word) { return (float)((word >> (8 * c)) & 255u); };
				const float tnx = dm_fmaf(at_byte(nxw), gx, cx) * inv.x, tfx = dm_fmaf(at_byte(fxw), gx, cx) * inv.x;
				const float tny = dm_fmaf(at_byte(nyw), gy, cy) * inv.y, tfy = dm_fmaf(at_byte(fyw), gy, cy) * inv.y;
				const float tnz = dm_fmaf(at_byte(nzw), gz, cz) * inv.z, tfz = dm_fmaf(at_byte(fzw), gz, cz) * inv.z;
				const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz), 0.0f);
				const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), tmax);
				return tn <= tf * 1.000001f && there;
			};
			// the first child the ray enters is next, the others wait in slot order: one store each
			auto child = [&](int c, bool there) {
				if (entry(c, there)) {
					const uint32_t ref = ((first + (uint32_t)c) << 5) | ((tags >> (8 * c)) & SRT_BVH_TAG_MASK);
					if (next == SRT_BVH_NONE) next = ref;
					else stack[sp] = top, top = ref, sp += 1u;
				}
			};
			child(0, true), child(1, true), child(2, nk > 2u), child(3, nk > 3u);
		}
		if (next == SRT_BVH_NONE) { // nothing to enter from here: the youngest waiting child, or the sentinel
			next = top;
			sp = sp > 0u ? sp - 1u : 0u;
			top = stack[sp];
		}
		cur = next;
	}
	return any;
}

} // namespace

// What both kernels start with: the lasso into LDS, the lane's pixel and M(p), and for the lanes inside M the pixel centre's ray
// as the ID pass makes and refuses it. Declares lane, wave, m, org, dir, tmax, valid.
#define SRT_THROUGH_HEAD                                                                                                                           \
	const ThroughParams &ap = through_base(args);                                                                                                  \
	const TraceParams &p = ap.tp;                                                                                                                  \
	__shared__ int32_t lasso[LASSO ? 2 * SRT_AREA_MAX_VERTICES : 2];                                                                               \
	__shared__ uint32_t sums[4][2];                                                                                                                \
	const uint32_t lane = threadIdx.x & 63u;                                                                                                       \
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                                                       \
	if constexpr (LASSO) {                                                                                                                         \
		for (uint32_t i = threadIdx.x; i < 2u * ap.n_vertices; i += 256u) lasso[i] = args.v2[i]; /* n_vertices <= SRT_AREA_MAX_VERTICES */          \
		__syncthreads();                                                                                                                           \
	}                                                                                                                                              \
	const uint32_t col_group = blockIdx.x % ap.col_groups, row_group = blockIdx.x / ap.col_groups;                                                 \
	const int32_t y = ap.y0 + (int32_t)(row_group * 4u + wave); /* the wave's row */                                                               \
	const int32_t x = ap.x0 + (int32_t)(col_group * 64u + lane);                                                                                   \
	const bool m = through_mask<LASSO>(ap, lasso, x, y);                                                                                           \
	f3 org = mk(0.f, 0.f, 0.f), dir = org;                                                                                                         \
	if (m) camera_ray(p, make_float2((float)x + 0.5f, (float)y + 0.5f), org, dir);                                                                 \
	const float tmax = DM_INF_F;                                                                                                                   \
	const uint32_t flags = SRT_RAYS_UNIT_DIRECTIONS;

template <bool LASSO, bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(256) void srt_area_through_kernel(const typename ThroughArgs<LASSO>::type args) {
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	SRT_THROUGH_HEAD
#include "ray_valid.inc"
	bool found = false; // the lane's ray has a candidate
	if (m && valid) {   // (the ballots below are over the lanes in here; a wave with no lane in M walks nothing)
		AnyStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_model = [&](float lx, float ly, float lz, float hx, float hy, float hz, uint32_t ref, uint32_t count, int idx) {
			bool hit = false;
			if (test_aabb(lx, ly, lz, hx, hy, hz, org, inv, tmax)) // the model's box against the constant limit, then existence alone
				hit = USE_BVH ? walk_bvh_any(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, ref, org, dir, tmax SRT_RC_ARG)
				              : test_triangles_any(p.wtris, ref, count, org, dir, tmax SRT_RC_ARG);
			found = found || hit;
			through_add(ap, lane, (uint32_t)idx, hit); // (reconverged)
		};
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u, cnt = (code >> 2) & 7u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
#pragma unroll
				for (int i = 0; i < 4; i++) {
					if ((uint32_t)i < cnt) { // (wave-uniform)
						float t;
						const bool hit = sphere_hit_t(b.v + 4 * i, org, dir, t) && t < tmax;
						found = found || hit;
						through_add(ap, lane, (uint32_t)(base + i), hit);
					}
				}
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
#pragma unroll
				for (int i = 0; i < 2; i++) {
					if ((uint32_t)i < cnt) {
						float t;
						const bool hit = plane_hit_t(b.v + 8 * i, org, dir, t) && t < tmax;
						found = found || hit;
						through_add(ap, lane, (uint32_t)(base + i), hit);
					}
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
	through_summary<false>(ap, sums, lane, wave, m, m && !found);
}

template <bool LASSO, bool USE_BVH>
__global__ __launch_bounds__(256) void srt_area_through_triangles_kernel(const typename ThroughArgs<LASSO>::type args) {
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	SRT_THROUGH_HEAD
#include "ray_valid.inc"
	bool found = false; // the lane's ray has a candidate on the target
	if (m && valid) {
		AnyStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		const float4 *const blocks = reinterpret_cast<const float4 *>(p.bvh_blocks);
		const f3 inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_model = [&](float lx, float ly, float lz, float hx, float hy, float hz, uint32_t ref, uint32_t count) {
			if (test_aabb(lx, ly, lz, hx, hy, hz, org, inv, tmax)) {
				if (USE_BVH) {
					found = walk_bvh_each(blocks, bvh_stack, ref, org, dir, tmax, [&](uint32_t rec) {
						const uint32_t k = bvh_tri_in_model(blocks, rec);
						if (k < ap.n_counts) atomicAdd(ap.counts + k, 1u);
					} SRT_RC_ARG);
				} else {
					found = scan_triangles_each(p.wtris, ref, count, org, dir, tmax, [&](uint32_t k) {
						if (k < ap.n_counts) atomicAdd(ap.counts + k, 1u);
					} SRT_RC_ARG);
				}
			}
		};
		for (int g = 0; g < p.num_runs; g++) { // (wave-uniform) the one block that holds the target
			float gh[4];
			ld_uniform<4, 16>(reinterpret_cast<const float *>(p.runs + g), gh);
			const uint32_t code = f2u(gh[0]);
			const float *__restrict__ gd = p.run_data + 48 * g;
#pragma unroll
			for (int j = 0; j < 3; j++) {
				const uint32_t c = (code >> (8 * j)) & 255u, base = f2u(gh[1 + j]);
				if ((c & 3u) != SRT_SHAPE_MODEL + 1u || ap.target - base >= ((c >> 2) & 7u)) continue; // (unsigned: target < base wraps)
				const Blk16 b = ld_blk16(gd + 16 * j);
				if (ap.target == base) test_model(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], f2u(b.v[3]), f2u(b.v[7]));
				else test_model(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], f2u(b.v[11]), f2u(b.v[15]));
			}
		}
	}
	through_summary<true>(ap, sums, lane, wave, m, m && !found);
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

template <class K, bool LASSO>
void launch_through(K kernel, const ThroughParams &ap, const int32_t *v2, uint32_t blocks, hipStream_t stream) {
	typename ThroughArgs<LASSO>::type args;
	if constexpr (LASSO) {
		memset(&args, 0, sizeof args);
		args.a = ap;
		memcpy(args.v2, v2, 2 * sizeof(int32_t) * ap.n_vertices);
	} else {
		args = ap;
	}
	hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, args);
}

template <bool LASSO>
void launch_shapes(const ThroughParams &ap, const int32_t *v2, uint32_t blocks, hipStream_t stream) {
	if (!(ap.tp.num_models > 0)) launch_through<decltype(&srt_area_through_kernel<LASSO, false, false>), LASSO>(srt_area_through_kernel<LASSO, false, false>, ap, v2, blocks, stream);
	else if (ap.tp.use_bvh != 0) launch_through<decltype(&srt_area_through_kernel<LASSO, true, true>), LASSO>(srt_area_through_kernel<LASSO, true, true>, ap, v2, blocks, stream);
	else launch_through<decltype(&srt_area_through_kernel<LASSO, true, false>), LASSO>(srt_area_through_kernel<LASSO, true, false>, ap, v2, blocks, stream);
}
template <bool LASSO>
void launch_triangles(const ThroughParams &ap, const int32_t *v2, uint32_t blocks, hipStream_t stream) {
	if (ap.tp.use_bvh != 0) launch_through<decltype(&srt_area_through_triangles_kernel<LASSO, true>), LASSO>(srt_area_through_triangles_kernel<LASSO, true>, ap, v2, blocks, stream);
	else launch_through<decltype(&srt_area_through_triangles_kernel<LASSO, false>), LASSO>(srt_area_through_triangles_kernel<LASSO, false>, ap, v2, blocks, stream);
}

// What every through call does first: the block and the frame checked. No ID planes are made or read
int through_begin(srt_tracer *t, const char *who, const srt_render_data *options, const srt_area *area, const int32_t *vertices) {
	if (!options) return fail(t, SRT_ERR_INVALID, std::string(who) + ": options is required (there are no ID planes to fall back on)");
	if (area_check(area, vertices) != SRT_OK) return fail(t, SRT_ERR_INVALID, std::string(who) + ": the area is refused (srt_area_check_host)");
	if (area_through_frame_check(options->width, options->height) != SRT_OK)
		return fail(t, SRT_ERR_INVALID, std::string(who) + ": options->width and height must be positive and the frame below 2^31 pixels");
	SRT_HIP(t, hipSetDevice(t->device));
	t->ar.last_id_ran = false;
	return SRT_OK;
}

// the clear and the launches into counts (n words, of which n_counts are counted) and summary (8 words), both on the device, on
// the handle's stream
int enqueue_through(srt_tracer *t, const srt_render_data &rd, const srt_area &area, const int32_t *vertices, bool by_triangle, uint32_t target, uint32_t *counts,
                    size_t n, uint32_t n_counts, uint32_t *summary, bool one_block) {
	if (const int rc = srt_area_clear(t, counts, n, summary, one_block)) return rc;
	AreaThroughGrid grid;
	area_through_grid(area, rd.width, rd.height, &grid);
	if (grid.blocks) { // else: all zeros, nothing to launch
		ThroughParams ap;
		memset(&ap, 0, sizeof ap);
		ap.tp = srt_trace_params_for_query(t, &rd);
		ap.counts = counts, ap.summary = summary;
		ap.n_counts = n_counts, ap.target = target;
		ap.x0 = grid.c[0], ap.y0 = grid.c[1], ap.x1 = grid.c[2], ap.y1 = grid.c[3];
		ap.col_groups = grid.col_groups;
		ap.n_vertices = area.n_vertices;
		if (area.n_vertices) {
			int32_t v2[2 * SRT_AREA_MAX_VERTICES], yr[2];
			area_double(vertices, area.n_vertices, v2, yr);
			ap.ylo2 = yr[0], ap.yhi2 = yr[1];
			if (by_triangle) launch_triangles<true>(ap, v2, grid.blocks, t->stream);
			else launch_shapes<true>(ap, v2, grid.blocks, t->stream);
		} else {
			if (by_triangle) launch_triangles<false>(ap, nullptr, grid.blocks, t->stream);
			else launch_shapes<false>(ap, nullptr, grid.blocks, t->stream);
		}
		SRT_HIP(t, hipGetLastError());
	}
	return srt_area_finish(t, counts, n_counts, summary, grid.blocks != 0u);
}

uint32_t scene_shapes(const srt_tracer *t) { return t->scene_set ? (uint32_t)t->sd.num_shapes : 0u; }

} // namespace

extern "C" {

int srt_area_coverage_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                              srt_area_summary *out) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !out) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through: NULL argument");
	const uint32_t n = scene_shapes(t);
	if (cap_shapes < n || (n && !counts)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through: counts is smaller than the scene's shape count");
	try {
		if (const int rc = through_begin(t, "srt_area_coverage_through", options, area, vertices)) return rc;
		return srt_area_result_host(t, n, counts, out, [&](uint32_t *d_counts, uint32_t *d_summary) {
			return enqueue_through(t, *options, *area, vertices, false, 0u, d_counts, n, n, d_summary, true);
		});
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_area_triangle_coverage_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                       uint32_t *counts, size_t cap_triangles, srt_area_summary *out) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !out) return fail(t, SRT_ERR_INVALID, "srt_area_triangle_coverage_through: NULL argument");
	try {
		if (const int rc = through_begin(t, "srt_area_triangle_coverage_through", options, area, vertices)) return rc;
		uint32_t n = 0;
		if (const int rc = srt_area_model_triangles(t, "srt_area_triangle_coverage_through", shape, &n)) return rc;
		if (cap_triangles < n || (n && !counts))
			return fail(t, SRT_ERR_INVALID, "srt_area_triangle_coverage_through: counts is smaller than the model's triangle count");
		return srt_area_result_host(t, n, counts, out, [&](uint32_t *d_counts, uint32_t *d_summary) {
			return enqueue_through(t, *options, *area, vertices, true, shape, d_counts, n, n, d_summary, true);
		});
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_area_coverage_through_device(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *d_counts, size_t n,
                                     uint32_t *d_summary) {
	if (!t) return SRT_ERR_INVALID;
	if (!area || !d_summary) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through_device: NULL argument");
	const uint32_t n_shapes = scene_shapes(t);
	if (n < n_shapes || (n && !d_counts)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through_device: d_counts is smaller than the scene's shape count");
	if (n >= ((size_t)1 << 31)) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through_device: n must stay below 2^31");
	if (((uintptr_t)d_counts | (uintptr_t)d_summary) & 3u) return fail(t, SRT_ERR_INVALID, "srt_area_coverage_through_device: arrays must be aligned to 4 bytes");
	if (const int rc = through_begin(t, "srt_area_coverage_through_device", options, area, vertices)) return rc;
	return enqueue_through(t, *options, *area, vertices, false, 0u, d_counts, n, n_shapes, d_summary, false);
}

int srt_select_area_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                            size_t *n_selected) {
	if (!t) return SRT_ERR_INVALID;
	if (mode < SRT_SELECT_REPLACE || mode > SRT_SELECT_TOGGLE)
		return fail(t, SRT_ERR_INVALID, "srt_select_area_through: mode is SRT_SELECT_REPLACE, ADD, SUBTRACT or TOGGLE");
	if (!area) return fail(t, SRT_ERR_INVALID, "srt_select_area_through: NULL argument");
	try {
		std::vector<uint32_t> counts(scene_shapes(t));
		srt_area_summary sum;
		if (const int rc = srt_area_coverage_through(t, options, area, vertices, counts.data(), counts.size(), &sum)) return rc;
		return srt_area_select_counts(t, counts.data(), counts.size(), mode, min_pixels, n_selected);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_pick_rays(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, srt_ray *rays_out) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = query_check_count(t, "srt_pick_rays", n, 0u)) return rc;
	if (n == 0) return SRT_OK;
	if (!options || !xy || !rays_out) return fail(t, SRT_ERR_INVALID, "srt_pick_rays: NULL argument");
	if (options->width <= 0 || options->height <= 0) return fail(t, SRT_ERR_INVALID, "srt_pick_rays: options->width and height must be positive");
	SRT_HIP(t, hipSetDevice(t->device));
	QueryStage st;
	if (const int rc = query_reserve_stage(t, n, &st)) return rc;
	uint8_t *const stage = t->rq_stage.ptr;
	SRT_HIP(t, hipMemcpyAsync(stage + st.xy, xy, n * 2 * sizeof(float), hipMemcpyHostToDevice, t->stream));
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = srt_enqueue_pick_rays(t, options, stage + st.xy, n, stage + st.rays)) return rc;
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(rays_out, stage + st.rays, n * sizeof(srt_ray), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

} // extern "C"
