// device_multihit.h -- the multi-hit forms of device_intersect.h's tests, for the multi-hit kernel (multi_hit.hip): "the first K
// candidates of a ray in order", not "the closest". A candidate is a primitive whose own intersector accepts the ray with
// t < tmax (include/srt_abi.h "multi-hit ray queries"); the order is t as a float, then the shape index, then the triangle index
// inside the model. What a lane keeps is a sorted list of up to CAP entries in REGISTERS: every index into it is a compile-time
// constant (the insertion and every read are unrolled over CAP), so nothing of it goes to scratch. Boxes, slack and
// moller_trumbore are device_intersect.h's own, the walk is device_anyhit.h's without its early exit.
#ifndef SRT_DEVICE_MULTIHIT_H
#define SRT_DEVICE_MULTIHIT_H

#include "device_anyhit.h"

namespace {

// The lane's list: entries [0, min(total, CAP)) in order, the others empty (t = +inf, shape = NONE: a candidate has t < tmax <=
// +inf, so it precedes every empty entry by t alone). ref: the triangle inside its model (scan), its leaf record (hierarchy),
// SRT_HIT_NONE for a sphere or a plane. kth: the t of entry k - 1 (+inf while the list holds fewer than k) -- what a candidate
// must not exceed to enter; equal t reaches the comparison.
template <int CAP>
struct HitList {
	float t[CAP];
	uint32_t shape[CAP];
	uint32_t ref[CAP];
	float kth;
	uint32_t total; // candidates offered with t < tmax: all of them under SRT_RAYS_COUNT_ALL, at least min(k, all) otherwise
};

template <int CAP>
__device__ __forceinline__ void list_clear(HitList<CAP> &L) {
#pragma unroll
	for (int i = 0; i < CAP; i++) L.t[i] = DM_INF_F, L.shape[i] = SRT_HIT_NONE, L.ref[i] = SRT_HIT_NONE;
	L.kth = DM_INF_F;
	L.total = 0u;
}

// entry j of the list for a wave-uniform j: a chain of selects, no indexing
template <int CAP>
__device__ __forceinline__ void list_get(const HitList<CAP> &L, uint32_t j, float &t, uint32_t &shape, uint32_t &ref) {
	t = L.t[0], shape = L.shape[0], ref = L.ref[0];
#pragma unroll
	for (int i = 1; i < CAP; i++) {
		const bool here = j == (uint32_t)i;
		t = here ? L.t[i] : t, shape = here ? L.shape[i] : shape, ref = here ? L.ref[i] : ref;
	}
}

// does candidate (ct, cs, cr) stand before entry (et, es, er): t as floats (-0 == +0; no NaN gets here), then the shape, then
// the triangle inside the model -- under a hierarchy fetched from the two leaf records, only when t and shape tie
template <bool USE_BVH>
__device__ __forceinline__ bool hit_precedes(const float4 *__restrict__ blocks, float ct, uint32_t cs, uint32_t cr, float et, uint32_t es, uint32_t er) {
	bool before = ct < et;
	if (ct == et) {
		before = cs < es;
		if (cs == es) before = USE_BVH ? bvh_tri_in_model(blocks, cr) < bvh_tri_in_model(blocks, er) : cr < er;
	}
	return before;
}

// Sorted insertion, unrolled: the candidate moves down the list until it stands before an entry, from there on every entry
// moves one slot down (no comparison: the list was in order) and the last one drops out. k: the caller's K (1 .. CAP).
template <int CAP, bool USE_BVH>
__device__ __forceinline__ void list_insert(HitList<CAP> &L, const float4 *__restrict__ blocks, uint32_t k, float t, uint32_t shape, uint32_t ref) {
	bool moved = false;
#pragma unroll
	for (int i = 0; i < CAP; i++) {
		if (!moved) moved = hit_precedes<USE_BVH>(blocks, t, shape, ref, L.t[i], L.shape[i], L.ref[i]);
		const float et = L.t[i];
		const uint32_t es = L.shape[i], er = L.ref[i];
		L.t[i] = moved ? t : et, L.shape[i] = moved ? shape : es, L.ref[i] = moved ? ref : er;
		t = moved ? et : t, shape = moved ? es : shape, ref = moved ? er : ref;
	}
	float kth = L.t[0];
#pragma unroll
	for (int i = 1; i < CAP; i++) kth = k == (uint32_t)(i + 1) ? L.t[i] : kth;
	L.kth = kth;
}

// a primitive's own intersector has accepted the ray at t: a candidate when t < tmax (a NaN is none), kept when it does not lie
// behind the k-th
template <int CAP, bool USE_BVH>
__device__ __forceinline__ void list_offer(HitList<CAP> &L, const float4 *__restrict__ blocks, uint32_t k, float tmax, float t, uint32_t shape, uint32_t ref) {
	if (t < tmax) {
		L.total += 1u;
		if (t <= L.kth) list_insert<CAP, USE_BVH>(L, blocks, k, t, shape, ref);
	}
}

// the far limit of a box test: tmax when everything is counted, else the k-th entry's t once there is one (inclusive: the box
// tests compare tn <= tf * 1.000001f)
template <int CAP>
__device__ __forceinline__ float list_limit(const HitList<CAP> &L, float tmax, bool count_all) {
	return count_all ? tmax : __builtin_fminf(tmax, L.kth);
}

// ---- spheres and planes: intersect_sphere's and intersect_plane's t for EVERY primitive of a block ----
// render.cl:180-204 on one sphere {cx, cy, cz, r*r} of a block: the reference's sequence with the IEEE root (what test_spheres
// runs on its slow path). A filler (r*r = -inf) has a discriminant of -inf or NaN: never accepted, or accepted with a NaN t,
// which is no candidate.
__device__ __forceinline__ bool sphere_hit_t(const float *s, f3 org, f3 dir, float &t) {
	const f3 L = mk(s[0] - org.x, s[1] - org.y, s[2] - org.z);
	const float bq = dot3(L, dir);
	const float c = dot3(L, L) - s[3];
	const float disc = bq * bq - c;
	const float sq = __builtin_sqrtf(disc);
	t = bq - sq;
	if (t < 0.0f) t = bq + sq;
	return !(disc < 0.0f) && !(t < 0.0f);
}
// render.cl:206-221 on one plane {p, 0, n, 0} of a block: test_planes2's statements. denom == 0 needs no test of its own: the
// quotient is +-inf or NaN, and neither +inf nor a NaN is below tmax, -inf is below 0.
__device__ __forceinline__ bool plane_hit_t(const float *b, f3 org, f3 dir, float &t) {
	const f3 n = mk(b[4], b[5], b[6]);
	const float denom = dot3(n, dir);
	t = dot3(n, mk(b[0] - org.x, b[1] - org.y, b[2] - org.z)) / denom;
	return !(t < 0.0f);
}

// ---- models ----
// test_triangles for the list: the same wave-uniform pair loads, every accepted triangle offered with its index in the model
template <int CAP>
__device__ __forceinline__ void scan_triangles_multi(const float *__restrict__ wtris, uint32_t first, uint32_t count, f3 org, f3 dir, uint32_t shape, uint32_t k,
                                                     float tmax, HitList<CAP> &L SRT_RC_PARAM) {
	const float *__restrict__ blk = wtris + (size_t)first * SRT_WTRI_FLOATS;
	const uint32_t npair = ((count + 3u) >> 2) << 1; // pairs, always even (the padding triangles are zero: they fail R1)
	uint32_t unused = 0u;
	auto pair = [&](const Tri2 &t, uint32_t j) {
		float t0 = 0.0f, t1 = 0.0f;
		const bool h0 = moller_trumbore<false>(t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], t.v[6], t.v[7], t.v[8], org, dir, true, t0, unused SRT_RC_ARG);
		const bool h1 = moller_trumbore<false>(t.v[9], t.v[10], t.v[11], t.v[12], t.v[13], t.v[14], t.v[15], t.v[16], t.v[17], org, dir, true, t1, unused SRT_RC_ARG);
		if (h0) list_offer<CAP, false>(L, nullptr, k, tmax, t0, shape, j);
		if (h1) list_offer<CAP, false>(L, nullptr, k, tmax, t1, shape, j + 1u);
	};
	Tri2 a = ld_tri2(blk);
	for (uint32_t b = 0; b < npair; b += 2) {
		const Tri2 c = ld_tri2(blk + 18u * (b + 1u)); // in flight while `a` is tested
		pair(a, 2u * b);
		a = ld_tri2(blk + 18u * (b + 2u)); // (one pair of slack is allocated past the end)
		pair(c, 2u * b + 2u);
	}
}

// walk_bvh_any without the early exit: per lane over the same blocks, the same box arithmetic, slack and stack discipline; the
// far side of a box is clamped by the list's current limit, and every accepted triangle is offered with its leaf record.
// A waiting child was tested against the limit that held when its parent was visited; the 4-byte entries keep no distance, so
// it is not tested again when it is popped although the k-th entry's t may have shrunk since: such a stale child is walked (its
// own children and triangles meet the current limit). Correct, only less pruning than keyed entries would give; not measured.
template <int CAP>
__device__ __forceinline__ void walk_bvh_multi(const float4 *__restrict__ blocks, AnyStackEntry *__restrict__ stack, uint32_t root, f3 org, f3 dir, uint32_t shape,
                                               uint32_t k, float tmax, bool count_all, HitList<CAP> &L SRT_RC_PARAM) {
	if (root == SRT_BVH_NONE) return;
	// 1/d, or +-2^100 where |d| < 2^-100, and the planes a ray meets first: as walk_bvh
	f3 inv;
	inv.x = dm_fabs(dir.x) >= 0x1p-100f ? 1.0f / dir.x : __builtin_copysignf(0x1p100f, dir.x);
	inv.y = dm_fabs(dir.y) >= 0x1p-100f ? 1.0f / dir.y : __builtin_copysignf(0x1p100f, dir.y);
	inv.z = dm_fabs(dir.z) >= 0x1p-100f ? 1.0f / dir.z : __builtin_copysignf(0x1p100f, dir.z);
	const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
	uint32_t unused = 0u;
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
				if (moller_trumbore<false>(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, org, dir, true, t, unused SRT_RC_ARG))
					list_offer<CAP, true>(L, blocks, k, tmax, t, shape, rec0 + slot);
			};
			tri(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, 0u);
			if (cnt > 1u) tri(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, 1u);
			if (cnt > 2u) tri(q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, 2u);
		} else {
			const float lim = list_limit(L, tmax, count_all);
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
				const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), lim);
				return tn <= tf * 1.000001f && there; // inclusive: a candidate of the k-th entry's t is not pruned
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
}

} // namespace

#endif
