// device_nearest.h -- the nearest-surface query's parts (nearest.hip): the best-so-far record, the conservative pruning bound,
// the wave-uniform triangle scan and the per-lane point-to-box walk over the wide hierarchy. The distance functions themselves
// are nearest_math.h, the text the host exports compile too.
//
// PRUNING. The answer is the minimum of nm_*'s `distance` over the primitives, ties to the lower index; a box (a model record's,
// a child's decoded byte box) may only be left out when no triangle inside it can reach or TIE the best distance so far. Box
// distance and triangle distance come out of different rounded paths, so "inside the box" does not by itself order the two
// floats. What holds (DESIGN.md 31 has the derivation): every triangle under a box has its three vertices a, a + e1, a + e2,
// as floats, inside the box (the builder's boxes contain them and are rounded outwards, bvh_host.cpp, bvh_device.h
// triangle_box), so in exact arithmetic its distance is at least the box's. nm_triangle's point differs from a point of the
// exact triangle by rounding errors of its coordinates, which are relative to the COORDINATES' magnitude, not to the
// distance: at most a few dozen units of 2^-24 (B + Q), B the largest |coordinate| of the model's box, Q of the query point;
// the box distance's own error (origin - q, one fmaf, squares and two sums) is of the same kind and smaller. So
//     slack = (B + Q) * 2^-17      (128 such units: several times the bound)
// is added to the best distance, and the squares are compared with a relative margin of 1e-5 (84 ulp, for the squarings, the
// sums and the square root between `distance` and its square), strictly:
//     skip a box  <=>  d2(box) > ((best + slack)^2) * 1.00001f
// A box at exactly the best distance is therefore visited (the tie rule may prefer a triangle in it). Every comparison is
// written so that a NaN anywhere (hostile boxes, overflow) means "visit". tests/test_gpu_nearest.py compares every word of every
// record with the brute force under every mode, far from the origin included.
#ifndef SRT_DEVICE_NEAREST_H
#define SRT_DEVICE_NEAREST_H

#include "device_math.h"
#include "device_intersect.h" // the scalar-load blocks, BvhStackEntry, bvh_quarter, bvh_tri_in_model, bvh_order2
#include "nearest_math.h"

namespace {

struct NearestBest {
	float d;      // the distance to beat: max_distance at first, the closest primitive's afterwards
	int shape;    // -1: nothing yet
	uint32_t rec; // the triangle inside its model (scan) or its leaf record (hierarchy); SRT_HIT_NONE for a sphere or a plane
	float px, py, pz;
	uint32_t flags; // nm_result's
};

__device__ __forceinline__ void nearest_take(NearestBest &b, const nm_result &r, int shape, uint32_t rec) {
	b.d = r.distance, b.shape = shape, b.rec = rec;
	b.px = r.px, b.py = r.py, b.pz = r.pz, b.flags = r.flags;
}

// the squared distance beyond which a box cannot matter (PRUNING above); +inf while nothing is found under max_distance = +inf
__device__ __forceinline__ float nearest_reach2(float best, float slack) {
	const float r = best + slack;
	return (r * r) * 1.00001f;
}
// max(lo - q, q - hi, 0) from lo - q and hi - q; v_max_f32 drops a NaN operand, which errs towards "near"
__device__ __forceinline__ float nearest_gap(float lo_q, float hi_q) { return __builtin_fmaxf(__builtin_fmaxf(lo_q, -hi_q), 0.0f); }
__device__ __forceinline__ float nearest_box_d2(float gx, float gy, float gz) { return (gx * gx + gy * gy) + gz * gz; }

// ---- array scan: every lane tests the same triangle, fetched by scalar loads two at a time (test_triangles' loop and prefetch) ----
// The padding triangles past `count` are all zeros -- for this query a point at the world origin -- so they are left out by
// `count` (wave-uniform), not by a test that fails. Ascending j and a strict compare keep the lower index of equal distances.
__device__ __forceinline__ void nearest_pair(const Tri2 &t, f3 q, int idx, uint32_t j, uint32_t count, NearestBest &best) {
	if (j < count) {
		const nm_result r = nm_triangle(t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], t.v[6], t.v[7], t.v[8], q.x, q.y, q.z);
		if (r.distance < best.d) nearest_take(best, r, idx, j);
	}
	if (j + 1u < count) {
		const nm_result r = nm_triangle(t.v[9], t.v[10], t.v[11], t.v[12], t.v[13], t.v[14], t.v[15], t.v[16], t.v[17], q.x, q.y, q.z);
		if (r.distance < best.d) nearest_take(best, r, idx, j + 1u);
	}
}
__device__ __forceinline__ void nearest_scan(const float *__restrict__ wtris, uint32_t first, uint32_t count, f3 q, int idx, NearestBest &best) {
	const float *__restrict__ blk = wtris + (size_t)first * SRT_WTRI_FLOATS;
	const uint32_t npair = ((count + 3u) >> 2) << 1; // pairs, always even (the model's records are padded to a multiple of 4)
	Tri2 a = ld_tri2(blk);
	for (uint32_t b = 0; b < npair; b += 2) {
		const Tri2 c = ld_tri2(blk + 18u * (b + 1u)); // in flight while `a` is tested
		nearest_pair(a, q, idx, 2u * b, count, best);
		a = ld_tri2(blk + 18u * (b + 2u)); // (one pair of slack is allocated past the end)
		nearest_pair(c, q, idx, 2u * b + 2u, count, best);
	}
}

// ---- hierarchy: a per-lane walk over the 128-byte blocks, nearest child first, with a shrinking radius ----
// walk_bvh's block layout, tags, one-dword keys and stack discipline (device_intersect.h), with the squared point-to-box
// distance where the ray walk has the entry distance: the four children's byte boxes are decoded relative to the point with the
// walk's own fmaf(byte, 2^e, origin - q), the nearest child that is not beyond the bound is entered, the others that are not
// wait on the stack, nearest youngest, and a popped entry is tested again against the bound as the best has shrunk it since.
// The push pattern is the ray walk's -- enter one child, push up to three -- so SRT_BVH_STACK_CAP and the host's depth check
// (bvh_host.cpp fold_wide, scene_prep.cpp) cover this walk too. A key's low five bits are the tag: the distance is rounded
// DOWN, which only lets a child in. Leaves hold cnt triangles (the tag's): unused slots are zero triangles, a point at the
// origin here, and are never looked at. A triangle's index inside the model (SRT_BVH_LEAF_J) is fetched only where a
// candidate ties the best of the same model.
__device__ __forceinline__ void nearest_walk(const float4 *__restrict__ blocks, BvhStackEntry *__restrict__ stack, uint32_t root, f3 q, int idx, float slack,
                                             NearestBest &best) {
	uint32_t cur = root == SRT_BVH_NONE ? SRT_BVH_NONE : (root & SRT_BVH_INDEX_MASK);
	uint32_t cur_key = SRT_BVH_TAG(root, 0u);
	// the youngest waiting entry in registers, the older ones in stack[0 .. sp); under them a sentinel that always passes and
	// leads to block NONE
	uint32_t top_key = 0u, top_first = SRT_BVH_NONE;
	uint32_t sp = 0u;
	stack[0].key = 0u, stack[0].first = SRT_BVH_NONE;
	while (cur != SRT_BVH_NONE) {
		bool pending = true;
		uint32_t next = SRT_BVH_NONE, next_key = 0u;
		bool inner = false;
		uint32_t k0 = SRT_BVH_KEY_INF, k1 = SRT_BVH_KEY_INF, k2 = SRT_BVH_KEY_INF, k3 = SRT_BVH_KEY_INF, first = 0u;
		{
			const bool leaf = (cur_key & SRT_BVH_TAG_LEAF) != 0u;
			const uint32_t at = cur << 7;
			const float4 q0 = bvh_quarter(blocks, at, 0u), q1 = bvh_quarter(blocks, at, 16u), q2 = bvh_quarter(blocks, at, 32u);
			if (leaf) {
				const uint32_t cnt = (cur_key >> 2) & 3u, rec0 = cur << 2;
				const float4 q3 = bvh_quarter(blocks, at, 48u), q4 = bvh_quarter(blocks, at, 64u);
				const float4 q5 = bvh_quarter(blocks, at, 80u), q6 = bvh_quarter(blocks, at, 96u);
				auto tri = [&](float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, uint32_t k) {
					const nm_result r = nm_triangle(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, q.x, q.y, q.z);
					bool wins = r.distance < best.d;
					if (r.distance == best.d && best.shape == idx) // a tie inside the model: the lower triangle index (fetched only here)
						wins = bvh_tri_in_model(blocks, rec0 + k) < bvh_tri_in_model(blocks, best.rec);
					if (wins) nearest_take(best, r, idx, rec0 + k);
				};
				if (cnt > 0u) tri(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, 0u);
				if (cnt > 1u) tri(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, 1u);
				if (cnt > 2u) tri(q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, 2u);
			} else {
				const uint32_t ex = f2u(q0.w), nk = ex >> 24;
				const float gx = dm_u2f((ex & 255u) << 23), gy = dm_u2f(((ex >> 8) & 255u) << 23), gz = dm_u2f(((ex >> 16) & 255u) << 23);
				const float cx = q0.x - q.x, cy = q0.y - q.y, cz = q0.z - q.z;
				const uint32_t lxw = f2u(q1.x), lyw = f2u(q1.y), lzw = f2u(q1.z), hxw = f2u(q1.w), hyw = f2u(q2.x), hzw = f2u(q2.y);
				const uint32_t tags = f2u(q2.z);
				first = f2u(q2.w);
				const float reach2 = nearest_reach2(best.d, slack);
				auto child = [&](int k, bool there) -> uint32_t {
					auto at_byte = [k](uint32_t word) { return (float)((word >> (8 * k)) & 255u); };
					const float ax = nearest_gap(dm_fmaf(at_byte(lxw), gx, cx), dm_fmaf(at_byte(hxw), gx, cx));
					const float ay = nearest_gap(dm_fmaf(at_byte(lyw), gy, cy), dm_fmaf(at_byte(hyw), gy, cy));
					const float az = nearest_gap(dm_fmaf(at_byte(lzw), gz, cz), dm_fmaf(at_byte(hzw), gz, cz));
					const float d2 = nearest_box_d2(ax, ay, az);
					const bool skip = d2 > reach2 || !there; // (a NaN on either side: not skipped)
					float dk = d2 >= 0.0f ? d2 : 0.0f;        // the key: a NaN sorts first, +inf below KEY_INF
					dk = dk < 0x1.fffffep127f ? dk : 0x1.fffffep127f;
					return ((skip ? SRT_BVH_KEY_INF : f2u(dk)) & ~SRT_BVH_TAG_MASK) | ((tags >> (8 * k)) & 255u);
				};
				k0 = child(0, true), k1 = child(1, true), k2 = child(2, nk > 2u), k3 = child(3, nk > 3u);
				inner = true;
			}
		}
		if (inner) {
			bvh_order2(k0, k1);
			bvh_order2(k2, k3);
			bvh_order2(k0, k2);
			bvh_order2(k1, k3);
			bvh_order2(k1, k2); // nearest first; the children that are not entered (keys >= KEY_INF) last
			const uint32_t w1 = k1 < SRT_BVH_KEY_INF ? 1u : 0u, w2 = k2 < SRT_BVH_KEY_INF ? 1u : 0u, w3 = k3 < SRT_BVH_KEY_INF ? 1u : 0u;
			const uint32_t n = w1 + w2 + w3;
			if (w1) stack[sp].key = top_key, stack[sp].first = top_first;
			if (w3) stack[sp + 1u].key = k3, stack[sp + 1u].first = first;
			if (w2) stack[sp + n - 1u].key = k2, stack[sp + n - 1u].first = first;
			top_key = w1 ? k1 : top_key, top_first = w1 ? first : top_first;
			sp += n;
			if (k0 < SRT_BVH_KEY_INF) next = first + (k0 & 3u), next_key = k0, pending = false;
		}
		// the youngest waiting child that the best so far has not put out of reach
		const float reach2 = nearest_reach2(best.d, slack);
		const uint32_t reach = reach2 < DM_INF_F ? (f2u(reach2) | SRT_BVH_TAG_MASK) : 0x7fffffffu; // (+inf or a NaN: everything)
		while (pending) {
			if (top_key <= reach) next = top_first + (top_key & 3u), next_key = top_key, pending = false;
			sp = sp > 0u ? sp - 1u : 0u;
			top_key = stack[sp].key, top_first = stack[sp].first;
		}
		cur = next, cur_key = next_key;
	}
}

} // namespace

#endif
