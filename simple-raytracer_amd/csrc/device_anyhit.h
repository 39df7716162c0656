// device_anyhit.h -- the any-hit forms of device_intersect.h's triangle scan and BVH walk, for the occlusion kernel
// (occlusion.hip): "is there a hit closer than tmax", not "which is the closest". The limit never shrinks, a lane is done at
// its first accepted hit, and there is no order among hits: no best_tri, no first-in-array-order tie rule, no
// bvh_tri_in_model fetch. Boxes, slack and moller_trumbore are device_intersect.h's own, so a triangle is accepted here
// exactly when the closest-hit forms accept it against the same limit.
#ifndef SRT_DEVICE_ANYHIT_H
#define SRT_DEVICE_ANYHIT_H

#include "device_intersect.h"

namespace {

// The walk's stack: 4-byte block references, children entered in slot order (what the early exit allows: a
// popped entry needs no distance test against a limit that never shrinks, so neither the distance nor the order is kept).
// walk_bvh's own {key, first} entries with the children sorted nearest first were measured against it and lost
// (profiles/r30_occlusion.json); that form is kept as profiles/r32_anyhit_key_stack_experiment.patch.
typedef uint32_t AnyStackEntry; // (block << 5) | tag

// test_triangles for occlusion: the pairs arrive through the same wave-uniform scalar loads, so the exit is the wave's -- one
// ballot per iteration (two pairs) over the lanes that came in. Within an iteration every lane that came in runs the tests, as
// in test_triangles, whether it is occluded already or not: taking the occluded lanes out of moller_trumbore one test at a time
// (`if (!occ && ...)`) was built first and measured 1.35 to 1.41 times the cast on the rows where nothing is occluded early --
// four more exec regions per iteration and SGPR spills in a loop that is bound by its scalar loads
// (profiles/r30_occlusion_scan_masked.json).
__device__ __forceinline__ void test_pair_any(const Tri2 &t, f3 org, f3 dir, float tmax, bool &occ SRT_RC_PARAM) {
	uint32_t unused = 0u;
	float t0 = 0.0f, t1 = 0.0f;
	const bool h0 = moller_trumbore<false>(t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], t.v[6], t.v[7], t.v[8], org, dir, true, t0, unused SRT_RC_ARG);
	const bool h1 = moller_trumbore<false>(t.v[9], t.v[10], t.v[11], t.v[12], t.v[13], t.v[14], t.v[15], t.v[16], t.v[17], org, dir, true, t1, unused SRT_RC_ARG);
	occ = occ || (h0 && t0 < tmax) || (h1 && t1 < tmax);
}

__device__ __forceinline__ bool test_triangles_any(const float *__restrict__ wtris, uint32_t first, uint32_t count, f3 org, f3 dir, float tmax SRT_RC_PARAM) {
	const float *__restrict__ blk = wtris + (size_t)first * SRT_WTRI_FLOATS;
	const uint32_t npair = ((count + 3u) >> 2) << 1; // pairs, always even (the padding triangles are zero: they fail R1)
	bool occ = false;
	Tri2 a = ld_tri2(blk);
	for (uint32_t b = 0; b < npair; b += 2) {
		const Tri2 c = ld_tri2(blk + 18u * (b + 1u)); // in flight while `a` is tested
		test_pair_any(a, org, dir, tmax, occ SRT_RC_ARG);
		a = ld_tri2(blk + 18u * (b + 2u)); // (one pair of slack is allocated past the end)
		test_pair_any(c, org, dir, tmax, occ SRT_RC_ARG);
		if (!any64(!occ)) break; // (wave-uniform) every lane that came in is occluded
	}
	return occ;
}

// walk_bvh for occlusion: per lane over the same blocks, true at the first triangle accepted with t < tmax.
__device__ __forceinline__ bool walk_bvh_any(const float4 *__restrict__ blocks, AnyStackEntry *__restrict__ stack, uint32_t root, f3 org, f3 dir, float tmax SRT_RC_PARAM) {
	if (root == SRT_BVH_NONE) return false;
	// 1/d, or +-2^100 where |d| < 2^-100, and the planes a ray meets first: as walk_bvh
	f3 inv;
	inv.x = dm_fabs(dir.x) >= 0x1p-100f ? 1.0f / dir.x : __builtin_copysignf(0x1p100f, dir.x);
	inv.y = dm_fabs(dir.y) >= 0x1p-100f ? 1.0f / dir.y : __builtin_copysignf(0x1p100f, dir.y);
	inv.z = dm_fabs(dir.z) >= 0x1p-100f ? 1.0f / dir.z : __builtin_copysignf(0x1p100f, dir.z);
	const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
	bool occ = false;
	uint32_t unused = 0u;
	// a block and what it is, in one dword: its index and the tag of device_types.h (leaf, triangles, slot)
	uint32_t cur = ((root & SRT_BVH_INDEX_MASK) << 5) | SRT_BVH_TAG(root, 0u);
	// The youngest waiting entry lives in registers, stack[0 .. sp) holds the older ones, under them a sentinel that leads to
	// block NONE: popping it ends the walk (as walk_bvh).
	uint32_t sp = 0u;
	uint32_t top = SRT_BVH_NONE;
	stack[0] = SRT_BVH_NONE;
	while (cur != SRT_BVH_NONE) {
		uint32_t next = SRT_BVH_NONE;
		const uint32_t at = (cur >> 5) << 7;
		const float4 q0 = bvh_quarter(blocks, at, 0u), q1 = bvh_quarter(blocks, at, 16u), q2 = bvh_quarter(blocks, at, 32u);
		if (cur & SRT_BVH_TAG_LEAF) {
			const uint32_t cnt = (cur >> 2) & 3u;
			const float4 q3 = bvh_quarter(blocks, at, 48u), q4 = bvh_quarter(blocks, at, 64u);
#if SRT_BVH_LEAF_MAX > 2
			const float4 q5 = bvh_quarter(blocks, at, 80u), q6 = bvh_quarter(blocks, at, 96u);
#else
			const float4 q5 = q3, q6 = q3;
#endif
			auto tri = [&](float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
				float t = 0.0f;
				if (moller_trumbore<false>(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, org, dir, true, t, unused SRT_RC_ARG) && t < tmax) occ = true;
			};
			tri(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x);
			if (!occ && cnt > 1u) tri(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y);
			if (!occ && cnt > 2u) tri(q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z);
			if (occ) break; // the lane's answer: whatever waits on its stack is left there
		} else {
			// the four children's boxes, walk_bvh's arithmetic with the far side clamped by the constant tmax
			const uint32_t ex = f2u(q0.w), nk = ex >> 24;
			const float gx = dm_u2f((ex & 255u) << 23), gy = dm_u2f(((ex >> 8) & 255u) << 23), gz = dm_u2f(((ex >> 16) & 255u) << 23);
			const float cx = q0.x - org.x, cy = q0.y - org.y, cz = q0.z - org.z;
			const uint32_t nxw = sx ? f2u(q1.w) : f2u(q1.x), fxw = sx ? f2u(q1.x) : f2u(q1.w);
			const uint32_t nyw = sy ? f2u(q2.x) : f2u(q1.y), fyw = sy ? f2u(q1.y) : f2u(q2.x);
			const uint32_t nzw = sz ? f2u(q2.y) : f2u(q1.z), fzw = sz ? f2u(q1.z) : f2u(q2.y);
			const uint32_t tags = f2u(q2.z), first = f2u(q2.w);
			auto entry = [&](int k, bool there, float &tn) -> bool {
				auto at_byte = [k](uint32_t word) { return (float)((word >> (8 * k)) & 255u); };
				const float tnx = dm_fmaf(at_byte(nxw), gx, cx) * inv.x, tfx = dm_fmaf(at_byte(fxw), gx, cx) * inv.x;
				const float tny = dm_fmaf(at_byte(nyw), gy, cy) * inv.y, tfy = dm_fmaf(at_byte(fyw), gy, cy) * inv.y;
				const float tnz = dm_fmaf(at_byte(nzw), gz, cz) * inv.z, tfz = dm_fmaf(at_byte(fzw), gz, cz) * inv.z;
				tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz), 0.0f);
				const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), tmax);
				return tn <= tf * 1.000001f && there;
			};
			// the first child the ray enters is next, the others wait in no particular order: one store each
			auto child = [&](int k, bool there) {
				float tn;
				if (entry(k, there, tn)) {
					const uint32_t ref = ((first + (uint32_t)k) << 5) | ((tags >> (8 * k)) & SRT_BVH_TAG_MASK);
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
	return occ;
}

} // namespace

#endif
