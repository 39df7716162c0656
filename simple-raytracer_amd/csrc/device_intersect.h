// device_intersect.h -- closest_intersection's parts: the scalar-load blocks, the sphere / plane / triangle tests (and the
// camera forms of the scene classes) and the BVH walk. Used by the trace and feature kernels (kernels.hip).
#ifndef SRT_DEVICE_INTERSECT_H
#define SRT_DEVICE_INTERSECT_H

#include "device_math.h"
#include "trace_regions.h" // moller_trumbore and walk_bvh carry SRT_REGION markers

namespace {

// ---- wave-uniform scene data: 64-byte blocks fetched with ONE scalar load each ----
// The persistent kernel stores to global memory (radiance) inside its main loop, after which
// the compiler can no longer prove that scene data is not clobbered and would fall back to
// per-lane VMEM loads of the same address. Reading through the CONSTANT address space states
// what is true here -- runs, packed records and world triangles are never written by this
// kernel -- and keeps these loads on the scalar unit (s_load_dwordx*, results in SGPRs).
#define SRT_AS_CONST __attribute__((address_space(4)))
struct Blk16 {
	float v[16];
};
struct Tri2 {
	float v[18];
};
template <int N, int ALIGN>
__device__ __forceinline__ void ld_uniform(const float *p, float (&out)[N]) {
	const SRT_AS_CONST float *c = (const SRT_AS_CONST float *)__builtin_assume_aligned(p, ALIGN);
#pragma unroll
	for (int i = 0; i < N; i++) out[i] = c[i];
}
__device__ __forceinline__ Blk16 ld_blk16(const float *p) {
	Blk16 b;
	ld_uniform<16, 64>(p, b.v);
	return b;
}
__device__ __forceinline__ Tri2 ld_tri2(const float *p) {
	Tri2 t;
	ld_uniform<18, 8>(p, t.v);
	return t;
}

__device__ __forceinline__ uint32_t f2u(float f) { return __float_as_uint(f); }

// render.cl:180-204 against FOUR spheres held in SGPRs (one 64-byte block {cx, cy, cz, r*r} x 4; the host fills a
// run's last block with spheres of r*r = -inf, whose discriminant is -inf or NaN: never a hit). Straight-line:
// the four tests are independent chains the scheduler can interleave, and the four square roots share ONE
// small-argument guard (sqrt_ieee above) instead of a branch each. Updates the lane's closest hit in array order.
// ---- closest-hit update with floats compared as unsigned integers --------------------------------------------------
// render.cl keeps a hit when `!(t < 0) && t < tmin` (after `disc < 0` / `denom == 0` have returned a miss). For floats that
// are not -0, "t >= 0 and t < tmin" is ONE unsigned compare of the bit patterns: non-negative floats (and +inf) order like
// their bits, every negative float and every NaN has bits above +inf's, and tmin is never negative (it only ever takes a t
// that passed this test; it starts at +inf). A miss reported through a NaN or an infinity needs no test of its own then:
// the root of a negative discriminant is NaN, n.(p - o) / 0 is +-inf or NaN. -0 is the one value the two orders disagree on
// (the reference accepts t = -0 and afterwards rejects every t >= +0 against tmin = -0): a wave that holds one -- as tmin, or
// as a plane's quotient; a sphere's bq -+ sq cannot be -0 when sq > 0 -- runs the reference's own sequence instead.
// Per sphere: sub, add, v_min_u32, compare, two selects (before: sub, add, compare, select, two compares, two selects and the
// wait states of one more compare -> select pair).
__device__ __forceinline__ bool is_neg_zero(float x) { return dm_f2u(x) == 0x80000000u; }
__device__ __forceinline__ void take_if_closer(float t_key, int idx, float &tmin, int &best) {
	if (dm_f2u(t_key) < dm_f2u(tmin)) {
		tmin = t_key;
		best = idx;
	}
}

// render.cl:180-204 against N of the FOUR spheres held in a 64-byte block {cx, cy, cz, r*r} x 4 (the host fills a run's last
// block with spheres of r*r = -inf, whose discriminant is -inf or NaN: never a hit; with N = 2 only the first two are
// looked at). Straight-line: the tests are independent chains the scheduler can interleave. Updates the lane's closest hit
// in array order.
template <int N>
__device__ __forceinline__ void test_spheres(const Blk16 &s, f3 org, f3 dir, int idx0, float &tmin, int &best) {
	float bq[4], disc[4];
	bool slow = is_neg_zero(tmin);
#pragma unroll
	for (int i = 0; i < N; i++) {
		f3 L = mk(s.v[4 * i] - org.x, s.v[4 * i + 1] - org.y, s.v[4 * i + 2] - org.z);
		bq[i] = dot3(L, dir);
		float c = dot3(L, L) - s.v[4 * i + 3];
		disc[i] = bq[i] * bq[i] - c;
		slow = slow || dm_fabs(disc[i]) < 0x1p-96f; // +-0 and 0 < |x| < 2^-96: one compare with |.| as a source modifier (a NaN is not "tiny")
	}
	if (__builtin_expect(any64(slow), 0)) { // (wave-uniform) the reference's sequence, IEEE square root
#pragma unroll
		for (int i = 0; i < N; i++) { // @rare
			const float sq = __builtin_sqrtf(disc[i]); // @rare
			float t = bq[i] - sq; // @rare
			if (t < 0.0f) t = bq[i] + sq; // @rare
			if (!(disc[i] < 0.0f) && !(t < 0.0f) && t < tmin) tmin = t, best = idx0 + i; // @rare
		}
	} else {
		// disc is NaN, negative, +inf or normal and >= 2^-96 here. sqrt_rsq is the IEEE root on the last range and NaN on the others;
		// IEEE sqrt is NaN on the first two and +inf for +inf -- and a discriminant of +inf never updates the hit either way: with
		// sq = +inf, bq -+ inf is -inf then +inf (or NaN), and +inf < tmin is false; with sq = NaN every t is NaN.
		float dd[N], sq[N];
#pragma unroll
		for (int i = 0; i < N; i++) dd[i] = disc[i];
		sqrt_rsq_n<N, false>(dd, sq);
#pragma unroll
		for (int i = 0; i < N; i++) {
			// the smaller root if it is not negative, else the larger: the smaller of the two bit patterns (bq - sq <= bq + sq)
			const uint32_t k = min(dm_f2u(bq[i] - sq[i]), dm_f2u(bq[i] + sq[i]));
			take_if_closer(dm_u2f(k), idx0 + i, tmin, best);
		}
	}
}

// render.cl:206-221 against TWO planes (one 64-byte block {p, 0, n, 0} x 2; a run's last block is filled with a
// plane of normal 0: denom == 0, never a hit). (The unsigned-key update of take_if_closer does not pay here: a plane's
// quotient can be -0, and testing for it costs what the key saves.)
__device__ __forceinline__ void test_planes2(const Blk16 &b, uint32_t count, f3 org, f3 dir, int idx0, float &tmin, int &best) {
#pragma unroll
	for (int i = 0; i < 2; i++) {
		if (i == 1 && count < 2u) break; // (wave-uniform) a run's last block may hold one plane: the filler's test, division included, is skipped
		f3 n = mk(b.v[8 * i + 4], b.v[8 * i + 5], b.v[8 * i + 6]);
		float denom = dot3(n, dir);
		float t = dot3(n, mk(b.v[8 * i] - org.x, b.v[8 * i + 1] - org.y, b.v[8 * i + 2] - org.z)) / denom;
		// render.cl:209 `denom == 0 -> miss` needs no test of its own: x / 0 is +-inf or NaN, and +inf or a NaN is never below
		// tmin, -inf is below 0
		bool hit = !(t < 0.0f);
		if (hit && t < tmin) {
			tmin = t;
			best = idx0 + i;
		}
	}
}

// ---- CAMERA PHASES of the scene classes (trace_body.inc EXTEND) ------------------------------------------------
// Every camera ray of a launch starts at camera_to_world[3], so what the two tests above make from a shape and the origin
// alone is the same number for all of them: a sphere's L = centre - org and c = dot3(L, L) - r*r, a plane's
// num = dot3(n, p - org). A class kernel makes them once per wave in its prologue (cam_records_of_block: the expressions of
// test_spheres / test_planes2, on the device, so the bits are theirs) and keeps them in LDS: a sphere's {L, c} as a record of
// its own behind the hit queue, a plane's num in the unused fourth dword of its point in the staged block. An EXTEND phase in
// which every ray is a fresh camera ray (one wave-uniform flag, set by REFILL) runs the forms below, which start from those
// numbers and are otherwise the sequences above. The 64 rays of such a phase are (nearly) one pixel's, so they mostly agree on
// which spheres they cannot hit, and one vote per sphere takes out work that would change no lane's tmin / best: a sphere whose
// discriminant is negative or NaN on every lane that holds a ray has a NaN root there, both keys are above +inf's bits, and
// take_if_closer takes nothing. (+inf votes "may hit" and is rooted as before; tiny and zero discriminants have gone to the
// slow path before the vote.) The same vote for a plane -- skip the division where every lane's quotient is certainly negative
// and not -0 -- was built and measured nothing beyond the hoisting (profiles/r13_camera_phase_ab.txt, `hoist_pln`): not kept.
// cam: the block's records {L, c}; actm: the lanes that hold a ray (the others compute on whatever they hold and must not vote)
template <int N>
__device__ __forceinline__ void test_spheres_cam(const float4 *__restrict__ cam, f3 dir, unsigned long long actm, int idx0, float &tmin, int &best) {
	float bq[4], disc[4];
	bool slow = is_neg_zero(tmin);
#pragma unroll
	for (int i = 0; i < N; i++) {
		const float4 lc = cam[i];
		bq[i] = dot3(mk(lc.x, lc.y, lc.z), dir);
		disc[i] = bq[i] * bq[i] - lc.w;
		slow = slow || dm_fabs(disc[i]) < 0x1p-96f;
	}
	if (__builtin_expect(any64(slow), 0)) { // (wave-uniform) the reference's sequence, as in test_spheres
#pragma unroll
		for (int i = 0; i < N; i++) { // @rare
			const float sq = __builtin_sqrtf(disc[i]); // @rare
			float t = bq[i] - sq; // @rare
			if (t < 0.0f) t = bq[i] + sq; // @rare
			if (!(disc[i] < 0.0f) && !(t < 0.0f) && t < tmin) tmin = t, best = idx0 + i; // @rare
		}
	} else {
#pragma unroll
		for (int i = 0; i < N; i++) {
			if ((ballot64(disc[i] >= 0.0f) & actm) != 0ull) { // (wave-uniform) somebody's ray may hit sphere i
				const float sq = sqrt_rsq(disc[i]);
				const uint32_t k = min(dm_f2u(bq[i] - sq), dm_f2u(bq[i] + sq));
				take_if_closer(dm_u2f(k), idx0 + i, tmin, best);
			}
		}
	}
}
// blk: the staged block {p, num, n, 0} x 2
__device__ __forceinline__ void test_planes2_cam(const float4 *__restrict__ blk, uint32_t count, f3 dir, int idx0, float &tmin, int &best) {
#pragma unroll
	for (int i = 0; i < 2; i++) {
		if (i == 1 && count < 2u) break;
		const float4 nq = blk[2 * i + 1];
		const float num = reinterpret_cast<const float *>(blk + 2 * i)[3];
		const float denom = dot3(mk(nq.x, nq.y, nq.z), dir);
		const float t = num / denom;
		const bool hit = !(t < 0.0f);
		if (hit && t < tmin) {
			tmin = t;
			best = idx0 + i;
		}
	}
}
// The prologue's part: block K of the class, staged at blk, seen from the camera's origin. Lane i makes shape i's numbers.
template <uint32_t K>
__device__ __forceinline__ void cam_records_of_block(float4 *__restrict__ blk, float4 *__restrict__ cam, f3 org, int lane) {
	if constexpr ((K & 3u) == SRT_SHAPE_SPHERE + 1u) {
		if (lane < 4) {
			const float4 s = blk[lane];
			const f3 L = mk(s.x - org.x, s.y - org.y, s.z - org.z);
			const float c = dot3(L, L) - s.w;
			cam[lane] = make_float4(L.x, L.y, L.z, c);
		}
	} else if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		if (lane < 2) {
			const float4 pq = blk[2 * lane], nq = blk[2 * lane + 1];
			reinterpret_cast<float *>(blk + 2 * lane)[3] = dot3(mk(nq.x, nq.y, nq.z), mk(pq.x - org.x, pq.y - org.y, pq.z - org.z));
		}
	}
}
// ---- AXIS PLANES of a scene class's axis twin (device_types.h SRT_SCENE_AXIS_LIST; DESIGN.md 5 "Axis planes") ------------------------
// A plane whose normal is s e_k (s = +-1, the other two components +-0) and whose position is tame (scene_prep.cpp
// srt_plane_axis_code). With dm_dot3 = fma(az, bz, fma(ay, by, ax * bx)), a product with a zero component is a zero whenever the
// other factor is finite, and adding a zero to a number that is not one returns that number, so
//   dot3(n, dir) = s dir[k]              when the other two components of dir are finite and dir[k] != 0,
//   dot3(n, p - org) = s (p[k] - org[k]) when the other two differences are finite and p[k] - org[k] != 0,
// and (s a) / (s b) = a / b bit for bit: t = (p[k] - org[k]) / dir[k]. Where a side is +-0 the two forms may differ in the zero's
// sign (which reaches org + dir * tmin through t = +-0, a hit), and where an unused component is not finite the reference has a NaN
// the folded form does not. ONE test per EXTEND phase (axis_operands_ok, voted over the lanes that hold a ray) excludes all of it
// and puts the quotients inside div_core's box, where rcp_refined + div_core IS the division (device_math.h; srt_selftest_math
// out[8], out[9]):
//   the planes' numerators a = p[k] - org[k]:  2^-60 <= |a|, sum |a| <= 2^50   (not zero, finite; a NaN fails the sum's compare)
//   the direction's three components b:        2^-40 <= |b|, sum |b| <= 2^40
// The numerators between them hold every component of org (srt_axes_buildable: the planes use all three axes), and a plane's
// position is at most 2^100 in every component (the host's predicate), so every p[j] - org[j] of the reference is finite too. A
// wave with a lane outside runs today's test_planes2 / test_planes2_cam for that phase. min3 skips a NaN; the sums do not.
#ifndef SRT_AXIS_SHORT_DIV
#define SRT_AXIS_SHORT_DIV 1 // (0: the compiler's division behind the same guard -- the "folding alone" build of profiles/r21_axis_planes_ab.txt)
#endif
template <int C>
__device__ __forceinline__ float f3_at(f3 v) { return C == 0 ? v.x : C == 1 ? v.y : v.z; }
// the numerators of block K's planes (blk: its 16 floats) as seen from org, a[i] for slot i
template <uint32_t K, uint32_t AX>
__device__ __forceinline__ void axis_numerators(const float *__restrict__ blk, f3 org, float *__restrict__ a) {
	if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		constexpr int C0 = (int)(AX & 3u) - 1, C1 = (int)((AX >> 2) & 3u) - 1;
		a[0] = blk[C0 < 0 ? 0 : C0] - f3_at<C0>(org);
		if constexpr (((K >> 2) & 7u) > 1u) a[1] = blk[8 + (C1 < 0 ? 0 : C1)] - f3_at<C1>(org);
	}
}
template <int N>
__device__ __forceinline__ bool axis_operands_ok(const float *__restrict__ a, f3 dir) {
	float mn = dm_fabs(a[0]), sm = dm_fabs(a[0]);
#pragma unroll
	for (int i = 1; i < N; i++) mn = __builtin_fminf(mn, dm_fabs(a[i])), sm = sm + dm_fabs(a[i]);
	const float bx = dm_fabs(dir.x), by = dm_fabs(dir.y), bz = dm_fabs(dir.z);
	const float mnb = __builtin_fminf(__builtin_fminf(bx, by), bz), smb = (bx + by) + bz;
	return mn >= 0x1p-60f && sm <= 0x1p50f && mnb >= 0x1p-40f && smb <= 0x1p40f;
}
// a / b for operands that passed axis_operands_ok
__device__ __forceinline__ float axis_div(float a, float b) {
#if SRT_AXIS_SHORT_DIV
	return div_core(a, b, rcp_refined(b));
#else
	return a / b;
#endif
}
// test_planes2 / test_planes2_cam for a wave that passed: a[i] = slot i's numerator (axis_numerators; in a camera phase the
// prologue's, from the staged block)
template <uint32_t AX>
__device__ __forceinline__ void test_planes2_axis(const float *__restrict__ a, uint32_t count, f3 dir, int idx0, float &tmin, int &best) {
#pragma unroll
	for (int i = 0; i < 2; i++) {
		if (i == 1 && count < 2u) break;
		const float b = i == 0 ? f3_at<(int)(AX & 3u) - 1>(dir) : f3_at<(int)((AX >> 2) & 3u) - 1>(dir);
		const float t = axis_div(a[i], b);
		const bool hit = !(t < 0.0f);
		if (hit && t < tmin) {
			tmin = t;
			best = idx0 + i;
		}
	}
}
// The prologue's part for the camera phases: the folded numerator of block K's planes seen from the camera's origin, in the
// unused fourth dword of the plane's normal in the staged block (num itself stays where the reference form reads it).
template <uint32_t K, uint32_t AX>
__device__ __forceinline__ void cam_axis_numerators(float4 *__restrict__ blk, f3 org, int lane) {
	if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		if (lane < 2) {
			const float4 pq = blk[2 * lane];
			const int c = (int)((AX >> (2 * lane)) & 3u) - 1;
			const float pk = c == 0 ? pq.x : c == 1 ? pq.y : pq.z, ok = c == 0 ? org.x : c == 1 ? org.y : org.z;
			reinterpret_cast<float *>(blk + 2 * lane + 1)[3] = pk - ok;
		}
	}
}
// render.cl:279-290 with tmax = the lane's current closest t
__device__ __forceinline__ bool test_aabb(float lx, float ly, float lz, float hx, float hy, float hz, f3 org, f3 inv, float tmax) {
	float t0 = 0.0f, t1 = tmax;
	float a1 = (lx - org.x) * inv.x, a2 = (hx - org.x) * inv.x;
	t0 = dm_max(t0, dm_min(a1, a2));
	t1 = dm_min(t1, dm_max(a1, a2));
	a1 = (ly - org.y) * inv.y, a2 = (hy - org.y) * inv.y;
	t0 = dm_max(t0, dm_min(a1, a2));
	t1 = dm_min(t1, dm_max(a1, a2));
	a1 = (lz - org.z) * inv.z, a2 = (hz - org.z) * inv.z;
	t0 = dm_max(t0, dm_min(a1, a2));
	t1 = dm_min(t1, dm_max(a1, a2));
	return t0 < t1;
}

// One Moller-Trumbore test (render.cl:243-275) against a pre-pass triangle in SGPRs.
//
// The reference rejects at `u < 0 || u > 1` with u = fl(fl(1/a) * sh); that needs an IEEE
// reciprocal (11 instructions) before the first reject. For brute force over 10^5
// triangles almost every lane of almost every wave fails that test, so a conservative,
// division-free pre-reject runs first. With sh = dot(s, h):
//   R1  a == 0                                            (the reference's own test)
//   R2  |sh| > 1.001 |a|              =>  |u| > 1         (u > 1 or u < 0: miss either way)
//   R3  sh*a < 0 and |sh| >= 0.001 |a| =>  u < 0, not an underflow to -0
// Each implies the reference's miss for every finite, infinite or denormal a (margins of
// 2^-10 dwarf the 2^-22 worst-case relative error of fl(1/a)*sh; NaNs compare false and
// fall through). Lanes not rejected compute the reference's q and dot(dir, q) and meet two
// more such rejects, on v (R4, R5 below); what is left runs the reference's exact sequence.
// The wave skips each stage when no lane is left (s_cbranch_execz). Results are therefore
// bit-identical.
// Returns true when the reference accepts the triangle; t is then its hit distance.
template <bool COUNT_TRIS>
__device__ __forceinline__ bool moller_trumbore(float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y,
                                                float e2z, f3 org, f3 dir, bool counted, float &t, uint32_t &n_tri_u SRT_RC_PARAM) {
	f3 e1 = mk(e1x, e1y, e1z), e2 = mk(e2x, e2y, e2z);
	f3 h = cross3(dir, e2);
	float a = dot3(e1, h);
	f3 sv = mk(org.x - v0x, org.y - v0y, org.z - v0z);
	float sh = dot3(sv, h);
	float aa = dm_fabs(a), ash = dm_fabs(sh);
	bool reject = (a == 0.0f) || (ash > aa * 1.001f) || ((sh * a < 0.0f) && (ash >= aa * 0.001f));
	bool ok = false;
	if (!reject) {
		SRT_REGION(EXTEND_TRI_EXACT);
		// The reference's q and dot(dir, q) first, and two more division-free rejects on v = f * dv before the IEEE reciprocal
		// (11 instructions that a wave pays as soon as ONE lane is left):
		//   R4  dv*a < 0 and |dv| >= 0.001 |a|  =>  v < 0, not an underflow to -0        (as R3 for u)
		//   R5  |sh + dv| > 1.01 |a|             =>  |u + v| > 1: u + v > 1, or one of u, v is below -0.5
		// (u + v as the reference rounds it differs from (sh + dv) / a by parts in 10^6; NaNs compare false and fall through).
		// Meshes whose triangles are large on screen send a third of all wave-tests past R1-R3 with a handful of lanes each;
		// most of those lanes fail on v. The instrumented variant counts the lanes that pass the u test and keeps them all.
		// (Measured and left out: the same for t -- dt*a < 0 => t not > 0, |dt| > 1.001 tmin |a| => not closer -- costs the
		// wave-tests that get here more than the reciprocals it saves: configs[2] 107.2 -> 108.6 ms, configs[4] 4,297 -> 4,340.)
		f3 q = cross3(sv, e1);
		float dv = dot3(dir, q);
		bool reject2 = false;
		if (!COUNT_TRIS) reject2 = ((dv * a < 0.0f) && (dm_fabs(dv) >= aa * 0.001f)) || (dm_fabs(sh + dv) > aa * 1.01f);
		if (!reject2) {
			SRT_REGION(EXTEND_TRI_DIV);
			float f = 1.0f / a;
			float u = f * sh;
			ok = !(u < 0.0f || u > 1.0f);
			if (COUNT_TRIS) n_tri_u += (ok && counted) ? 1u : 0u; // padding triangles (NaN rays reach here) are not tests
			float v = f * dv;
			ok = ok && !(v < 0.0f || u + v > 1.0f);
			t = f * dot3(e2, q);
			ok = ok && t > 0.0f;
		}
	}
	return ok;
}

template <bool COUNT_TRIS>
__device__ __forceinline__ void test_triangle(float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y,
                                              float e2z, f3 org, f3 dir, int idx, uint32_t j, uint32_t count, float &tmin, int &best,
                                              uint32_t &best_tri, uint32_t &n_tri_u SRT_RC_PARAM) {
	float t = 0.0f;
	if (moller_trumbore<COUNT_TRIS>(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, org, dir, j < count, t, n_tri_u SRT_RC_ARG) && t < tmin) {
		tmin = t;
		best = idx;
		best_tri = j;
	}
}

// Each model's block of world triangles starts on a multiple of 4 and is padded to a
// multiple of 4 with all-zero triangles (which fail R1), so the loop below needs no tail
// handling. Triangles are fetched two at a time (18 dwords: s_load_dwordx16 + x2) into
// TWO alternating SGPR sets: the load of the next pair is issued before the current
// pair is tested, which hides the scalar-cache / L2 latency that a single buffer would
// expose once per block (the loop is otherwise latency-bound at low occupancy).

template <bool COUNT_TRIS>
__device__ __forceinline__ void test_pair(const Tri2 &t, f3 org, f3 dir, int idx, uint32_t j, uint32_t count, float &tmin, int &best,
                                          uint32_t &best_tri, uint32_t &n_tri_u SRT_RC_PARAM) {
	test_triangle<COUNT_TRIS>(t.v[0], t.v[1], t.v[2], t.v[3], t.v[4], t.v[5], t.v[6], t.v[7], t.v[8], org, dir, idx, j, count, tmin, best, best_tri,
	                          n_tri_u SRT_RC_ARG);
	test_triangle<COUNT_TRIS>(t.v[9], t.v[10], t.v[11], t.v[12], t.v[13], t.v[14], t.v[15], t.v[16], t.v[17], org, dir, idx, j + 1u, count, tmin,
	                          best, best_tri, n_tri_u SRT_RC_ARG);
}

template <bool COUNT_TRIS>
__device__ __forceinline__ void test_triangles(const float *__restrict__ wtris, uint32_t first, uint32_t count, f3 org, f3 dir, int idx,
                                               float &tmin, int &best, uint32_t &best_tri, uint32_t &n_tri_u SRT_RC_PARAM) {
	const float *__restrict__ blk = wtris + (size_t)first * SRT_WTRI_FLOATS;
	const uint32_t npair = ((count + 3u) >> 2) << 1; // pairs, always even
	Tri2 a = ld_tri2(blk);
	for (uint32_t b = 0; b < npair; b += 2) {
		SRT_REGION(EXTEND_TRI_LOOP);
		const Tri2 c = ld_tri2(blk + 18u * (b + 1u)); // in flight while `a` is tested
		test_pair<COUNT_TRIS>(a, org, dir, idx, 2u * b, count, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
		a = ld_tri2(blk + 18u * (b + 2u)); // in flight while `c` is tested (one pair of slack is allocated past the end)
		test_pair<COUNT_TRIS>(c, org, dir, idx, 2u * b + 2u, count, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
	}
}

// ---- BVH walk (opt-in; device_types.h "wide hierarchy") ------------------------------------
// Per lane: rays of a wave are incoherent after the first bounce, so blocks come through per-lane
// loads. What binds the walk is the CU's vector memory pipe -- ONE address unit for its 20 waves, busy
// two thirds of a launch; a divergent load costs it ~7 ns plus ~0.3 ns per lane that executes it, whatever
// its width (profiles/r04_bvh_vmem_probe.md, scripts/microbench/ta_rates.hip) -- so a step is built around as
// few lane-loads as the data allows: an inner block holds the boxes of FOUR children as bytes on a grid of its
// own (48 bytes: three quarters; a ray takes about a quarter of the steps of a binary walk), a leaf block up to
// three triangles (27 dwords: seven quarters, four of them fetched only by the lanes that stand on a leaf).
// Children are visited nearest first by their entry distance; the others wait, with that distance, on a
// per-lane stack in scratch memory whose top entry lives in registers.
// Same Moller-Trumbore as the array scan, so every accepted hit has the same t; what the walk must
// guarantee is that the triangle the array-order scan would settle on is visited and wins:
//  * boxes were padded on the host and the slab test errs towards "hit" (safe inverse for zero
//    direction components, relative slack on the exit distance and on the stacked entry distance);
//  * the scan keeps the FIRST triangle of equal t (strict <, render.cl:254-256): a hit with
//    t == tmin inside the same model replaces the incumbent only if its index j is lower.
struct BvhStackEntry {
	uint32_t key;   // entry distance | tag (device_types.h)
	uint32_t first; // block of the parent's child 0: the entry is block first + (key & 3)
};

// one plane quarter of a block: the hierarchy's base stays in SGPRs, the lane supplies a 32-bit byte offset
__device__ __forceinline__ float4 bvh_quarter(const float4 *__restrict__ blocks, uint32_t byte_offset, uint32_t imm) {
	return *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(blocks) + (size_t)byte_offset + imm);
}

// index inside its model of the triangle in record rec = (leaf block << 2) | slot
__device__ __forceinline__ uint32_t bvh_tri_in_model(const float4 *__restrict__ blocks, uint32_t rec) {
	return reinterpret_cast<const uint32_t *>(blocks)[(size_t)(rec >> 2) * 32u + SRT_BVH_LEAF_J + (rec & 3u)];
}

__device__ __forceinline__ void bvh_order2(uint32_t &a, uint32_t &b) {
	const uint32_t lo = a < b ? a : b, hi = a < b ? b : a; // v_min_u32 / v_max_u32
	a = lo, b = hi;
}

template <bool COUNT_TRIS>
__device__ __forceinline__ void walk_bvh(const float4 *__restrict__ blocks, BvhStackEntry *__restrict__ stack, uint32_t root, f3 org, f3 dir, int idx,
                                         float &tmin, int &best, uint32_t &best_rec, uint32_t &n_tri, uint32_t &n_tri_u SRT_RC_PARAM) {
	// 1/d, or +-2^100 where |d| < 2^-100: (lo - o) * inv stays finite (no 0 * inf = NaN), and keeps its sign
	f3 inv;
	inv.x = dm_fabs(dir.x) >= 0x1p-100f ? 1.0f / dir.x : __builtin_copysignf(0x1p100f, dir.x);
	inv.y = dm_fabs(dir.y) >= 0x1p-100f ? 1.0f / dir.y : __builtin_copysignf(0x1p100f, dir.y);
	inv.z = dm_fabs(dir.z) >= 0x1p-100f ? 1.0f / dir.z : __builtin_copysignf(0x1p100f, dir.z);
	// which planes of a box the ray meets first: lo for a positive direction, hi for a negative one
	const bool sx = inv.x < 0.0f, sy = inv.y < 0.0f, sz = inv.z < 0.0f;
	uint32_t cur = root == SRT_BVH_NONE ? SRT_BVH_NONE : (root & SRT_BVH_INDEX_MASK);
	uint32_t cur_key = SRT_BVH_TAG(root, 0u);
	// The youngest waiting entry lives in registers, stack[0 .. sp) holds the older ones. Under them all lies a sentinel that
	// always passes the distance test and leads to block NONE: popping it ends the walk, so no pop asks whether the stack is empty.
	uint32_t top_key = 0u, top_first = SRT_BVH_NONE;
	uint32_t sp = 0u;
	stack[0].key = 0u, stack[0].first = SRT_BVH_NONE; // (what a pop of the sentinel itself reads back into the registers)
	while (cur != SRT_BVH_NONE) {
		SRT_REGION(EXTEND_BVH_STEP);
		bool pending = true; // nothing to enter from here: take the youngest waiting child
		uint32_t next = SRT_BVH_NONE, next_key = 0u;
		bool inner = false;
		uint32_t k0 = SRT_BVH_KEY_INF, k1 = SRT_BVH_KEY_INF, k2 = SRT_BVH_KEY_INF, k3 = SRT_BVH_KEY_INF, first = 0u;
		{
		// An inner block is 48 bytes: every lane fetches three quarters, the lanes that stand on a leaf the other four (what a
		// load costs the CU's address unit it costs per lane that executes it: scripts/microbench/ta_rates.hip).
		const bool leaf = (cur_key & SRT_BVH_TAG_LEAF) != 0u;
		const uint32_t at = cur << 7;
		const float4 q0 = bvh_quarter(blocks, at, 0u), q1 = bvh_quarter(blocks, at, 16u), q2 = bvh_quarter(blocks, at, 32u);
		if (leaf) {
			const uint32_t cnt = (cur_key >> 2) & 3u, rec0 = cur << 2;
			const float4 q3 = bvh_quarter(blocks, at, 48u), q4 = bvh_quarter(blocks, at, 64u);
#if SRT_BVH_LEAF_MAX > 2
			const float4 q5 = bvh_quarter(blocks, at, 80u), q6 = bvh_quarter(blocks, at, 96u); // (only for the one leaf in four that holds a third triangle: 30.6 against 30.3 ms)
#else
			const float4 q5 = q3, q6 = q3;
#endif
			if (COUNT_TRIS) n_tri += cnt;
			auto tri = [&](float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, uint32_t k) {
				float t = 0.0f;
				if (moller_trumbore<COUNT_TRIS>(v0x, v0y, v0z, e1x, e1y, e1z, e2x, e2y, e2z, org, dir, true, t, n_tri_u SRT_RC_ARG)) {
					bool wins = t < tmin;
					if (t == tmin && best == idx) // the reference keeps the FIRST triangle of equal t: the indices inside the model decide (fetched only here)
						wins = bvh_tri_in_model(blocks, rec0 + k) < bvh_tri_in_model(blocks, best_rec);
					if (wins) {
						tmin = t;
						best = idx;
						best_rec = rec0 + k;
					}
				}
			};
			tri(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, 0u);
			if (cnt > 1u) tri(q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, 1u);
			if (cnt > 2u) tri(q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, q6.x, q6.y, q6.z, 2u);
		} else {
			// four children, their boxes as bytes on a power-of-two grid relative to the block's origin: bound - o = fmaf(byte, 2^e,
			// origin - o) (the host rounded the bytes outwards and checked them in fmaf(byte, 2^e, origin)); no product can be
			// 0 * inf here: byte * 2^e is finite or, for the all-embracing boxes of hostile input, +inf
			const uint32_t ex = f2u(q0.w), nk = ex >> 24;
			const float gx = dm_u2f((ex & 255u) << 23), gy = dm_u2f(((ex >> 8) & 255u) << 23), gz = dm_u2f(((ex >> 16) & 255u) << 23);
			const float cx = q0.x - org.x, cy = q0.y - org.y, cz = q0.z - org.z;
			// the planes the ray meets first / last on each axis: lo / hi for a positive direction, hi / lo for a negative one
			const uint32_t nxw = sx ? f2u(q1.w) : f2u(q1.x), fxw = sx ? f2u(q1.x) : f2u(q1.w);
			const uint32_t nyw = sy ? f2u(q2.x) : f2u(q1.y), fyw = sy ? f2u(q1.y) : f2u(q2.x);
			const uint32_t nzw = sz ? f2u(q2.y) : f2u(q1.z), fzw = sz ? f2u(q1.z) : f2u(q2.y);
			const uint32_t tags = f2u(q2.z);
			first = f2u(q2.w);
			auto child = [&](int k, bool there) -> uint32_t {
				auto at_byte = [k](uint32_t word) { return (float)((word >> (8 * k)) & 255u); };
				const float tnx = dm_fmaf(at_byte(nxw), gx, cx) * inv.x, tfx = dm_fmaf(at_byte(fxw), gx, cx) * inv.x;
				const float tny = dm_fmaf(at_byte(nyw), gy, cy) * inv.y, tfy = dm_fmaf(at_byte(fyw), gy, cy) * inv.y;
				const float tnz = dm_fmaf(at_byte(nzw), gz, cz) * inv.z, tfz = dm_fmaf(at_byte(fzw), gz, cz) * inv.z;
				const float tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz), 0.0f);
				const float tf = __builtin_fminf(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), tmin);
				const bool hit = tn <= tf * 1.000001f && there;
				return ((hit ? f2u(tn) : SRT_BVH_KEY_INF) & ~SRT_BVH_TAG_MASK) | ((tags >> (8 * k)) & 255u);
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
			// k0 is entered now. The n others wait, farthest deepest: the registers' entry goes to memory and k1 takes its place,
			// k3 and k2 go between them. (Three unconditional stores, the idle ones into a spare slot, measured 37.7 / 37.8 ms
			// against 34.7 / 33.9 on the float-box walk.)
			const uint32_t w1 = k1 < SRT_BVH_KEY_INF ? 1u : 0u, w2 = k2 < SRT_BVH_KEY_INF ? 1u : 0u, w3 = k3 < SRT_BVH_KEY_INF ? 1u : 0u;
			const uint32_t n = w1 + w2 + w3;
			if (w1) {
				SRT_REGION(EXTEND_BVH_SPILL);
				stack[sp].key = top_key, stack[sp].first = top_first;
			}
			if (w3) {
				SRT_REGION(EXTEND_BVH_PUSH3);
				stack[sp + 1u].key = k3, stack[sp + 1u].first = first;
			}
			if (w2) {
				SRT_REGION(EXTEND_BVH_PUSH2);
				stack[sp + n - 1u].key = k2, stack[sp + n - 1u].first = first;
			}
			top_key = w1 ? k1 : top_key, top_first = w1 ? first : top_first;
			sp += n;
			if (k0 < SRT_BVH_KEY_INF) next = first + (k0 & 3u), next_key = k0, pending = false;
		}
		// the youngest waiting child that the closest hit so far has not put out of reach (its distance was rounded down: compare
		// against the limit's bits with the tag bits set)
		const uint32_t reach = f2u(tmin * 1.000001f) | SRT_BVH_TAG_MASK;
		while (pending) {
			SRT_REGION(EXTEND_BVH_POP);
			if (top_key <= reach) next = top_first + (top_key & 3u), next_key = top_key, pending = false;
			sp = sp > 0u ? sp - 1u : 0u;
			top_key = stack[sp].key, top_first = stack[sp].first;
		}
		cur = next, cur_key = next_key;
	}
}

} // namespace

#endif
