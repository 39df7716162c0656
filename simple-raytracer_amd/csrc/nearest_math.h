/* nearest_math.h -- the three distance functions of the nearest-surface queries (include/srt_abi.h "nearest-surface queries",
 * where every operation below is stated): the closest point of a sphere, a plane and a pre-pass triangle {v0, e1, e2} to a
 * point, its distance, and the BACK / feature bits. No HIP header: the kernels of nearest.hip, the host exports
 * srt_nearest_*_host and tests/csrc/nearest_math_check.cpp compile this one text, so the device, the host and the stand-alone
 * check run the same float32 operations in the same order.
 *
 * Everything is unfused float32 (-ffp-contract=off, as every file that includes detmath.h), IEEE division and dm_sqrtf.
 * nm_dot3 takes its terms in dm_dot3's order, x then y then z, left-associated, but rounds every product and every sum: a
 * numpy float32 restatement (tests/nearest_ref.py) is then exact, which it cannot be for a fused chain.
 */
#ifndef SRT_NEAREST_MATH_H
#define SRT_NEAREST_MATH_H

#include "detmath.h"

/* the flag bits the functions return: SRT_NEAREST_BACK (2) and the feature in bits 8..10 (include/srt_types.h) */
#define NM_BACK 2u
#define NM_FEATURE_SHIFT 8

typedef struct nm_result {
	float distance; /* NaN: never a candidate */
	float px, py, pz;
	uint32_t flags; /* NM_BACK | feature << NM_FEATURE_SHIFT */
} nm_result;

DM_FN float nm_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* c: the centre, radius as stored (its magnitude is the sphere's) */
DM_FN nm_result nm_sphere(float cx, float cy, float cz, float radius, float qx, float qy, float qz) {
	nm_result o;
	const float r = dm_fabs(radius);
	const float vx = qx - cx, vy = qy - cy, vz = qz - cz;
	const float len = dm_sqrtf(nm_dot3(vx, vy, vz, vx, vy, vz));
	o.distance = dm_fabs(len - r);
	if (len > 0.0f) {
		const float s = r / len;
		o.px = cx + vx * s, o.py = cy + vy * s, o.pz = cz + vz * s;
	} else {
		o.px = cx + r, o.py = cy + 0.0f, o.pz = cz + 0.0f;
	}
	o.flags = len < r ? NM_BACK : 0u;
	return o;
}

/* p, n as stored: n is not assumed to be of unit length */
DM_FN nm_result nm_plane(float px, float py, float pz, float nx, float ny, float nz, float qx, float qy, float qz) {
	nm_result o;
	const float nn = nm_dot3(nx, ny, nz, nx, ny, nz);
	const float k = nm_dot3(qx - px, qy - py, qz - pz, nx, ny, nz);
	o.distance = dm_fabs(k / dm_sqrtf(nn));
	const float s = k / nn;
	o.px = qx - nx * s, o.py = qy - ny * s, o.pz = qz - nz * s;
	o.flags = k < 0.0f ? NM_BACK : 0u;
	return o;
}

/* Ericson, Real-Time Collision Detection 5.1.5, over a = v0, ab = e1, ac = e2; the regions in the book's order */
DM_FN nm_result nm_triangle(float ax, float ay, float az, float abx, float aby, float abz, float acx, float acy, float acz, float qx, float qy,
                            float qz) {
	nm_result o;
	uint32_t feature;
	const float apx = qx - ax, apy = qy - ay, apz = qz - az;
	const float d1 = nm_dot3(abx, aby, abz, apx, apy, apz), d2 = nm_dot3(acx, acy, acz, apx, apy, apz);
	const float bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
	const float d3 = nm_dot3(abx, aby, abz, bpx, bpy, bpz), d4 = nm_dot3(acx, acy, acz, bpx, bpy, bpz);
	const float cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
	const float d5 = nm_dot3(abx, aby, abz, cpx, cpy, cpz), d6 = nm_dot3(acx, acy, acz, cpx, cpy, cpz);
	const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
	if (d1 <= 0.0f && d2 <= 0.0f) { /* vertex region A */
		o.px = ax, o.py = ay, o.pz = az;
		feature = 1u;
	} else if (d3 >= 0.0f && d4 <= d3) { /* B */
		o.px = ax + abx, o.py = ay + aby, o.pz = az + abz;
		feature = 2u;
	} else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { /* edge AB */
		const float v = d1 / (d1 - d3);
		o.px = ax + abx * v, o.py = ay + aby * v, o.pz = az + abz * v;
		feature = 4u;
	} else if (d6 >= 0.0f && d5 <= d6) { /* C */
		o.px = ax + acx, o.py = ay + acy, o.pz = az + acz;
		feature = 3u;
	} else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { /* edge AC */
		const float w = d2 / (d2 - d6);
		o.px = ax + acx * w, o.py = ay + acy * w, o.pz = az + acz * w;
		feature = 5u;
	} else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) { /* edge BC */
		const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
		o.px = (ax + abx) + (acx - abx) * w, o.py = (ay + aby) + (acy - aby) * w, o.pz = (az + abz) + (acz - abz) * w;
		feature = 6u;
	} else { /* the face */
		const float denom = 1.0f / ((va + vb) + vc);
		const float v = vb * denom, w = vc * denom;
		o.px = (ax + abx * v) + acx * w, o.py = (ay + aby * v) + acy * w, o.pz = (az + abz * v) + acz * w;
		feature = 0u;
	}
	const float dx = qx - o.px, dy = qy - o.py, dz = qz - o.pz;
	o.distance = dm_sqrtf(nm_dot3(dx, dy, dz, dx, dy, dz));
	const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx; /* cross(e1, e2) */
	o.flags = (nm_dot3(dx, dy, dz, nx, ny, nz) < 0.0f ? NM_BACK : 0u) | (feature << NM_FEATURE_SHIFT);
	return o;
}

#endif
