// device_math.h -- the device helpers every kernel unit shares (kernels.hip, frame.hip, selftest.hip): wave votes, f3, the
// exact square roots and divisions, the RNG and the bounce's specialised detmath routines. All __forceinline__ in an anonymous
// namespace: where a kernel's helpers live does not reach its code.
#ifndef SRT_DEVICE_MATH_H
#define SRT_DEVICE_MATH_H

#include <hip/hip_runtime.h>

#include "detmath.h"
#include "device_types.h"

namespace {

// The lanes of the wave for which p holds, straight from the compare's SGPR pair. HIP's __ballot / __any take an int: the
// bool is first materialised per lane (v_cndmask 0 / 1) and compared again (v_cmp_ne) -- two VALU instructions for each of the
// ~10 votes of a loop iteration.
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool any64(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }

struct f3 {
	float x, y, z;
};

__device__ __forceinline__ f3 mk(float x, float y, float z) { return f3{x, y, z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ f3 operator/(f3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ f3 neg(f3 a) { return mk(-a.x, -a.y, -a.z); }
// neither an infinity nor a NaN: the exponent's bits are not all ones
__device__ __forceinline__ bool finite_bits(float x) { return (dm_f2u(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite3(f3 a) { return finite_bits(a.x) && finite_bits(a.y) && finite_bits(a.z); }
// the OpenCL built-ins dot and cross as detmath.h pins them (FMA forms: 3 and 6 instructions)
__device__ __forceinline__ float dot3(f3 a, f3 b) { return dm_dot3(a.x, a.y, a.z, b.x, b.y, b.z); }
__device__ __forceinline__ f3 cross3(f3 a, f3 b) {
	return mk(dm_cross1(a.y, b.z, a.z, b.y), dm_cross1(a.z, b.x, a.x, b.z), dm_cross1(a.x, b.y, a.y, b.x));
}
// Correctly rounded sqrt. hipcc's own expansion (v_sqrt_f32 + two FMA residual tests
// against the neighbouring floats) spends 7 more instructions on 2^32 pre/post scaling
// for inputs below 2^-96 and on a zero/inf class fix-up. For x = 0, x >= 2^-96, inf, NaN
// and x <= -2^-96 the unscaled core already returns the IEEE result (see DESIGN.md
// "Numerics"), so only 0 < |x| < 2^-96 takes the compiler's full sequence (v_sqrt_f32
// flushes denormal inputs: sqrt(-denormal) must be NaN, not -0). Verified against
// __builtin_sqrtf on all 2^32 bit patterns by srt_selftest_math.
__device__ __forceinline__ float sqrt_ieee(float x) {
	const uint32_t mag = dm_f2u(x) & 0x7fffffffu;
	if (__builtin_expect((mag - 1u) < 0x0f7fffffu, 0)) return __builtin_sqrtf(x); // 0 < |x| < 2^-96 @rare
	float s = __builtin_amdgcn_sqrtf(x); // within 1 ulp
	const uint32_t si = dm_f2u(s);
	float down = dm_u2f(si - 1u), up = dm_u2f(si + 1u);
	float vp = __builtin_fmaf(-down, s, x);
	float vs = __builtin_fmaf(-up, s, x);
	s = (vp <= 0.0f) ? down : s;
	s = (vs > 0.0f) ? up : s;
	return s;
}
// sqrt_ieee without its slow-path guard, for arguments known to be 0, inf, NaN or of
// magnitude >= 2^-96.
__device__ __forceinline__ float sqrt_core(float x) {
	float s = __builtin_amdgcn_sqrtf(x);
	const uint32_t si = dm_f2u(s);
	float down = dm_u2f(si - 1u), up = dm_u2f(si + 1u);
	float vp = __builtin_fmaf(-down, s, x);
	float vs = __builtin_fmaf(-up, s, x);
	s = (vp <= 0.0f) ? down : s;
	s = (vs > 0.0f) ? up : s;
	return s;
}

// Correctly rounded sqrt of a NORMAL x >= 2^-96 from v_rsq_f32 and one residual step: y ~ 1/sqrt(x) (1 ulp), s = x y (within
// 2 ulp of the root), then s + (x - s s) (y / 2) rounded once (Markstein's form of the Newton step: the residual comes out of
// one fma, and the correction is far below the distance of any root of a float from a rounding boundary). One transcendental
// and four plain instructions, no compare / select pair (each of which costs wait states on gfx950, where a VALU may not read
// an SGPR or VCC a VALU wrote in the two slots before): sqrt_core above is 1 + 8 and two such pairs.
// EXHAUSTIVE: equal to __builtin_sqrtf on every float in [2^-96, inf) (scripts/microbench/exact_math_probe.hip;
// srt_selftest_math out[12] repeats the sweep inside the library). Outside that range: NaN for negative x and NaN (as IEEE),
// NaN for +inf (IEEE: inf), NaN for +-0 (IEEE: +-0), garbage for tiny x -- callers route those elsewhere or show that NaN and
// the IEEE value act alike where the result goes.
__device__ __forceinline__ float sqrt_rsq(float x) {
	const float y = __builtin_amdgcn_rsqf(x);
	const float s = x * y, h = 0.5f * y;
	const float r = __builtin_fmaf(-s, s, x);
	return __builtin_fmaf(r, h, s);
}
// The same with the reciprocal root clamped to [0, 2^100] (v_med3_f32; a NaN becomes 0): additionally +-0 -> +-0. For
// arguments that are -0, +0 or normal and >= 2^-96: Box-Muller's -2 log u for every u != 0 (u = 1 gives -0).
__device__ __forceinline__ float sqrt_rsq_zero_ok(float x) {
	const float y = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rsqf(x), 0.0f, 0x1p100f);
	const float s = x * y, h = 0.5f * y;
	const float r = __builtin_fmaf(-s, s, x);
	return __builtin_fmaf(r, h, s);
}

// sqrt_rsq / sqrt_rsq_zero_ok of N independent values, stage by stage. gfx950 wants one wait state between a transcendental
// instruction and the first use of its result: left to itself the scheduler emits each root as one chain (v_rsq, s_nop, ...),
// paying the s_nop -- an issue slot like any other -- N times. The barriers keep the N v_rsq together, which covers it.
template <int N, bool ZERO_OK>
__device__ __forceinline__ void sqrt_rsq_n(const float (&x)[N], float (&out)[N]) {
	float y[N], s[N], h[N];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < N; i++) y[i] = __builtin_amdgcn_rsqf(x[i]);
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < N; i++) {
		if (ZERO_OK) y[i] = __builtin_amdgcn_fmed3f(y[i], 0.0f, 0x1p100f);
		s[i] = x[i] * y[i], h[i] = 0.5f * y[i];
	}
#pragma unroll
	for (int i = 0; i < N; i++) out[i] = __builtin_fmaf(__builtin_fmaf(-s[i], s[i], x[i]), h[i], s[i]);
}

// ---- IEEE division with the operand scaling factored out ------------------------------
// hipcc expands a / b into v_div_scale (x2), v_rcp, two Newton steps on the reciprocal,
// q = a*r with two residual corrections, v_div_fmas and v_div_fixup: 11 instructions, one
// of them transcendental, per quotient. v_div_scale / v_div_fmas only rescale by 2^+-64 when
// an operand or the quotient comes near the ends of the exponent range, and v_div_fixup only
// replaces the result for zero / inf / NaN operands and out-of-range quotients (CDNA3 ISA
// guide, V_DIV_SCALE_F32 / V_DIV_FIXUP_F32). For
//     2^-40 <= |b| <= 2^40   and   2^-60 <= |a| <= 2^50
// none of those cases applies (both normal, exponent(a) > 23, -126 < e_a - e_b < 96, 1/b
// normal), so the expansion reduces to the plain sequence below, bit for bit -- and its
// first three instructions depend on b alone, so quotients that share a denominator share
// them. Outside that box the compiler's division runs. A NaN numerator gives NaN either way.
// srt_selftest_math compares both against `/` on the device (out[8], out[9]).
__device__ __forceinline__ float rcp_refined(float b) {
	float r = __builtin_amdgcn_rcpf(b);
	float e = __builtin_fmaf(-b, r, 1.0f);
	return __builtin_fmaf(e, r, r);
}
__device__ __forceinline__ float div_core(float a, float b, float r) {
	float q = a * r;
	float m = __builtin_fmaf(-b, q, a);
	q = __builtin_fmaf(m, r, q);
	m = __builtin_fmaf(-b, q, a);
	return __builtin_fmaf(m, r, q);
}
// a / b with y = the CORRECTLY ROUNDED 1 / b (an IEEE quotient made on the host), for 0 <= a < 2^32 that is zero or at least
// 2^-40 and 1 <= b <= 2^31: the camera's (pixel + jitter) / image size. q0 = a y is within 2 ulp of a / b, the first
// correction leaves a faithful quotient (its residual a - b q0 is exact in one fma), and for a faithful q and y = RN(1 / b)
// RN(q + (a - b q) y) is the correctly rounded quotient (Markstein, IBM J. Res. Dev. 34, 1990, theorem 8.5; no step over- or
// underflows in that range; a = +0 gives +0). Five plain instructions instead of the compiler's eleven, one of them
// transcendental. scripts/microbench/exact_math_probe.hip (2^32 quotients over eight image sizes) and srt_selftest_math
// compare it with `/` on the device.
__device__ __forceinline__ float div_by_rcp(float a, float b, float y) { return div_core(a, b, y); }
__device__ __forceinline__ bool div_num_ok(f3 a) {
	const float ax = dm_fabs(a.x), ay = dm_fabs(a.y), az = dm_fabs(a.z);
	const float mn = __builtin_fminf(__builtin_fminf(ax, ay), az); // v_min3 / v_max3: skip NaNs
	const float mx = __builtin_fmaxf(__builtin_fmaxf(ax, ay), az);
	return mn >= 0x1p-60f && mx <= 0x1p50f;
}
// a / b, component-wise
__device__ __forceinline__ f3 div3(f3 a, float b) {
	const float ab = dm_fabs(b);
	if (__builtin_expect(div_num_ok(a) && ab >= 0x1p-40f && ab <= 0x1p40f, 1)) {
		const float r = rcp_refined(b);
		return mk(div_core(a.x, b, r), div_core(a.y, b, r), div_core(a.z, b, r));
	}
	return a / b; // @rare (scripts/isa_phase_mix.py: behind a range guard, counted as never executed)
}
// a / b, component-wise, with y = the host's correctly rounded 1 / b, or 0 when b is outside [2^-40, 2^40] (or not a number): the
// sphere normal (p - c) / r with the radius' reciprocal from the winner record. Inside div3's box for the numerators the two
// residual steps of div_core give the IEEE quotient for y = RN(1 / b) (Markstein, see div_by_rcp) -- one transcendental and two
// fmas fewer than refining v_rcp_f32; everything else takes the compiler's division.
__device__ __forceinline__ f3 div3_by_rcp(f3 a, float b, float y) {
	if (__builtin_expect(div_num_ok(a) && y != 0.0f, 1)) return mk(div_core(a.x, b, y), div_core(a.y, b, y), div_core(a.z, b, y));
	return a / b; // @rare
}
// the built-in normalize: a * rsqrt(dot(a, a)) with detmath.h's division-free rsqrt -- 15 plain instructions, no
// transcendental, no guard (before: IEEE sqrt and three IEEE quotients behind a range check)
__device__ __forceinline__ f3 normalize3(f3 a) {
	const float r = dm_rsqrtf(dot3(a, a));
	return mk(a.x * r, a.y * r, a.z * r);
}
__device__ __forceinline__ f3 mix3(f3 x, f3 y, float a) {
	return mk(dm_mix(x.x, y.x, a), dm_mix(x.y, y.y, a), dm_mix(x.z, y.z, a));
}
__device__ __forceinline__ f3 ld3(const srt_float3 &p) { return mk(p.x, p.y, p.z); }
__device__ __forceinline__ f3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }

// The built-in sign (detmath.h dm_sign: 1, -1, the zero itself, 0 for a NaN) without branches: the sign bit over 1.0 where x is
// less or greater than 0 (v_cmp_lg: false for +-0 and NaN), else x where it is a zero, else 0. Five plain instructions (the
// generic form compiles to two nested exec-mask branches); equal to dm_sign on all 2^32 bit patterns (srt_selftest_math out[14]).
__device__ __forceinline__ float sign_fast(float x) {
	const float one = dm_u2f((dm_f2u(x) & 0x80000000u) | 0x3f800000u);
	const float zero_or_x = __builtin_amdgcn_class(x, 0x60) ? x : 0.0f; // class mask: -0 | +0
	return __builtin_islessgreater(x, 0.0f) ? one : zero_or_x;
}

// v * sign(d) for the WAVE (the bounce's `rd * sign(dot(n, rd))` and `n * sign(dot(n, dir))`). Where d is less or greater than 0,
// sign(d) is +-1 and the product is v or -v exactly: d's sign bit xor-ed into the three components (one v_and, three v_xor; the
// five instructions of sign_fast and the three multiplies go). One v_cmp_class vote on d (zero | NaN) sends the whole wave
// through today's form otherwise. A NaN component is the one value on which the xor and the multiply differ (the multiply
// keeps a NaN's sign, the xor flips it: exact_math_probe.hip "sign xor", NaN rows) -- and is never seen here: d is a dot
// product WITH v, so a NaN in v makes d NaN and the wave votes. EXHAUSTIVE for every other component, both signs, same probe.
// (Denormal components included: this build keeps f32 denormals -- build.py never passes -fgpu-flush-denormals-to-zero -- so
// v_mul_f32 by +-1 returns them unchanged, as the xor does. A build that flushed them would have to vote on them too.)
__device__ __forceinline__ f3 mul_sign_wave(f3 v, float d) {
	if (__builtin_expect(any64(__builtin_amdgcn_class(d, 0x63)), 0)) return v * sign_fast(d); // (wave-uniform) sNaN | qNaN | -0 | +0 @rare
	const uint32_t sb = dm_f2u(d) & 0x80000000u;
	return mk(dm_u2f(dm_f2u(v.x) ^ sb), dm_u2f(dm_f2u(v.y) ^ sb), dm_u2f(dm_f2u(v.z) ^ sb));
}

// column-major 4x4 times (v, w): ((m0*v.x + m1*v.y) + m2*v.z) + m3*w  (render.cl:114-120)
__device__ __forceinline__ f3 mat_by_vec(const srt_float4 *m, f3 v, float w) {
	return mk(((m[0].x * v.x + m[1].x * v.y) + m[2].x * v.z) + m[3].x * w,
	          ((m[0].y * v.x + m[1].y * v.y) + m[2].y * v.z) + m[3].y * w,
	          ((m[0].z * v.x + m[1].z * v.y) + m[2].z * v.z) + m[3].z * w);
}

// the same, the matrix given by its columns' x, y, z
__device__ __forceinline__ f3 mat_cols_by_vec(f3 c0, f3 c1, f3 c2, f3 c3, f3 v, float w) {
	return mk(((c0.x * v.x + c1.x * v.y) + c2.x * v.z) + c3.x * w, ((c0.y * v.x + c1.y * v.y) + c2.y * v.z) + c3.y * w,
	          ((c0.z * v.x + c1.z * v.y) + c2.z * v.z) + c3.z * w);
}

// The camera ray through the image point (x, y), in pixels: srt_trace_kernel's CAMERA with the point in place of pixel + jitter,
// for srt_pick_rays_kernel (ray_query.hip) and srt_id_pass_kernel (selection.hip). features_body.inc keeps its own form: it
// hoists the camera's columns out of its sample loop. p.rd: the camera and the frame; p.f_width .. p.inv_f_height as a dispatch
// of p.rd has them.
__device__ __forceinline__ void camera_ray(const TraceParams &p, float2 xy, f3 &org, f3 &dir) {
	const f3 c0 = mk(p.rd.camera_to_world[0].x, p.rd.camera_to_world[0].y, p.rd.camera_to_world[0].z);
	const f3 c1 = mk(p.rd.camera_to_world[1].x, p.rd.camera_to_world[1].y, p.rd.camera_to_world[1].z);
	const f3 c2 = mk(p.rd.camera_to_world[2].x, p.rd.camera_to_world[2].y, p.rd.camera_to_world[2].z);
	const f3 cam = mk(p.rd.camera_to_world[3].x, p.rd.camera_to_world[3].y, p.rd.camera_to_world[3].z);
	const float ndc_x = div_by_rcp(xy.x, p.f_width, p.inv_f_width);
	const float ndc_y = div_by_rcp(xy.y, p.f_height, p.inv_f_height);
	const float sx = ((2.f * ndc_x - 1.f) * p.rd.aspect_ratio) * p.rd.fov_scale;
	const float sy = (1.f - 2.f * ndc_y) * p.rd.fov_scale;
	org = cam;
	dir = normalize3(mat_cols_by_vec(c0, c1, c2, cam, mk(sx, sy, -1.0f), 0.0f));
}

// v - 2 (v.n) n  (render.cl:139-141)
__device__ __forceinline__ f3 reflect3(f3 v, f3 n) { return v - n * (2.0f * dot3(v, n)); }

// PCG-RXS-M-XS-32 (render.cl:143-148); (float)UINT_MAX == 2^32
// random_count = (float)r, random_float = random_count / 2^32. The scaling by 2^-32 is exact and
// never underflows (the smallest non-zero count is 1), so it commutes with any later rounding:
// users that can absorb it into a constant or an exponent take the count and save the multiply.
__device__ __forceinline__ uint32_t random_bits(uint32_t &seed) {
	seed = seed * 747796405u + 2891336453u;
	uint32_t r = ((seed >> ((seed >> 28) + 4u)) ^ seed) * 277803737u;
	return (r >> 22) ^ r;
}
__device__ __forceinline__ float random_count(uint32_t &seed) { return (float)random_bits(seed); }
__device__ __forceinline__ float random_float(uint32_t &seed) {
	return random_count(seed) * 2.3283064365386963e-10f; // exact: division by 2^32
}
// `probability > random_float(seed)` (render.cl:427-430) as an integer compare: random_float is a monotone function of the
// generator's 32 output bits r, so {r : p > random_float} is a prefix [0, T) of them; T(p) comes with the material from the
// host (srt_update_scene, found by bisection with the same int -> float conversion), the conversion and the scaling are not
// executed. Only for scenes whose probabilities all have T < 2^32 (p <= 1 does); others keep the float compare (unit_materials).
__device__ __forceinline__ bool bernoulli(float p_or_threshold, bool thresholds, uint32_t &seed) {
	if (thresholds) return random_bits(seed) < dm_f2u(p_or_threshold);
	return p_or_threshold > random_float(seed);
}

// dm_logf restricted to what random_float can return: 0 or a normal float in
// [2^-32, 1]. Same operations on that domain as detmath.h's dm_logf (whose negative /
// subnormal / inf / NaN handling can never trigger here), so the same bits.
// EXP_BIAS = 127 for u itself; 159 when handed the count c = u * 2^32 instead (same mantissa,
// exponent 32 higher, zero stays zero).
template <int EXP_BIAS, bool ZERO_OK>
__device__ __forceinline__ float log_unit_biased(float u) {
	const float LN2_HI = 6.93138123e-01f, LN2_LO = 9.05800061e-06f;
	const float L0 = 6.66666687e-01f, L1 = 4.00001287e-01f, L2 = 2.85499692e-01f, L3 = 2.33534276e-01f;
	uint32_t ix = dm_f2u(u);
	int k = (int)(ix >> 23) - EXP_BIAS;
	ix &= 0x007fffffu;
	uint32_t i = (ix + 0x4afb20u) & 0x00800000u;
	float x = dm_u2f(ix | (i ^ 0x3f800000u));
	k += (int)(i >> 23);
	float f = x - 1.0f;
	// f is +0 or a multiple of 2^-24 in [-0.293, 0.415] and 2 + f lies in [1.7, 2.42]: inside the
	// box of div_core (which also returns the +0 the division gives for f = +0)
	const float den = 2.0f + f;
	// f / den from the raw v_rcp_f32 and ONE residual step. Not a general division: f takes 2^24 values here, and the quotient is
	// the IEEE one for every single u the RNG can return (exhaustive: exact_math_probe.hip "log div D1"; srt_selftest_math
	// out[1] compares this function with dm_logf on all 2^32 of them). 1 + 3 instructions (shared-reciprocal form: 1 + 7).
	const float rc = __builtin_amdgcn_rcpf(den);
	const float q0 = f * rc;
	float s = __builtin_fmaf(__builtin_fmaf(-den, q0, f), rc, q0);
	float z = s * s;
	float R = z * dm_fmaf(z, dm_fmaf(z, dm_fmaf(z, L3, L2), L1), L0);
	float hfsq = (0.5f * f) * f;
	float dk = (float)k;
	float r = dm_fmaf(dk, LN2_HI, f - (hfsq - dm_fmaf(s, hfsq + R, dk * LN2_LO)));
	if (!ZERO_OK) return r; // the caller deals with u = 0 (for which r is some finite number)
	// Keep the zero test a select: left alone, the compiler sinks the whole polynomial into a branch
	// on u != 0, which also keeps the three logarithms of a bounce from being scheduled together.
	asm volatile("" : "+v"(r));
	return u == 0.0f ? -DM_INF_F : r;
}
__device__ __forceinline__ float log_unit(float u) { return log_unit_biased<127, true>(u); }
__device__ __forceinline__ float log_count(float c) { return log_unit_biased<159, true>(c); } // log(c / 2^32)

// dm_cosf restricted to finite x in [0, 8): detmath.h's range / NaN guard dropped.
__device__ __forceinline__ float cos_2pi(float x) {
	int k = (int)dm_fmaf(x, 6.36619747e-01f, 0.5f);
	float fk = (float)k;
	float r = dm_fmaf(-fk, 1.570796371e+00f, x);
	r = dm_fmaf(-fk, -4.371138829e-08f, r);
	r = dm_fmaf(-fk, -1.715124510e-15f, r);
	float z = r * r;
	int odd = k & 1;
	float c0 = odd ? -1.66666642e-01f : 4.16666642e-02f;
	float c1 = odd ? 8.33272468e-03f : -1.38882792e-03f;
	float c2 = odd ? -1.95828557e-04f : 2.45428964e-05f;
	float p = dm_fmaf(z, dm_fmaf(z, c2, c1), c0);
	float s_res = dm_fmaf(r * z, p, r);
	float c_res = dm_fmaf(z * z, p, dm_fmaf(-0.5f, z, 1.0f));
	float res = odd ? s_res : c_res;
	// -res in quadrants 1 and 2: bit 1 of k + 1, moved to the sign position and xor-ed in (three integer ops and no compare /
	// select pair; same bits as the select for every angle, srt_selftest_math out[2])
	return dm_u2f(dm_f2u(res) ^ ((((uint32_t)k << 30) + 0x40000000u) & 0x80000000u));
}

// Three Box-Muller normals (render.cl:150-158: x, y, z in that order, theta drawn before rho each time), the three square
// roots side by side. box_muller_draws makes the six draws (the rho draws' bits are kept for the wave form's vote) and the
// three arguments -2 log u, which are -0 (u = 1), +inf (u = 0) or in [1.19e-7, 44.4] for every u random_float can return.
__device__ __forceinline__ void box_muller_draws(uint32_t &seed, float (&th)[3], uint32_t (&rb)[3], float (&cnt)[3], float (&arg)[3]) {
#pragma unroll
	for (int k = 0; k < 3; k++) {
		th[k] = (6.28318548f * 2.3283064365386963e-10f) * random_count(seed); // = 6.28318548f * random_float, bit for bit
		rb[k] = random_bits(seed);
		cnt[k] = (float)rb[k];
	}
#pragma unroll
	for (int k = 0; k < 3; k++) arg[k] = -2.0f * log_unit_biased<159, false>(cnt[k]);
}
// The roots for EVERY u: sqrt_rsq_zero_ok, and u = 0 (whose logarithm is left some finite number) selected to sqrt(+inf) = +inf
// afterwards. Equal to the IEEE sqrt(-2 log u) for all 2^32 u: srt_selftest_math out[10]. Three v_med3 and three compare /
// select pairs, for 129 of the generator's 2^32 outputs.
__device__ __forceinline__ void box_muller_rho_any(const float (&arg)[3], const float (&cnt)[3], float (&rho)[3]) {
	sqrt_rsq_n<3, true>(arg, rho);
#pragma unroll
	for (int k = 0; k < 3; k++) {
		asm volatile("" : "+v"(rho[k])); // keep the zero test a select (see log_unit_biased)
		rho[k] = cnt[k] == 0.0f ? DM_INF_F : rho[k];
	}
}
// The per-lane form (the general kernels; the selftest's reference for the wave form below).
__device__ __forceinline__ f3 random_normal3_lane(uint32_t &seed) {
	float th[3], cnt[3], arg[3], rho[3];
	uint32_t rb[3];
	box_muller_draws(seed, th, rb, cnt, arg);
	box_muller_rho_any(arg, cnt, rho);
	return mk(rho[0] * cos_2pi(th[0]), rho[1] * cos_2pi(th[1]), rho[2] * cos_2pi(th[2]));
}
// The same for the WAVE. The two arguments sqrt_rsq gets wrong come from 129 generator outputs: r = 0 (u = 0, -2 log u = +inf)
// and the 128 largest, r >= 2^32 - 128, which the conversion rounds to 2^32 (u = 1, -2 log u = -0). One vote on the three rho
// draws' bits (v_min3_u32, v_max3_u32, two compares); a wave that holds one -- three draws x 64 lanes x 129 / 2^32: one bounce in
// 170,000 -- runs the per-lane tail above on all its lanes. Every other count is an integer in [1, 2^32 - 256]:
// u in [2^-32, 1 - 2^-24], log u in [-22.18, -5.96e-8], so -2 log u is a normal float in [1.19e-7, 44.4] -- far inside
// [2^-96, inf), where sqrt_rsq IS the IEEE root (exhaustive: srt_selftest_math out[12]) -- and the clamp of the reciprocal root
// and the select to +inf would be the identity. Checked draw by draw over all those counts: exact_math_probe.hip "Box-Muller
// sqrt S1 (admitted u)" (its sqrt_s1 is sqrt_rsq_n<3, false>'s sequence -- rsq, x y, y / 2, two fmas -- for one value, on
// -2 dm_logf(u), which log_unit_biased<159, false> equals on every count but 0: srt_selftest_math out[1], out[11]).
__device__ __forceinline__ bool rho_draws_rare(uint32_t r0, uint32_t r1, uint32_t r2) {
	return min(min(r0, r1), r2) == 0u || max(max(r0, r1), r2) >= 0xffffff80u;
}
__device__ __forceinline__ f3 random_normal3(uint32_t &seed) {
	float th[3], cnt[3], arg[3], rho[3];
	uint32_t rb[3];
	box_muller_draws(seed, th, rb, cnt, arg);
	if (__builtin_expect(any64(rho_draws_rare(rb[0], rb[1], rb[2])), 0)) box_muller_rho_any(arg, cnt, rho); // (wave-uniform) @rare
	else sqrt_rsq_n<3, false>(arg, rho);
	return mk(rho[0] * cos_2pi(th[0]), rho[1] * cos_2pi(th[1]), rho[2] * cos_2pi(th[2]));
}

// fp64 Schlick (render.cl:173-178); r0 = ((1-mu)/(1+mu))^2 is a per-material constant
__device__ __forceinline__ float schlick(float r0, float cos_theta) {
	double x = 1.0 - (double)cos_theta;
	double x5 = x * ((x * x) * (x * x)); // dm_pown_d(x, 5)
	return (float)((double)r0 + (1.0 - (double)r0) * x5);
}

} // namespace

#endif
