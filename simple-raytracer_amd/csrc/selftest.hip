// selftest.hip -- kernels that check the device helpers against their generic definitions, on the device, and their launch
// wrappers (srt_selftest_math, srt_selftest_rare in srt_abi.hip).
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_intersect.h" // test_planes2 and the axis forms
#include "device_shading.h" // powi_uniform

// ---------------------------------------------------------------------------------
// Math self-test: the kernel-local specialisations against their generic definitions,
// and checksums of the generic ones for comparison with the HOST build of detmath.h.
// r walks 0, stride, 2*stride, ... over all 2^32 values; u = r * 2^-32 is exactly what
// random_float returns for that r.
//   out[0] sqrt_ieee(bits r) != __builtin_sqrtf   out[1] log_unit(u) != dm_logf(u)
//   out[2] cos_2pi(t) != dm_cosf(t), t = 2pi*u    out[3] sum of bits of dm_logf(u)
//   out[4] sum of bits of dm_cosf(t)              out[5] sum of bits of sqrt(u)
//   out[6] sum of bits of dm_atan2pif(u - 0.5, 0.37 - u)   out[7] sum of bits of dm_powf(u, 25)
//   out[8] div3(a, b) != a / b, or div3_by_rcp(a, b, RN(1 / b) or 0) != a / b          out[9] sum of bits of normalize(u - 0.5, 0.37 - u, (r & 0xffff) * 1e-3 - 30)
//          (a, b: random mantissas and signs, exponents straddling the fast paths' guards,
//           zero components mixed in)
//   out[10] Box-Muller's rho as random_normal3 computes it (sqrt_rsq_zero_ok of -2 log of the raw count, u = 0 selected to +inf)
//           != IEEE sqrt(-2 dm_logf(u))
//   out[11] the 2^-32 scaling folded away: log_count(r) != log_unit(u), or K' * r != 6.28318548f * u
//   out[12] sqrt_rsq(bits r) != __builtin_sqrtf for r a float in [2^-96, +inf) (every one of them at stride 1)
//   out[13] div_by_rcp((px + u), W, 1 / W) != (px + u) / W over eight image sizes W (the host's 1 / W passed in)
//   out[14] sign_fast(bits r) != dm_sign
//   out[15] powi_uniform(x, n) != dm_powi(x, n) for x = u, -u and the float with r's bits, n = 1 + (block % 32)
// ---------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ bool same_float(float a, float b) { return (a != a && b != b) || dm_f2u(a) == dm_f2u(b); }
__device__ __forceinline__ unsigned long long canon_bits(float a) { return (a != a) ? 0x7fc00000ull : (unsigned long long)dm_f2u(a); }
__device__ __forceinline__ uint32_t mix32(uint32_t &h) {
	h = h * 747796405u + 2891336453u;
	uint32_t r = ((h >> ((h >> 28) + 4u)) ^ h) * 277803737u;
	return (r >> 22) ^ r;
}
// random sign and mantissa, biased exponent uniform in [lo, lo + span)
__device__ __forceinline__ float rand_float_exp(uint32_t &h, uint32_t lo, uint32_t span) {
	const uint32_t m = mix32(h), e = lo + mix32(h) % span;
	return dm_u2f((m & 0x807fffffu) | (e << 23));
}
__device__ __forceinline__ bool same_f3(f3 a, f3 b) { return same_float(a.x, b.x) && same_float(a.y, b.y) && same_float(a.z, b.z); }
} // namespace

struct SelftestSizes {
	float w[8], inv_w[8]; // image sizes and their reciprocals as the HOST rounds them
};
__global__ __launch_bounds__(256) void srt_selftest_kernel(unsigned long long *out, uint32_t stride, const SelftestSizes sz) {
	unsigned long long bad_sqrt = 0, bad_log = 0, bad_cos = 0, s_log = 0, s_cos = 0, s_sqrt = 0, s_atan = 0, s_pow = 0;
	unsigned long long bad_div = 0, bad_norm = 0, bad_rn = 0, bad_fold = 0, bad_rsq = 0, bad_cam = 0, bad_sign = 0, bad_powi = 0;
	const int pw_n = 1 + (int)(blockIdx.x & 31u); // (uniform per workgroup, as powi_uniform requires)
	const unsigned long long total = (0x100000000ull + stride - 1) / stride;
	for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < total;
	     i += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t r = (uint32_t)(i * stride);
		const float asbits = dm_u2f(r);
		bad_sqrt += same_float(sqrt_ieee(asbits), __builtin_sqrtf(asbits)) ? 0 : 1;
		const float u = (float)r * 2.3283064365386963e-10f;
		const float lg = dm_logf(u);
		bad_log += same_float(log_unit(u), lg) ? 0 : 1;
		const float th = 6.28318548f * u;
		const float cs = dm_cosf(th);
		bad_cos += same_float(cos_2pi(th), cs) ? 0 : 1;
		s_log += canon_bits(lg);
		s_cos += canon_bits(cs);
		s_sqrt += canon_bits(dm_sqrtf(u));
		s_atan += canon_bits(dm_atan2pif(u - 0.5f, 0.37f - u));
		s_pow += canon_bits(dm_powf(u, 25.0f));
		const float cnt = (float)r;
		bad_fold += (same_float(log_count(cnt), log_unit(u)) && same_float((6.28318548f * 2.3283064365386963e-10f) * cnt, th)) ? 0 : 1;
		const float arg = -2.0f * lg;
		{
			float rho = sqrt_rsq_zero_ok(-2.0f * log_unit_biased<159, false>(cnt));
			rho = cnt == 0.0f ? DM_INF_F : rho;
			bad_rn += same_float(rho, __builtin_sqrtf(arg)) ? 0 : 1;
		}
		bad_sign += same_float(sign_fast(asbits), dm_sign(asbits)) ? 0 : 1;
		bad_powi += (same_float(powi_uniform(u, pw_n), dm_powi(u, pw_n)) && same_float(powi_uniform(-u, pw_n), dm_powi(-u, pw_n)) &&
		             same_float(powi_uniform(asbits, pw_n), dm_powi(asbits, pw_n)))
		                ? 0
		                : 1;
		if (r >= 0x0f800000u && r < 0x7f800000u) bad_rsq += same_float(sqrt_rsq(asbits), __builtin_sqrtf(asbits)) ? 0 : 1;
		{
			const float W = sz.w[r & 7u];
			const float a = (float)((r >> 3) % (uint32_t)W) + u;
			bad_cam += same_float(div_by_rcp(a, W, sz.inv_w[r & 7u]), a / W) ? 0 : 1;
		}
		// guards: numerators 2^-60 .. 2^50, denominator 2^-40 .. 2^40, squared length 2^-80 .. 2^80
		uint32_t h = r ^ 0x9e3779b9u;
		f3 a = mk(rand_float_exp(h, 127 - 64, 118), rand_float_exp(h, 127 - 64, 118), rand_float_exp(h, 127 - 64, 118));
		if ((r & 15u) == 3u) a.x = 0.0f;
		if ((r & 31u) == 5u) a.y = -0.0f;
		if ((r & 0xfffu) == 7u) a.z = dm_u2f(mix32(h)); // any bit pattern: denormals, inf, NaN
		float b = rand_float_exp(h, 127 - 44, 88);
		if ((r & 0xffffu) == 11u) b = dm_u2f(0x7fc00000u | (mix32(h) & 0x3fffffu)); // a NaN denominator now and then
		bad_div += same_f3(div3(a, b), a / b) ? 0 : 1;
		{ // the sphere normal's form: the host's correctly rounded 1 / b for b in [2^-40, 2^40], else 0 (WinnerRec.inv_w, scene_prep.cpp)
			const float ab = dm_fabs(b);
			const float y = (ab >= 0x1p-40f && ab <= 0x1p40f) ? 1.0f / b : 0.0f;
			bad_div += same_f3(div3_by_rcp(a, b, y), a / b) ? 0 : 1;
		}
		// the built-in normalize on a vector made from r with plain float operations: checksum against the host build
		const f3 nv = normalize3(mk(u - 0.5f, 0.37f - u, (float)(r & 0xffffu) * 1e-3f - 30.0f));
		bad_norm += canon_bits(nv.x) + canon_bits(nv.y) + canon_bits(nv.z);
	}
	atomicAdd(&out[0], bad_sqrt);
	atomicAdd(&out[1], bad_log);
	atomicAdd(&out[2], bad_cos);
	atomicAdd(&out[3], s_log);
	atomicAdd(&out[4], s_cos);
	atomicAdd(&out[5], s_sqrt);
	atomicAdd(&out[6], s_atan);
	atomicAdd(&out[7], s_pow);
	atomicAdd(&out[8], bad_div);
	atomicAdd(&out[9], bad_norm);
	atomicAdd(&out[10], bad_rn);
	atomicAdd(&out[11], bad_fold);
	atomicAdd(&out[12], bad_rsq);
	atomicAdd(&out[13], bad_cam);
	atomicAdd(&out[14], bad_sign);
	atomicAdd(&out[15], bad_powi);
}

void srt_launch_selftest(unsigned long long *out, uint32_t stride, void *stream) {
	SelftestSizes sz;
	const float w[8] = {1920.f, 1080.f, 256.f, 3840.f, 2160.f, 960.f, 37.f, 16777216.f};
	for (int i = 0; i < 8; i++) sz.w[i] = w[i], sz.inv_w[i] = 1.0f / w[i];
	hipLaunchKernelGGL(srt_selftest_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, out, stride, sz);
}

// The bounce's wave-voted forms (random_normal3, mul_sign_wave) against the per-lane forms they replaced,
// WAVE BY WAVE: one workgroup = one wave = 64 consecutive lanes of the input, so the caller decides which lanes of a wave hold
// a rare case (none, one, lane 0, lane 63, all). 8 input words and 4 output words per lane:
//   what 0  in {seed}                 out {x, y, z of the three normals, seed afterwards}
//   what 1  in {vx, vy, vz, d}        out {v * sign(d), 0}
// Both results go back to the host; *mismatches counts the words whose bits differ.
__global__ __launch_bounds__(64) void srt_selftest_rare_kernel(int what, const uint32_t *__restrict__ in, uint32_t *__restrict__ out_new,
                                                               uint32_t *__restrict__ out_ref, unsigned long long *mismatches) {
	const size_t lane = (size_t)blockIdx.x * 64u + threadIdx.x;
	const uint32_t *__restrict__ w = in + lane * 8u;
	f3 a = mk(0.0f, 0.0f, 0.0f), b = a;
	uint32_t ta = 0u, tb = 0u;
	if (what == 0) { // (uniform)
		uint32_t sa = w[0], sb = w[0];
		a = random_normal3(sa), b = random_normal3_lane(sb);
		ta = sa, tb = sb;
	} else {
		const f3 v = mk(dm_u2f(w[0]), dm_u2f(w[1]), dm_u2f(w[2]));
		const float d = dm_u2f(w[3]);
		a = mul_sign_wave(v, d), b = v * sign_fast(d);
	}
	const uint32_t ra[4] = {dm_f2u(a.x), dm_f2u(a.y), dm_f2u(a.z), ta}, rb[4] = {dm_f2u(b.x), dm_f2u(b.y), dm_f2u(b.z), tb};
	unsigned long long bad = 0;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		out_new[lane * 4u + k] = ra[k], out_ref[lane * 4u + k] = rb[k];
		bad += ra[k] != rb[k] ? 1u : 0u;
	}
	if (bad) atomicAdd(mismatches, bad);
}

void srt_launch_selftest_rare(int what, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, unsigned long long *mismatches, void *stream) {
	if (waves == 0) return;
	hipLaunchKernelGGL(srt_selftest_rare_kernel, dim3(waves), dim3(64), 0, (hipStream_t)stream, what, in, out_new, out_ref, mismatches);
}

// The axis twins' plane tests (device_intersect.h "AXIS PLANES") as an EXTEND phase of the benchmark layout's twin runs them
// (trace_body.inc: planes y, x | plane z), WAVE BY WAVE beside test_planes2 alone: numerators, guard, one vote over all 64
// lanes, then the folded tests or the reference's. what 0: in {org, dir, tmin}; what 1 (as in a camera phase): the origin is
// pl.cam_org for every lane, so the numerators are the wave's own; in {-, -, -, dir, tmin}. out {tmin, best}.
struct PlaneFormsArgs {
	float blk[32];    // the two staged plane blocks {p, 0, n, 0} x 2
	float cam_org[3];
};
__global__ __launch_bounds__(64) void srt_selftest_plane_forms_kernel(int what, const PlaneFormsArgs pl, const uint32_t *__restrict__ in, uint32_t *__restrict__ out_new,
                                                                      uint32_t *__restrict__ out_ref, uint32_t *__restrict__ fast, unsigned long long *mismatches) {
	constexpr uint32_t K0 = SRT_BLK_CODE(SRT_SHAPE_PLANE, 2), K1 = SRT_BLK_CODE(SRT_SHAPE_PLANE, 1);
	constexpr uint32_t A0 = SRT_AXES_PPS_YXZ & 15u, A1 = (SRT_AXES_PPS_YXZ >> 4) & 15u;
	const size_t lane = (size_t)blockIdx.x * 64u + threadIdx.x;
	const uint32_t *__restrict__ w = in + lane * 8u;
	const f3 org = what == 1 ? mk(pl.cam_org[0], pl.cam_org[1], pl.cam_org[2]) : mk(dm_u2f(w[0]), dm_u2f(w[1]), dm_u2f(w[2]));
	const f3 dir = mk(dm_u2f(w[3]), dm_u2f(w[4]), dm_u2f(w[5]));
	Blk16 b0, b1;
#pragma unroll
	for (int i = 0; i < 16; i++) b0.v[i] = pl.blk[i], b1.v[i] = pl.blk[16 + i];
	float tmin_r = dm_u2f(w[6]), tmin_n = tmin_r;
	int best_r = -1, best_n = -1;
	test_planes2(b0, 2u, org, dir, 0, tmin_r, best_r);
	test_planes2(b1, 1u, org, dir, 2, tmin_r, best_r);
	float an[3];
	axis_numerators<K0, A0>(b0.v, org, an);
	axis_numerators<K1, A1>(b1.v, org, an + 2);
	const bool pass = !any64(!axis_operands_ok<3>(an, dir));
	if (pass) {
		test_planes2_axis<A0>(an, 2u, dir, 0, tmin_n, best_n);
		test_planes2_axis<A1>(an + 2, 1u, dir, 2, tmin_n, best_n);
	} else {
		test_planes2(b0, 2u, org, dir, 0, tmin_n, best_n);
		test_planes2(b1, 1u, org, dir, 2, tmin_n, best_n);
	}
	out_new[lane * 2u] = dm_f2u(tmin_n), out_new[lane * 2u + 1u] = (uint32_t)best_n;
	out_ref[lane * 2u] = dm_f2u(tmin_r), out_ref[lane * 2u + 1u] = (uint32_t)best_r;
	if (threadIdx.x == 0) fast[blockIdx.x] = pass ? 1u : 0u;
	const unsigned long long bad = (dm_f2u(tmin_n) != dm_f2u(tmin_r) ? 1u : 0u) + (best_n != best_r ? 1u : 0u);
	if (bad) atomicAdd(mismatches, bad);
}

void srt_launch_selftest_plane_forms(int what, const float *planes32, const float *cam_org3, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref,
                                     uint32_t *fast, unsigned long long *mismatches, void *stream) {
	if (waves == 0) return;
	PlaneFormsArgs pl;
	for (int i = 0; i < 32; i++) pl.blk[i] = planes32[i];
	for (int i = 0; i < 3; i++) pl.cam_org[i] = cam_org3[i];
	hipLaunchKernelGGL(srt_selftest_plane_forms_kernel, dim3(waves), dim3(64), 0, (hipStream_t)stream, what, pl, in, out_new, out_ref, fast, mismatches);
}

// The NO_SPEC classes' bounce (device_shading.h "DIFFUSE WAVES") as a SHADE phase runs it, WAVE BY WAVE beside the per-lane form
// alone: the vote on the materials, the vote on the operands, then the short form or the per-lane form on all 64 lanes. 20
// input words per lane: {random_dir, dir, nrm, metallic threshold, transmittance threshold, smoothness, mask, mcolor, seed, -};
// 8 output words: {dir, mask, seed, 1 where the lane drew `transparent` (its dir is rough_dir then)}.
__global__ __launch_bounds__(64) void srt_selftest_diffuse_bounce_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out_new, uint32_t *__restrict__ out_ref,
                                                                         uint32_t *__restrict__ fast, unsigned long long *mismatches) {
	const size_t lane = (size_t)blockIdx.x * 64u + threadIdx.x;
	const uint32_t *__restrict__ w = in + lane * 20u;
	const f3 random_dir = mk(dm_u2f(w[0]), dm_u2f(w[1]), dm_u2f(w[2]));
	const f3 dir = mk(dm_u2f(w[3]), dm_u2f(w[4]), dm_u2f(w[5]));
	const f3 nrm = mk(dm_u2f(w[6]), dm_u2f(w[7]), dm_u2f(w[8]));
	const float metallic = dm_u2f(w[9]), transmittance = dm_u2f(w[10]), smoothness = dm_u2f(w[11]);
	const f3 mask = mk(dm_u2f(w[12]), dm_u2f(w[13]), dm_u2f(w[14]));
	const f3 mcolor = mk(dm_u2f(w[15]), dm_u2f(w[16]), dm_u2f(w[17]));
	f3 dir_r = dir, mask_r = mask, dir_n = dir, mask_n = mask;
	uint32_t seed_r = w[18], seed_n = w[18];
	const bool glass_r = bounce_nospec_lane(random_dir, nrm, smoothness, metallic, transmittance, mcolor, dir_r, mask_r, seed_r);
	bool glass_n = false;
	const bool pass = diffuse_wave_materials(metallic, transmittance) && diffuse_wave_operands(random_dir, dir, nrm, smoothness);
	if (pass) bounce_diffuse_wave(random_dir, mcolor, dir_n, mask_n, seed_n);
	else glass_n = bounce_nospec_lane(random_dir, nrm, smoothness, metallic, transmittance, mcolor, dir_n, mask_n, seed_n);
	const uint32_t rn[8] = {dm_f2u(dir_n.x), dm_f2u(dir_n.y), dm_f2u(dir_n.z), dm_f2u(mask_n.x), dm_f2u(mask_n.y), dm_f2u(mask_n.z), seed_n, glass_n ? 1u : 0u};
	const uint32_t rr[8] = {dm_f2u(dir_r.x), dm_f2u(dir_r.y), dm_f2u(dir_r.z), dm_f2u(mask_r.x), dm_f2u(mask_r.y), dm_f2u(mask_r.z), seed_r, glass_r ? 1u : 0u};
	unsigned long long bad = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		out_new[lane * 8u + k] = rn[k], out_ref[lane * 8u + k] = rr[k];
		bad += rn[k] != rr[k] ? 1u : 0u;
	}
	if (threadIdx.x == 0) fast[blockIdx.x] = pass ? 1u : 0u;
	if (bad) atomicAdd(mismatches, bad);
}

void srt_launch_selftest_diffuse_bounce(const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, uint32_t *fast, unsigned long long *mismatches, void *stream) {
	if (waves == 0) return;
	hipLaunchKernelGGL(srt_selftest_diffuse_bounce_kernel, dim3(waves), dim3(64), 0, (hipStream_t)stream, in, out_new, out_ref, fast, mismatches);
}
