// denoise.hip — the edge-aware denoiser (include/srt_abi.h srt_set_denoise): a spatial variance-guided a-trous filter,
// SVGF (Schied et al., HPG 2017) without its temporal part, over the canvas the trace kernel accumulates.
//
// Inputs, per pixel, accumulated since the last clear while the denoiser is on:
//   normal_depth  {sum of front-facing first-hit normals, sum of hit distances} over the hits of the feature rays
//   albedo_hits   {sum of hit material colours (sky: 1,1,1) over all feature rays, hits}   (kernels.hip srt_features_kernel)
//   moments       sum over dispatches of (1/n) sum_k lum(radiance_k)^2                    (frame.hip srt_reduce_kernel<true>)
// and the handle's counts T (dispatches), P (sum of num_samples), F (feature rays per pixel).
//
// Filter (tests/denoise_ref.py restates it in numpy):
//   set-up  c0 = canvas / ticks (per channel, as srt_resolve_kernel), V0 = max(0, M/T - lum(canvas/T)^2) / P (non-finite: 0),
//           N = normalize(sum of normals) (0 without hits), Z = sum t / hits, A = sum albedo / F, cov = hits / F
//   pass i  step s = 2^i, 5x5 taps q = p + s (dx, dy), h = [1/16, 1/4, 3/8, 1/4, 1/16], taps outside the image skipped,
//           w = h(dx) h(dy) exp(-|Zp - Zq| / (sz Zp s + 1e-6)) max(0, Np.Nq)^sn exp(-|Ap - Aq|^2 / sa^2)
//               exp(-|lp - lq| / (sl sqrt(g(V)p) + 1e-10)),
//           g = the 3x3 [1/4, 1/2, 1/4]^2 filter of the pass's input variance over in-image taps (renormalised),
//           c' = sum w c / sum w, V' = sum w^2 V / (sum w)^2; a tap with cov = 0 or a non-finite colour has weight 0; a pixel
//           with cov = 0 or a non-finite colour (or no weight at all) passes through unchanged
//   last    srt_resolve_kernel's tonemap (ACES fit, sqrt, bytes A,R,G,B); K = 0 gives the plain resolve's bytes.
// Albedo demodulation (srt_set_denoise_demodulation; tests/demod_ref.py), K >= 1 only: one launch after the set-up divides
//   a pixel with cov > 0 and a finite colour by D = max(A, SRT_DEMOD_EPS) per channel, I = c / D, V_I = V / lum(D)^2 (other
//   pixels stay as they are), the passes run the formula above over I and V_I without the albedo factor -- sigma_albedo is
//   ignored in this mode -- with lum(I) in the luminance term, and the last pass writes o = I' D_p, V' = V_I' lum(D_p)^2
//   for the pixels that were demodulated (one that got no weight: I_p D_p, within rounding of c, not bit-equal).
// Spatial variance estimate (srt_set_denoise_spatial_variance; tests/spatial_variance_ref.py), K >= 1 only: one launch before
//   the passes (after the demodulate launch) gives a pixel with fewer than min_samples samples the variance of the
//   edge-weighted moments of its 7x7 neighbourhood instead of its own (srt_denoise_spatial_variance_kernel below).
// History feedback (srt_set_denoise_history_feedback; tests/feedback_ref.py), K >= 1 and temporal reprojection only: pass 1 also
//   writes its colour result into the staging set of temporal.hip (srt_denoise_atrous_feedback_kernel below); the frame's own
//   output does not change.
// No atomics: every output is a fixed function of its inputs, so runs are bit-identical. The passes use the fast
// exp / log instructions: this stage is outside the parity contract (DESIGN.md "Denoiser").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/srt_abi.h"
#include "detmath.h"
#include "device_types.h"

#include "srt_internal.h"
#include "tonemap.h"

namespace {

struct FilterParams {
	int32_t width, height;
	uint32_t num_pixels;
	int32_t step;
	float sigma_l, sigma_n, sigma_z, inv_sigma_a2; // inv_sigma_a2 = min(1 / sigma_albedo^2, FLT_MAX)
	const float4 *guide;                           // 2 float4 per pixel: {N, Z}, {A, cov}
	const float4 *in;                              // {colour, variance}
	float4 *out;
	uint32_t *argb; // last pass only (else NULL): the tonemapped bytes
	float4 *staged; // the feedback form of pass 1 only (else NULL): the staging set's {colour, count} plane
};

struct SetupParams {
	uint32_t num_pixels;
	float ticks, T, P, F; // the resolve's divisor, dispatches, samples, feature rays per pixel
	const float4 *canvas;
	const float4 *normal_depth;
	const float4 *albedo_hits;
	const float *moments;
	float4 *guide;
	float4 *out;
	uint32_t *argb; // K = 0 only
};

__global__ __launch_bounds__(256) void srt_denoise_setup_kernel(const SetupParams p) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= p.num_pixels) return;
	const float4 c = p.canvas[i], nd = p.normal_depth[i], ah = p.albedo_hits[i];
	const float m = p.moments[i];
	const float4 c0 = make_float4(c.x / p.ticks, c.y / p.ticks, c.z / p.ticks, 0.f);
	const float l = lum(c.x / p.T, c.y / p.T, c.z / p.T);
	float v = m / p.T - l * l;
	v = v > 0.f ? v : 0.f;
	v = v / p.P;
	if (!__builtin_isfinite(v)) v = 0.f;
	const float hits = ah.w;
	float nx = 0.f, ny = 0.f, nz = 0.f, z = 0.f;
	if (hits > 0.f) {
		const float len = sqrtf(nd.x * nd.x + nd.y * nd.y + nd.z * nd.z);
		if (len > 0.f) nx = nd.x / len, ny = nd.y / len, nz = nd.z / len;
		z = nd.w / hits;
	}
	p.guide[2 * i] = make_float4(nx, ny, nz, z);
	p.guide[2 * i + 1] = make_float4(ah.x / p.F, ah.y / p.F, ah.z / p.F, hits / p.F);
	p.out[i] = make_float4(c0.x, c0.y, c0.z, v);
	if (p.argb) p.argb[i] = tonemap(c0.x, c0.y, c0.z);
}

// (The pass formula stands three times in this unit: here, in srt_denoise_atrous_demod_kernel and in atrous_feedback_pass, which
// restates both for pass 1 of the history feedback. An edit of the formula goes into all three; the feedback test's
// same-frame check holds the copies together bit for bit.)
__global__ __launch_bounds__(256) void srt_denoise_atrous_kernel(const FilterParams p) {
	const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	const float4 cp = p.in[i];
	const float4 g1p = p.guide[2 * i + 1];
	float4 o = cp;
	if (g1p.w > 0.f && finite3(cp)) {
		const float4 g0p = p.guide[2 * i];
		// g(V): 3x3 binomial prefilter of the input variance over in-image taps
		float gv = 0.f, gw = 0.f;
		for (int dy = -1; dy <= 1; dy++) {
			const int qy = y + dy;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -1; dx <= 1; dx++) {
				const int qx = x + dx;
				if (qx < 0 || qx >= p.width) continue;
				const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
				gv += k * p.in[(uint32_t)qy * (uint32_t)p.width + (uint32_t)qx].w;
				gw += k;
			}
		}
		gv = gv / gw;
		const float lp = lum(cp.x, cp.y, cp.z);
		const float inv_dl = 1.0f / (p.sigma_l * sqrtf(gv) + 1e-10f);
		const float inv_dz = 1.0f / (p.sigma_z * g0p.w * (float)p.step + 1e-6f);
		const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
		float sw = 0.f, sv = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
		for (int dy = -2; dy <= 2; dy++) {
			const int qy = y + dy * p.step;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -2; dx <= 2; dx++) {
				const int qx = x + dx * p.step;
				if (qx < 0 || qx >= p.width) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				const float4 g1q = p.guide[2 * j + 1];
				const float4 cq = p.in[j];
				if (!(g1q.w > 0.f) || !finite3(cq)) continue;
				const float4 g0q = p.guide[2 * j];
				const float d = g0p.x * g0q.x + g0p.y * g0q.y + g0p.z * g0q.z;
				if (!(d > 0.f)) continue; // max(0, d)^sigma_n = 0
				const float wn = __expf(p.sigma_n * __logf(d));
				const float ar = g1p.x - g1q.x, ag = g1p.y - g1q.y, ab = g1p.z - g1q.z;
				const float e = fabsf(g0p.w - g0q.w) * inv_dz + (ar * ar + ag * ag + ab * ab) * p.inv_sigma_a2 +
				                fabsf(lp - lum(cq.x, cq.y, cq.z)) * inv_dl;
				const float w = h[dx + 2] * h[dy + 2] * wn * __expf(-e);
				sw += w;
				sv += w * w * cq.w;
				sr += w * cq.x, sg += w * cq.y, sb += w * cq.z;
			}
		}
		if (sw > 0.f) o = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
	}
	p.out[i] = o;
	if (p.argb) p.argb[i] = tonemap(o.x, o.y, o.z);
}

struct DemodParams {
	uint32_t num_pixels;
	const float4 *guide;
	float4 *io; // the set-up's {colour, variance}, in place
};

// albedo demodulation: colour -> illumination, in place, between the set-up and the passes
__global__ __launch_bounds__(256) void srt_denoise_demodulate_kernel(const DemodParams p) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= p.num_pixels) return;
	const float4 g1 = p.guide[2 * i + 1];
	const float4 c = p.io[i];
	if (!(g1.w > 0.f) || !finite3(c)) return;
	const float dr = fmaxf(g1.x, SRT_DEMOD_EPS), dg = fmaxf(g1.y, SRT_DEMOD_EPS), db = fmaxf(g1.z, SRT_DEMOD_EPS);
	const float ld = lum(dr, dg, db);
	p.io[i] = make_float4(c.x / dr, c.y / dg, c.z / db, c.w / (ld * ld));
}

// srt_denoise_atrous_kernel over the illumination: no albedo term, so a tap is its {I, V_I} and {N, Z} alone (32 B, not 48).
// A tap without hits has N = 0 and fails d > 0, which is all its cov > 0 test would do; the centre keeps that test (a
// centre without hits is no filtered pixel). LAST: the remodulation and the tonemap. (atrous_feedback_pass<true, LAST> below is a
// copy of this body: edit both.)
template <bool LAST>
__global__ __launch_bounds__(256) void srt_denoise_atrous_demod_kernel(const FilterParams p) {
	const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	const float4 cp = p.in[i];
	const float4 g1p = p.guide[2 * i + 1];
	float4 o = cp;
	if (g1p.w > 0.f && finite3(cp)) {
		const float4 g0p = p.guide[2 * i];
		float gv = 0.f, gw = 0.f;
		for (int dy = -1; dy <= 1; dy++) {
			const int qy = y + dy;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -1; dx <= 1; dx++) {
				const int qx = x + dx;
				if (qx < 0 || qx >= p.width) continue;
				const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
				gv += k * p.in[(uint32_t)qy * (uint32_t)p.width + (uint32_t)qx].w;
				gw += k;
			}
		}
		gv = gv / gw;
		const float lp = lum(cp.x, cp.y, cp.z);
		const float inv_dl = 1.0f / (p.sigma_l * sqrtf(gv) + 1e-10f);
		const float inv_dz = 1.0f / (p.sigma_z * g0p.w * (float)p.step + 1e-6f);
		const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
		float sw = 0.f, sv = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
		for (int dy = -2; dy <= 2; dy++) {
			const int qy = y + dy * p.step;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -2; dx <= 2; dx++) {
				const int qx = x + dx * p.step;
				if (qx < 0 || qx >= p.width) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				const float4 g0q = p.guide[2 * j];
				const float4 cq = p.in[j];
				const float d = g0p.x * g0q.x + g0p.y * g0q.y + g0p.z * g0q.z;
				if (!(d > 0.f) || !finite3(cq)) continue; // max(0, d)^sigma_n = 0 (no hits: N = 0)
				const float wn = __expf(p.sigma_n * __logf(d));
				const float e = fabsf(g0p.w - g0q.w) * inv_dz + fabsf(lp - lum(cq.x, cq.y, cq.z)) * inv_dl;
				const float w = h[dx + 2] * h[dy + 2] * wn * __expf(-e);
				sw += w;
				sv += w * w * cq.w;
				sr += w * cq.x, sg += w * cq.y, sb += w * cq.z;
			}
		}
		if (sw > 0.f) o = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
		if (LAST) {
			const float dr = fmaxf(g1p.x, SRT_DEMOD_EPS), dg = fmaxf(g1p.y, SRT_DEMOD_EPS), db = fmaxf(g1p.z, SRT_DEMOD_EPS);
			const float ld = lum(dr, dg, db);
			o = make_float4(o.x * dr, o.y * dg, o.z * db, o.w * (ld * ld));
		}
	}
	p.out[i] = o;
	if (LAST) p.argb[i] = tonemap(o.x, o.y, o.z);
}

// Pass 1 in its feedback form (srt_set_denoise_history_feedback): the pass of srt_denoise_atrous_kernel (DEMOD false) or of
// srt_denoise_atrous_demod_kernel<LAST> (DEMOD true) -- the same statements in the same order -- which also stores the pixel's
// colour result into the rgb of the staging set's {colour, count} plane (p.staged): as colour, I' D_p under DEMOD (the expression
// LAST remodulates with), when the pixel entered the filter branch, received weight and all three values are finite; x, y, z
// alone in one 12-byte store, the count untouched. No lane reads that plane during the pass. argb may be NULL also for LAST (K = 1
// in the run a clear makes). One body for the three feedback kernels. The two kernels above keep bodies of their own: as
// wrappers of a body shared with these (tried: one template with a FEEDBACK parameter) they compiled to 6 to 8 % more
// instructions than before (2850 -> 3020, 752 -> 809, 914 -> 970), and with the switch off the library must launch what it launched.
template <bool DEMOD, bool LAST>
__device__ __forceinline__ void atrous_feedback_pass(const FilterParams &p) {
	const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	const float4 cp = p.in[i];
	const float4 g1p = p.guide[2 * i + 1];
	float4 o = cp;
	if (g1p.w > 0.f && finite3(cp)) {
		const float4 g0p = p.guide[2 * i];
		// g(V): 3x3 binomial prefilter of the input variance over in-image taps
		float gv = 0.f, gw = 0.f;
		for (int dy = -1; dy <= 1; dy++) {
			const int qy = y + dy;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -1; dx <= 1; dx++) {
				const int qx = x + dx;
				if (qx < 0 || qx >= p.width) continue;
				const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
				gv += k * p.in[(uint32_t)qy * (uint32_t)p.width + (uint32_t)qx].w;
				gw += k;
			}
		}
		gv = gv / gw;
		const float lp = lum(cp.x, cp.y, cp.z);
		const float inv_dl = 1.0f / (p.sigma_l * sqrtf(gv) + 1e-10f);
		const float inv_dz = 1.0f / (p.sigma_z * g0p.w * (float)p.step + 1e-6f);
		const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
		float sw = 0.f, sv = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
		for (int dy = -2; dy <= 2; dy++) {
			const int qy = y + dy * p.step;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -2; dx <= 2; dx++) {
				const int qx = x + dx * p.step;
				if (qx < 0 || qx >= p.width) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				float e;
				float4 cq;
				float wn;
				if constexpr (DEMOD) {
					const float4 g0q = p.guide[2 * j];
					cq = p.in[j];
					const float d = g0p.x * g0q.x + g0p.y * g0q.y + g0p.z * g0q.z;
					if (!(d > 0.f) || !finite3(cq)) continue; // max(0, d)^sigma_n = 0 (no hits: N = 0)
					wn = __expf(p.sigma_n * __logf(d));
					e = fabsf(g0p.w - g0q.w) * inv_dz + fabsf(lp - lum(cq.x, cq.y, cq.z)) * inv_dl;
				} else {
					const float4 g1q = p.guide[2 * j + 1];
					cq = p.in[j];
					if (!(g1q.w > 0.f) || !finite3(cq)) continue;
					const float4 g0q = p.guide[2 * j];
					const float d = g0p.x * g0q.x + g0p.y * g0q.y + g0p.z * g0q.z;
					if (!(d > 0.f)) continue; // max(0, d)^sigma_n = 0
					wn = __expf(p.sigma_n * __logf(d));
					const float ar = g1p.x - g1q.x, ag = g1p.y - g1q.y, ab = g1p.z - g1q.z;
					e = fabsf(g0p.w - g0q.w) * inv_dz + (ar * ar + ag * ag + ab * ab) * p.inv_sigma_a2 +
					    fabsf(lp - lum(cq.x, cq.y, cq.z)) * inv_dl;
				}
				const float w = h[dx + 2] * h[dy + 2] * wn * __expf(-e);
				sw += w;
				sv += w * w * cq.w;
				sr += w * cq.x, sg += w * cq.y, sb += w * cq.z;
			}
		}
		if (sw > 0.f) o = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
		[[maybe_unused]] float dr = 1.f, dg = 1.f, db = 1.f;
		if constexpr (DEMOD) dr = fmaxf(g1p.x, SRT_DEMOD_EPS), dg = fmaxf(g1p.y, SRT_DEMOD_EPS), db = fmaxf(g1p.z, SRT_DEMOD_EPS);
		float fr = o.x, fg = o.y, fb = o.z; // the colour that goes back
		if constexpr (DEMOD) fr = o.x * dr, fg = o.y * dg, fb = o.z * db;
		if constexpr (DEMOD && LAST) {
			const float ld = lum(dr, dg, db);
			o = make_float4(o.x * dr, o.y * dg, o.z * db, o.w * (ld * ld));
		}
		if (sw > 0.f && __builtin_isfinite(fr) && __builtin_isfinite(fg) && __builtin_isfinite(fb))
			*reinterpret_cast<float3 *>(p.staged + i) = make_float3(fr, fg, fb);
	}
	p.out[i] = o;
	if constexpr (!DEMOD || LAST) {
		if (p.argb) p.argb[i] = tonemap(o.x, o.y, o.z); // (NULL: a middle pass, or the clear's run)
	}
}

template <bool DEMOD, bool LAST>
__global__ __launch_bounds__(256) void srt_denoise_atrous_feedback_kernel(const FilterParams p) { atrous_feedback_pass<DEMOD, LAST>(p); }

// ---- spatial variance estimate (srt_set_denoise_spatial_variance; include/srt_abi.h has the definition, tests/spatial_variance_ref.py
// restates it): one launch between the set-up (and the demodulate launch) and the passes. A pixel with cov > 0, a finite
// colour and fewer than min_samples samples gets V = max(0, m2' - m1'^2) / s_p from the edge-weighted means m1', m2' of the
// moments of its 7x7 neighbourhood; only that pixel's variance slot is written, in place. (A neighbouring tile reads the
// float4 for its colour's finiteness while this one writes .w: no value that is read changes.)
struct SpatialVarParams {
	int32_t width, height;
	float min_samples;                    // (float)min_samples
	float T, P;                           // the spatial set-up's divisors (STAGED: unused)
	float sigma_n, sigma_z, inv_sigma_a2; // as FilterParams
	const float4 *guide;
	const float4 *canvas; // the spatial set-up's sources: s = P, m1 = lum(canvas / T), m2 = M / T
	const float *moments;
	const float4 *s_cc;   // STAGED, the temporal set-up's staging set: s = {c, count}.w, {m1, m2}
	const float2 *s_m;
	float4 *io;           // {colour, variance}
};

// what a tap contributes: its guide, its moments (DEMOD: scaled into illumination space, A unused) and whether it counts
struct SvTap {
	float4 g0;        // {N, Z}
	float ar, ag, ab; // A
	float m1, m2;
	bool ok;          // cov > 0, a finite colour, finite moments
};

enum { SV_R = 3, SV_HALO = 16 + 2 * SV_R, SV_ROW4 = 32, SV_ROW1 = 48 }; // LDS row strides: float4 arrays 32, the float array 48

// pixel j as a tap; *live = cov > 0 and a finite colour, *s = its sample count
template <bool STAGED, bool DEMOD>
__device__ inline SvTap sv_load(const SpatialVarParams &p, uint32_t j, bool *live, float *s) {
	SvTap t;
	t.g0 = p.guide[2 * j];
	const float4 g1 = p.guide[2 * j + 1];
	const float4 c = p.io[j];
	float m1, m2;
	if (STAGED) {
		*s = p.s_cc[j].w;
		const float2 m = p.s_m[j];
		m1 = m.x, m2 = m.y;
	} else {
		const float4 cv = p.canvas[j];
		*s = p.P;
		m1 = lum(cv.x / p.T, cv.y / p.T, cv.z / p.T);
		m2 = p.moments[j] / p.T;
	}
	*live = g1.w > 0.f && finite3(c);
	t.ok = *live && __builtin_isfinite(m1) && __builtin_isfinite(m2);
	if (DEMOD) {
		const float a = 1.0f / lum(fmaxf(g1.x, SRT_DEMOD_EPS), fmaxf(g1.y, SRT_DEMOD_EPS), fmaxf(g1.z, SRT_DEMOD_EPS));
		m1 = m1 * a;
		m2 = (m2 * a) * a;
		t.ar = t.ag = t.ab = 0.f;
	} else {
		t.ar = g1.x, t.ag = g1.y, t.ab = g1.z;
	}
	t.m1 = m1, t.m2 = m2;
	return t;
}

// one tap other than the centre into the sums; inv_dz = 1 / (sigma_z Zp r + 1e-6), r = max(|dx|, |dy|)
template <bool DEMOD>
__device__ inline void sv_tap(const SpatialVarParams &p, const SvTap &c, const SvTap &q, float inv_dz, float &sw, float &s1, float &s2) {
	if (!q.ok) return;
	const float d = c.g0.x * q.g0.x + c.g0.y * q.g0.y + c.g0.z * q.g0.z;
	if (!(d > 0.f)) return; // max(0, d)^sigma_n = 0
	const float wn = __expf(p.sigma_n * __logf(d));
	float e = fabsf(c.g0.w - q.g0.w) * inv_dz;
	if (!DEMOD) {
		const float ar = c.ar - q.ar, ag = c.ag - q.ag, ab = c.ab - q.ab;
		e = e + (ar * ar + ag * ag + ab * ab) * p.inv_sigma_a2;
	}
	const float w = wn * __expf(-e);
	sw += w;
	s1 += w * q.m1;
	s2 += w * q.m2;
}

// STAGED: the moments' source; DEMOD: illumination space; LDS: the 22x22 halo tile staged in LDS (else a tap is loaded where
// it is used, as in the a-trous passes). All instantiations run the same arithmetic in the same order.
template <bool STAGED, bool DEMOD, bool LDS>
__global__ __launch_bounds__(256) void srt_denoise_spatial_variance_kernel(const SpatialVarParams p) {
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
	const int x = x0 + tx, y = y0 + ty;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	SvTap c;
	float s = 0.f;
	bool qualifies = false;
	if (x < p.width && y < p.height) {
		bool live;
		c = sv_load<STAGED, DEMOD>(p, i, &live, &s);
		qualifies = live && s < p.min_samples;
	}
	float sw = 0.f, s1 = 0.f, s2 = 0.f;
	if (LDS) {
		// the halo tile: float4 rows of 32 and float rows of 48 entries, so that the two image rows a 32-lane group reads
		// fall on disjoint banks (16-B reads: 64 banks, 4-B reads: 32). A tap that does not count has m2 = NaN.
		__shared__ float4 t_g0[SV_HALO * SV_ROW4];
		__shared__ float4 t_am[SV_HALO * SV_ROW4];
		__shared__ float t_m2[SV_HALO * SV_ROW1];
		if (!__syncthreads_or(qualifies ? 1 : 0)) return; // no lane of the tile qualifies: nothing is staged
		for (int e = threadIdx.x; e < SV_HALO * SV_HALO; e += 256) {
			const int hy = e / SV_HALO, hx = e - hy * SV_HALO;
			const int qx = x0 - SV_R + hx, qy = y0 - SV_R + hy;
			SvTap q;
			q.ok = false;
			if (qx >= 0 && qx < p.width && qy >= 0 && qy < p.height) {
				bool live;
				float sq;
				q = sv_load<STAGED, DEMOD>(p, (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx, &live, &sq);
			}
			if (q.ok) {
				t_g0[hy * SV_ROW4 + hx] = q.g0;
				t_am[hy * SV_ROW4 + hx] = make_float4(q.ar, q.ag, q.ab, q.m1);
			}
			t_m2[hy * SV_ROW1 + hx] = q.ok ? q.m2 : __builtin_nanf("");
		}
		__syncthreads();
		if (!qualifies) return;
		const float zs = p.sigma_z * c.g0.w;
		const float inv_dz1 = 1.0f / (zs * 1.0f + 1e-6f), inv_dz2 = 1.0f / (zs * 2.0f + 1e-6f), inv_dz3 = 1.0f / (zs * 3.0f + 1e-6f);
		for (int dy = -SV_R; dy <= SV_R; dy++) {
			for (int dx = -SV_R; dx <= SV_R; dx++) {
				if (dx == 0 && dy == 0) {
					if (c.ok) sw += 1.0f, s1 += c.m1, s2 += c.m2; // the centre: weight 1
					continue;
				}
				const int hy = ty + SV_R + dy, hx = tx + SV_R + dx;
				SvTap q;
				q.m2 = t_m2[hy * SV_ROW1 + hx];
				q.ok = q.m2 == q.m2;
				if (!q.ok) continue;
				q.g0 = t_g0[hy * SV_ROW4 + hx];
				const float4 am = t_am[hy * SV_ROW4 + hx];
				q.ar = am.x, q.ag = am.y, q.ab = am.z, q.m1 = am.w;
				const int r = max(abs(dx), abs(dy));
				sv_tap<DEMOD>(p, c, q, r == 1 ? inv_dz1 : r == 2 ? inv_dz2 : inv_dz3, sw, s1, s2);
			}
		}
	} else {
		if (!qualifies) return;
		const float zs = p.sigma_z * c.g0.w;
		const float inv_dz1 = 1.0f / (zs * 1.0f + 1e-6f), inv_dz2 = 1.0f / (zs * 2.0f + 1e-6f), inv_dz3 = 1.0f / (zs * 3.0f + 1e-6f);
		for (int dy = -SV_R; dy <= SV_R; dy++) {
			const int qy = y + dy;
			if (qy < 0 || qy >= p.height) continue;
			for (int dx = -SV_R; dx <= SV_R; dx++) {
				const int qx = x + dx;
				if (qx < 0 || qx >= p.width) continue;
				if (dx == 0 && dy == 0) {
					if (c.ok) sw += 1.0f, s1 += c.m1, s2 += c.m2; // the centre: weight 1
					continue;
				}
				bool live;
				float sq;
				const SvTap q = sv_load<STAGED, DEMOD>(p, (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx, &live, &sq);
				const int r = max(abs(dx), abs(dy));
				sv_tap<DEMOD>(p, c, q, r == 1 ? inv_dz1 : r == 2 ? inv_dz2 : inv_dz3, sw, s1, s2);
			}
		}
	}
	const float m1 = s1 / sw, m2 = s2 / sw;
	float v = m2 - m1 * m1;
	v = v > 0.f ? v : 0.f;
	v = v / s;
	if (!__builtin_isfinite(v)) v = 0.f;
	reinterpret_cast<float *>(p.io)[4 * (size_t)i + 3] = v;
}

// the form the library launches: the halo tile in LDS, or (-DSRT_SV_GLOBAL, scripts/spatial_variance_probe.py's other
// build) the plain global loads; DESIGN.md "Spatial variance estimate" has both forms' times
#ifdef SRT_SV_GLOBAL
constexpr bool kSvLds = false;
#else
constexpr bool kSvLds = true;
#endif

void launch_spatial_variance(const SpatialVarParams &p, bool staged, bool demod, hipStream_t stream) {
	const dim3 grid((unsigned)((p.width + 15) / 16), (unsigned)((p.height + 15) / 16));
	if (staged && demod) hipLaunchKernelGGL((srt_denoise_spatial_variance_kernel<true, true, kSvLds>), grid, dim3(256), 0, stream, p);
	else if (staged) hipLaunchKernelGGL((srt_denoise_spatial_variance_kernel<true, false, kSvLds>), grid, dim3(256), 0, stream, p);
	else if (demod) hipLaunchKernelGGL((srt_denoise_spatial_variance_kernel<false, true, kSvLds>), grid, dim3(256), 0, stream, p);
	else hipLaunchKernelGGL((srt_denoise_spatial_variance_kernel<false, false, kSvLds>), grid, dim3(256), 0, stream, p);
}

bool params_ok(const srt_denoise_params &d) {
	auto sigma_ok = [](float s) { return std::isfinite(s) && s > 0.0f; };
	return d.iterations >= 0 && d.iterations <= 8 && d.feature_samples >= 1 && d.feature_samples <= 64 && sigma_ok(d.sigma_luminance) &&
	       sigma_ok(d.sigma_normal) && sigma_ok(d.sigma_depth) && sigma_ok(d.sigma_albedo) && d.reserved == 0;
}

} // namespace

// ---- host side (srt_internal.h) --------------------------------------------------------------------------------------

int srt_denoise_clear(srt_tracer *t) {
	const size_t px = full_pixels(t);
	SRT_HIP(t, hipMemsetAsync(t->dn_nd.ptr, 0, px * 16, t->stream));
	SRT_HIP(t, hipMemsetAsync(t->dn_ah.ptr, 0, px * 16, t->stream));
	SRT_HIP(t, hipMemsetAsync(t->dn_mom.ptr, 0, px * 4, t->stream));
	t->dn_T = t->dn_P = t->dn_F = 0;
	t->om_mixed = false;
	return SRT_OK;
}

// the feature pass's one fork: the kernels of the dispatch's kind (albedo textures: the texel at the first hit is the albedo,
// srt_texture.hip), storing shape indices when object motion is on (temporal.hip)
static void launch_features(srt_tracer *t, const FeatureParams &fp) {
	const bool tris = t->dn.object_motion && t->dn.vertex_motion; // per-triangle motion: the hit triangle's index beside the shape's
	if (t->last_trace_textured) {
		const TexFeatureParams fx = srt_with_textures<TexFeatureParams>(t, fp);
		if (tris) srt_launch_features_tris_tex(fx, t->om_ids[t->om_cur].ptr, t->vm_tri[t->om_cur].ptr, t->stream);
		else if (t->dn.object_motion) srt_launch_features_ids_tex(fx, t->om_ids[t->om_cur].ptr, t->stream);
		else srt_launch_features_tex(fx, t->stream);
	} else if (tris) srt_launch_features_tris(fp, t->om_ids[t->om_cur].ptr, t->vm_tri[t->om_cur].ptr, t->stream);
	else if (t->dn.object_motion) srt_launch_features_ids(fp, t->om_ids[t->om_cur].ptr, t->stream);
	else srt_launch_features(fp, t->stream);
}

int srt_denoise_after_trace(srt_tracer *t, const TraceParams &p, int num_samples) {
	const uint32_t ns = num_samples > 0 ? (uint32_t)num_samples : 0u;
	const uint32_t want = (uint32_t)(t->gd_on ? t->gd_feature_samples : t->dn.p.feature_samples);
	const uint32_t fs = want < ns ? want : ns;
	FeatureParams fp;
	fp.tp = p;
	// a group member (gd_on): its own rows into the planes behind its canvas rows; the counts are the group's (srt_group.hip)
	fp.normal_depth = t->gd_on ? gd_normal_depth(t) : t->dn_nd.ptr;
	fp.albedo_hits = t->gd_on ? gd_albedo_hits(t) : t->dn_ah.ptr;
	fp.num_pixels = (uint32_t)(t->gd_on ? owned_pixels(t) : full_pixels(t));
	fp.feature_samples = fs;
	if (t->dn.object_motion && t->dn.vertex_motion && fs > 0) { // the world vertices this frame is traced with, once per scene
		const int vrc = srt_vertex_table_sync(t);
		if (vrc) return vrc;
	}
	launch_features(t, fp);
	SRT_HIP(t, hipGetLastError());
	if (t->gd_on) return SRT_OK;
	srt_denoise_count(t, p.rd, t->dn.p.feature_samples);
	if (t->dn.object_motion && fs == 0) t->om_mixed = true; // a dispatch without feature rays wrote no shape indices
	return SRT_OK;
}

void srt_denoise_count(srt_tracer *t, const srt_render_data &rd, int feature_samples) {
	const uint32_t ns = rd.num_samples > 0 ? (uint32_t)rd.num_samples : 0u;
	t->dn_T += 1;
	t->dn_P += ns;
	t->dn_F += (uint32_t)feature_samples < ns ? (uint32_t)feature_samples : ns;
	t->dn_cam = rd;
	t->dn_serial++; // temporal.hip: a staging set made before this no longer holds what is traced since the clear
}

int srt_denoise_member(srt_tracer *t, int feature_samples) {
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // launches may still use the canvas that is about to be replaced
	if (feature_samples <= 0) {
		if (!t->gd_on) return SRT_OK;
		// what is accumulated stays: the canvas rows go back where they were before (as srt_set_denoise(t, NULL) keeps the canvas)
		const size_t rows_bytes = gd_plane_pixels(t->width, t->height, t->world, t->rows_per_block) * 16;
		SRT_HIP(t, hipMemcpyAsync(t->gd_prev_canvas, t->gd_pack.ptr, rows_bytes < t->gd_prev_bytes ? rows_bytes : t->gd_prev_bytes, hipMemcpyDeviceToDevice, t->stream));
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		t->canvas = t->gd_prev_canvas;
		t->canvas_bytes = t->gd_prev_bytes;
		t->gd_on = false;
		return SRT_OK;
	}
	const size_t floats = gd_slot_floats(gd_plane_pixels(t->width, t->height, t->world, t->rows_per_block));
	if (!t->gd_on) {
		SRT_HIP(t, t->gd_pack.reserve(floats));
		t->gd_prev_canvas = t->canvas;
		t->gd_prev_bytes = t->canvas_bytes;
		t->canvas = t->gd_pack.ptr;
		t->canvas_bytes = floats * sizeof(float); // srt_clear_canvas zeroes the canvas rows and the three planes in one fill
		t->gd_on = true;
	}
	t->gd_feature_samples = feature_samples;
	SRT_HIP(t, hipMemsetAsync(t->canvas, 0, t->canvas_bytes, t->stream));
	return SRT_OK;
}

// one pass: k = 0 .. K - 1, step 2^k, ping-pong between the two images of `col`; the last one writes argb (NULL: none)
static void launch_pass(srt_tracer *t, FilterParams fp, int k, const FilterPlan &plan, uint8_t *argb) {
	const size_t px = full_pixels(t);
	float4 *col = reinterpret_cast<float4 *>(t->dn_col.ptr);
	const dim3 grid((unsigned)((t->width + 15) / 16), (unsigned)((t->height + 15) / 16));
	const bool last = k == plan.K - 1, demod = plan.demod, feedback = plan.feedback && k == 0;
	fp.step = 1 << k;
	fp.in = col + (size_t)(k & 1) * px;
	fp.out = col + (size_t)((k + 1) & 1) * px;
	fp.argb = last ? reinterpret_cast<uint32_t *>(argb) : nullptr;
	if (!feedback) {
		fp.staged = nullptr;
		if (!demod) hipLaunchKernelGGL(srt_denoise_atrous_kernel, grid, dim3(256), 0, t->stream, fp);
		else if (last) hipLaunchKernelGGL(srt_denoise_atrous_demod_kernel<true>, grid, dim3(256), 0, t->stream, fp);
		else hipLaunchKernelGGL(srt_denoise_atrous_demod_kernel<false>, grid, dim3(256), 0, t->stream, fp);
	} else if (!demod) hipLaunchKernelGGL((srt_denoise_atrous_feedback_kernel<false, false>), grid, dim3(256), 0, t->stream, fp);
	else if (last) hipLaunchKernelGGL((srt_denoise_atrous_feedback_kernel<true, true>), grid, dim3(256), 0, t->stream, fp);
	else hipLaunchKernelGGL((srt_denoise_atrous_feedback_kernel<true, false>), grid, dim3(256), 0, t->stream, fp);
}

// What the front leaves for the passes after the first
struct FilterFront {
	FilterParams fp; // everything but the per-pass members
	FilterPlan plan;
};

// The filter's front: the set-up (spatial or temporal) into the filter image, the demodulate launch and the spatial-variance
// launch where those are on, and pass 1 (k = 0) -- in its feedback form when srt_set_denoise_history_feedback is on, which
// writes the pass's colour into the staging set the set-up has just written. A filter and a clear that has to make the staging
// set itself (srt_denoise_feedback_front) run this same code, so the history never depends on which of them ran.
static int filter_front(srt_tracer *t, uint32_t ticks_stopped, uint8_t *argb, FilterFront *f) {
	const size_t px = full_pixels(t);
	const FilterPlan plan = plan_filter(t->dn);
	const int K = plan.K;
	float4 *col = reinterpret_cast<float4 *>(t->dn_col.ptr);
	float4 *guide = reinterpret_cast<float4 *>(t->dn_guide.ptr);
	SetupParams sp;
	sp.num_pixels = (uint32_t)px;
	sp.ticks = (float)ticks_stopped;
	sp.T = (float)t->dn_T;
	sp.P = (float)t->dn_P;
	sp.F = (float)t->dn_F;
	sp.canvas = reinterpret_cast<const float4 *>(t->canvas);
	sp.normal_depth = reinterpret_cast<const float4 *>(t->dn_nd.ptr);
	sp.albedo_hits = reinterpret_cast<const float4 *>(t->dn_ah.ptr);
	sp.moments = t->dn_mom.ptr;
	sp.guide = guide;
	sp.out = col;
	sp.argb = K == 0 ? reinterpret_cast<uint32_t *>(argb) : nullptr;
	const float4 *fguide = guide;
	TemporalStaged staged = {nullptr, nullptr, nullptr};
	if (t->dn.temporal) { // temporal.hip: the set-up with the reprojected history blended in; it writes the guide into the staging set
		const int rc = srt_temporal_setup(t, col, sp.argb, &staged);
		if (rc) return rc;
		fguide = staged.guide;
	} else {
		hipLaunchKernelGGL(srt_denoise_setup_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, t->stream, sp);
		SRT_HIP(t, hipGetLastError());
	}
	if (plan.demod) { // colour -> illumination, in place on the set-up's image (whichever set-up ran)
		DemodParams dp;
		dp.num_pixels = (uint32_t)px;
		dp.guide = fguide;
		dp.io = col;
		hipLaunchKernelGGL(srt_denoise_demodulate_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, t->stream, dp);
		SRT_HIP(t, hipGetLastError());
	}
	FilterParams fp;
	memset(&fp, 0, sizeof fp);
	fp.width = t->width;
	fp.height = t->height;
	fp.num_pixels = (uint32_t)px;
	fp.sigma_l = t->dn.p.sigma_luminance;
	fp.sigma_n = t->dn.p.sigma_normal;
	fp.sigma_z = t->dn.p.sigma_depth;
	fp.inv_sigma_a2 = plan.inv_sigma_a2;
	fp.guide = fguide;
	if (plan.spatial_var) { // pixels with few samples: the variance of their 7x7 neighbourhood's moments (whichever set-up ran)
		SpatialVarParams vp;
		vp.width = t->width;
		vp.height = t->height;
		vp.min_samples = (float)t->dn.sv_min;
		vp.T = sp.T;
		vp.P = sp.P;
		vp.sigma_n = fp.sigma_n;
		vp.sigma_z = fp.sigma_z;
		vp.inv_sigma_a2 = fp.inv_sigma_a2;
		vp.guide = fguide;
		vp.canvas = sp.canvas;
		vp.moments = sp.moments;
		vp.s_cc = staged.cc;
		vp.s_m = staged.m;
		vp.io = col;
		launch_spatial_variance(vp, t->dn.temporal, plan.demod, t->stream);
		SRT_HIP(t, hipGetLastError());
	}
	if (K >= 1) { // the history feedback: pass 1's colour goes into the set the set-up staged
		fp.staged = plan.feedback ? const_cast<float4 *>(staged.cc) : nullptr;
		launch_pass(t, fp, 0, plan, argb);
		SRT_HIP(t, hipGetLastError());
	}
	f->fp = fp;
	f->plan = plan;
	return SRT_OK;
}

int srt_denoise_filter(srt_tracer *t, uint32_t ticks_stopped, uint8_t *argb) {
	if (full_pixels(t) == 0) return SRT_OK;
	FilterFront f;
	const int rc = filter_front(t, ticks_stopped, argb, &f);
	if (rc) return rc;
	for (int k = 1; k < f.plan.K; k++) {
		launch_pass(t, f.fp, k, f.plan, argb);
		SRT_HIP(t, hipGetLastError());
	}
	t->dn_out = f.plan.K & 1;
	t->dn_filtered = true;
	t->last_filter = f.plan;
	return SRT_OK;
}

int srt_denoise_feedback_front(srt_tracer *t) {
	FilterFront f;
	// no divisor: the temporal set-up divides by T. No ARGB: pass 1 gets none, whether or not it is the last pass (K = 1)
	const int rc = filter_front(t, 1u, nullptr, &f);
	if (rc) return rc;
	t->dn_filtered = false; // the filter's two images hold this run's set-up and pass 1, no filter result
	t->last_filter.feedback = f.plan.feedback; // the last pass 1 is this one; the rest still tells of the last filter
	return SRT_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------

int srt_denoise_defaults(srt_denoise_params *out) {
	if (!out) return SRT_ERR_INVALID;
	out->enable = 1;
	out->iterations = 5;
	out->feature_samples = 1;
	out->sigma_luminance = 4.0f;
	out->sigma_normal = 128.0f;
	out->sigma_depth = 1.0f;
	out->sigma_albedo = 0.1f;
	out->reserved = 0;
	return SRT_OK;
}

int srt_set_denoise(srt_tracer *t, const srt_denoise_params *params) {
	if (!t) return SRT_ERR_INVALID;
	if (!params || !params->enable) {
		t->dn.off(); // with every mode of the filter and the temporal stage
		srt_temporal_drop(t);
		return SRT_OK;
	}
	if (!params_ok(*params))
		return fail(t, SRT_ERR_INVALID, "srt_set_denoise: iterations 0..8, feature_samples 1..64, sigmas finite and > 0, reserved 0");
	if (t->world > 1) return fail(t, SRT_ERR_STATE, "srt_set_denoise: not available on a partitioned handle (srt_set_partition world > 1)");
	if (t->gd_on) return fail(t, SRT_ERR_STATE, "srt_set_denoise: the handle's group has its denoiser on (srt_group_set_denoise)");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	SRT_HIP(t, t->dn_nd.reserve(px * 4));
	SRT_HIP(t, t->dn_ah.reserve(px * 4));
	SRT_HIP(t, t->dn_mom.reserve(px));
	SRT_HIP(t, t->dn_guide.reserve(px * 8));
	SRT_HIP(t, t->dn_col.reserve(px * 8));
	const bool clear = !t->dn.on || params->feature_samples != t->dn.p.feature_samples;
	t->dn.p = *params;
	t->dn.on = true;
	if (clear) {
		t->dn_filtered = false;
		srt_temporal_drop(t);
		SRT_HIP(t, hipMemsetAsync(t->canvas, 0, t->canvas_bytes, t->stream)); // srt_clear_canvas
		return srt_denoise_clear(t);
	}
	return SRT_OK;
}

int srt_set_denoise_demodulation(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	if (enable && !t->dn.on) return fail(t, SRT_ERR_STATE, "srt_set_denoise_demodulation: the denoiser is off (srt_set_denoise)");
	t->dn.demod = enable != 0;
	return SRT_OK;
}

int srt_last_filter_demodulated(const srt_tracer *t, int *demodulated) {
	if (!t || !demodulated) return SRT_ERR_INVALID;
	*demodulated = t->last_filter.demod ? 1 : 0;
	return SRT_OK;
}

int srt_set_denoise_spatial_variance(srt_tracer *t, uint32_t min_samples) {
	if (!t) return SRT_ERR_INVALID;
	if (min_samples > (1u << 20)) return fail(t, SRT_ERR_INVALID, "srt_set_denoise_spatial_variance: min_samples 0..2^20");
	if (min_samples && !t->dn.on) return fail(t, SRT_ERR_STATE, "srt_set_denoise_spatial_variance: the denoiser is off (srt_set_denoise)");
	t->dn.sv_min = min_samples;
	return SRT_OK;
}

int srt_last_filter_spatial_variance(const srt_tracer *t, int *ran) {
	if (!t || !ran) return SRT_ERR_INVALID;
	*ran = t->last_filter.spatial_var ? 1 : 0;
	return SRT_OK;
}

int srt_resolve_denoised(srt_tracer *t, uint32_t ticks_stopped) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->dn.on) return fail(t, SRT_ERR_STATE, "srt_resolve_denoised: the denoiser is off (srt_set_denoise)");
	if (t->dn_T == 0) return fail(t, SRT_ERR_STATE, "srt_resolve_denoised: nothing traced since the last clear");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipEventRecord(t->ev_r0, t->stream));
	int rc = srt_denoise_filter(t, ticks_stopped, t->argb.ptr);
	if (rc) return rc;
	if ((rc = srt_exposure_apply_frame(t, ticks_stopped, t->argb.ptr))) return rc; // exposure.hip: nothing while the feature is off
	if ((rc = srt_selection_apply_frame(t, t->argb.ptr))) return rc;               // selection.hip: likewise
	SRT_HIP(t, hipEventRecord(t->ev_r1, t->stream));
	t->have_resolve_ev = true;
	return SRT_OK;
}

int srt_read_denoised(srt_tracer *t, float *rgba_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!rgba_out) return fail(t, SRT_ERR_INVALID, "srt_read_denoised: rgba_out is NULL");
	if (!t->dn_filtered) return fail(t, SRT_ERR_STATE, "srt_read_denoised: no filtered image (render or srt_resolve_denoised with the denoiser on)");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	SRT_HIP(t, hipMemcpyAsync(rgba_out, t->dn_col.ptr + (size_t)t->dn_out * px * 4, px * 16, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_read_denoise_inputs(srt_tracer *t, float *normal_depth, float *albedo_hits, float *moments, uint32_t counts[2]) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->dn_nd.ptr) return fail(t, SRT_ERR_STATE, "srt_read_denoise_inputs: the denoiser was never enabled");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	if (normal_depth) SRT_HIP(t, hipMemcpyAsync(normal_depth, t->dn_nd.ptr, px * 16, hipMemcpyDeviceToHost, t->stream));
	if (albedo_hits) SRT_HIP(t, hipMemcpyAsync(albedo_hits, t->dn_ah.ptr, px * 16, hipMemcpyDeviceToHost, t->stream));
	if (moments) SRT_HIP(t, hipMemcpyAsync(moments, t->dn_mom.ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if (counts) counts[0] = t->dn_T, counts[1] = t->dn_P;
	return SRT_OK;
}
