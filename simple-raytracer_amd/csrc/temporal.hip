// temporal.hip — temporal reprojection for the denoiser (include/srt_abi.h srt_set_denoise_temporal): SVGF's temporal
// half (Schied et al., HPG 2017) over the spatial filter of denoise.hip, for a camera that moves between clears.
//
// Per pixel p of the current frame (everything traced since the last clear: T dispatches, P samples), tests/temporal_ref.py
// restates it in numpy:
//   set-up     c_cur = canvas / T, m1_cur = lum(c_cur), m2_cur = M / T; N, Z, A, cov as srt_denoise_setup_kernel
//   reproject  no history when cov_p = 0 or c_cur is not finite. Same camera bit for bit (camera_to_world, aspect_ratio,
//              fov_scale): the one tap p, weight 1, D = Z_p. Else d = the camera ray through p's centre, X = cam + Z_p d,
//              D = |X - cam_h|, v = R_h^-1 (X - cam_h) (the host's inverse), none when v.z >= 0, else the bilinear 2x2
//              around fx = ((sx / (aspect_h fov_h) + 1) / 2) W - 0.5, fy = ((1 - sy / fov_h) / 2) H - 0.5 with
//              (sx, sy) = (v.x, v.y) / -v.z. A tap counts when it is in the image, cov_h > 0, c_h finite,
//              N_p . N_h >= normal_threshold and |Z_h - D| <= depth_threshold D. W = sum of the counted taps' weights;
//              W < 0.01: no history, else c_h, h, m1_h, m2_h = the weight-normalised sums
//   integrate  h' = min(h, history_limit), n = P + h'. h' = 0: the spatial set-up's values (for ticks = T, bit for bit).
//              Else c = (P c_cur + h' c_h) / n, m1, m2 likewise, V = max(0, m2 - m1^2) / n (non-finite: 0)
//   staging    {c, min(n, history_limit)}, {m1, m2} and the guide go to the set that becomes the history at the next clear
// One lane per pixel in 16x16 tiles, like srt_denoise_atrous_kernel; float4 loads, no atomics and no LDS, so runs are
// bit-identical.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/srt_abi.h"
#include "detmath.h"
#include "device_types.h"

#include "srt_internal.h"

namespace {

enum { TP_NONE = 0, TP_IDENTITY = 1, TP_PROJECT = 2 };

struct TemporalParams {
	int32_t width, height;
	int32_t mode;                  // TP_*: no history, the same camera, a camera move
	float T, P, F;                 // dispatches, samples, feature rays per pixel since the clear
	float limit;                   // history_limit
	float normal_threshold, depth_threshold;
	float f_width, f_height;       // exact conversions of width, height
	float c0[3], c1[3], c2[3], cam[3]; // current camera: rotation columns, position
	float aspect, fov;
	float rinv[9];                 // history camera: R_h^-1 (row-major), position, aspect_ratio, fov_scale
	float cam_h[3];
	float aspect_h, fov_h;
	const float4 *canvas;
	const float4 *normal_depth;
	const float4 *albedo_hits;
	const float *moments;
	const float4 *h_cc;    // history {colour, count}
	const float2 *h_m;     // history {m1, m2}
	const float4 *h_guide; // history guide, 2 float4 per pixel
	float4 *o_cc;          // staging set
	float2 *o_m;
	float4 *o_guide;
	float4 *out;    // {colour, variance} for the a-trous passes (NULL: the commit only integrates)
	uint32_t *argb; // K = 0 only
};

// as denoise.hip (srt_resolve_kernel's tonemap)
__device__ __forceinline__ float aces1(float x) {
	const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
	return dm_clamp((x * (x * a + b)) / (x * (x * c + d) + e), 0.0f, 1.0f);
}
__device__ __forceinline__ uint32_t to_uchar(float v) { return (v == v) ? ((uint32_t)(int)v & 255u) : 0u; }
__device__ __forceinline__ uint32_t tonemap(float x, float y, float z) {
	const float r = __builtin_sqrtf(aces1(x)), g = __builtin_sqrtf(aces1(y)), b = __builtin_sqrtf(aces1(z));
	return 255u | (to_uchar(r * 255.0f) << 8) | (to_uchar(g * 255.0f) << 16) | (to_uchar(b * 255.0f) << 24);
}
__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ bool finite3(float4 c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }

__global__ __launch_bounds__(256) void srt_temporal_setup_kernel(const TemporalParams p) {
	const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	// ---- the spatial set-up (srt_denoise_setup_kernel's expressions, divisor T) ----
	const float4 c = p.canvas[i], nd = p.normal_depth[i], ah = p.albedo_hits[i];
	const float m = p.moments[i];
	const float4 cc = make_float4(c.x / p.T, c.y / p.T, c.z / p.T, 0.f);
	const float l = lum(cc.x, cc.y, cc.z);
	const float m2c = m / p.T;
	float v = m2c - l * l;
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
	const float4 g0 = make_float4(nx, ny, nz, z);
	const float4 g1 = make_float4(ah.x / p.F, ah.y / p.F, ah.z / p.F, hits / p.F);

	// ---- reprojection ----
	float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sh = 0.f, s1 = 0.f, s2 = 0.f;
	if (p.mode != TP_NONE && g1.w > 0.f && finite3(cc)) {
		float D = z;
		int x0 = x, y0 = y;
		float ax = 0.f, ay = 0.f;
		bool any = true;
		if (p.mode == TP_PROJECT) {
			// the camera ray through the pixel's centre (kernels.hip CAMERA with 0.5 for the jitter; its division through the
			// host's reciprocal is the IEEE quotient)
			const float ndc_x = ((float)x + 0.5f) / p.f_width, ndc_y = ((float)y + 0.5f) / p.f_height;
			const float sx = ((2.f * ndc_x - 1.f) * p.aspect) * p.fov;
			const float sy = (1.f - 2.f * ndc_y) * p.fov;
			const float rx = ((p.c0[0] * sx + p.c1[0] * sy) + p.c2[0] * -1.0f) + p.cam[0] * 0.0f;
			const float ry = ((p.c0[1] * sx + p.c1[1] * sy) + p.c2[1] * -1.0f) + p.cam[1] * 0.0f;
			const float rz = ((p.c0[2] * sx + p.c1[2] * sy) + p.c2[2] * -1.0f) + p.cam[2] * 0.0f;
			const float rs = dm_rsqrtf(rx * rx + ry * ry + rz * rz);
			const float dx = rx * rs, dy = ry * rs, dz = rz * rs;
			const float ex = (p.cam[0] + z * dx) - p.cam_h[0], ey = (p.cam[1] + z * dy) - p.cam_h[1], ez = (p.cam[2] + z * dz) - p.cam_h[2];
			D = sqrtf(ex * ex + ey * ey + ez * ez);
			const float vx = (p.rinv[0] * ex + p.rinv[1] * ey) + p.rinv[2] * ez;
			const float vy = (p.rinv[3] * ex + p.rinv[4] * ey) + p.rinv[5] * ez;
			const float vz = (p.rinv[6] * ex + p.rinv[7] * ey) + p.rinv[8] * ez;
			const float qx = vx / -vz, qy = vy / -vz;
			const float fx = ((qx / (p.aspect_h * p.fov_h) + 1.f) / 2.f) * p.f_width - 0.5f;
			const float fy = ((1.f - qy / p.fov_h) / 2.f) * p.f_height - 0.5f;
			// in front of the history camera, and a 2x2 that touches the image (this also keeps the conversions in range)
			any = vz < 0.f && fx > -1.f && fx < p.f_width && fy > -1.f && fy < p.f_height;
			if (any) {
				const float flx = floorf(fx), fly = floorf(fy);
				x0 = (int)flx, y0 = (int)fly;
				ax = fx - flx, ay = fy - fly;
			}
		}
		if (any) {
			for (int k = 0; k < 4; k++) {
				const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
				const float w = (k & 1 ? ax : 1.f - ax) * (k >> 1 ? ay : 1.f - ay);
				if (p.mode == TP_IDENTITY && k) break;
				if (qx < 0 || qx >= p.width || qy < 0 || qy >= p.height) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				const float4 hg1 = p.h_guide[2 * j + 1];
				const float4 hc = p.h_cc[j];
				if (!(hg1.w > 0.f) || !finite3(hc)) continue;
				const float4 hg0 = p.h_guide[2 * j];
				if (!(nx * hg0.x + ny * hg0.y + nz * hg0.z >= p.normal_threshold)) continue;
				if (!(fabsf(hg0.w - D) <= p.depth_threshold * D)) continue;
				const float2 hm = p.h_m[j];
				sw += w;
				sr += w * hc.x, sg += w * hc.y, sb += w * hc.z;
				sh += w * hc.w;
				s1 += w * hm.x, s2 += w * hm.y;
			}
		}
	}

	// ---- integration ----
	float h = 0.f;
	if (sw >= 0.01f) h = fminf(sh / sw, p.limit);
	float4 o = make_float4(cc.x, cc.y, cc.z, v);
	float m1 = l, m2 = m2c, n = p.P;
	if (h > 0.f) {
		n = p.P + h;
		const float hr = sr / sw, hgc = sg / sw, hb = sb / sw, h1 = s1 / sw, h2 = s2 / sw;
		o.x = (p.P * cc.x + h * hr) / n;
		o.y = (p.P * cc.y + h * hgc) / n;
		o.z = (p.P * cc.z + h * hb) / n;
		m1 = (p.P * l + h * h1) / n;
		m2 = (p.P * m2c + h * h2) / n;
		float V = m2 - m1 * m1;
		V = V > 0.f ? V : 0.f;
		V = V / n;
		o.w = __builtin_isfinite(V) ? V : 0.f;
	}
	p.o_cc[i] = make_float4(o.x, o.y, o.z, fminf(n, p.limit));
	p.o_m[i] = make_float2(m1, m2);
	p.o_guide[2 * i] = g0;
	p.o_guide[2 * i + 1] = g1;
	if (p.out) p.out[i] = o;
	if (p.argb) p.argb[i] = tonemap(o.x, o.y, o.z);
}

size_t full_pixels(const srt_tracer *t) { return (size_t)t->width * (size_t)t->height; }

// set offsets, in floats: {colour, count} float4, {m1, m2} float2, guide 2 float4
size_t off_m(size_t px) { return px * 4; }
size_t off_guide(size_t px) { return px * 6; }
size_t set_floats(size_t px) { return px * 14; }

bool same_camera(const srt_render_data &a, const srt_render_data &b) {
	return memcmp(a.camera_to_world, b.camera_to_world, sizeof a.camera_to_world) == 0 &&
	       memcmp(&a.aspect_ratio, &b.aspect_ratio, sizeof(float)) == 0 && memcmp(&a.fov_scale, &b.fov_scale, sizeof(float)) == 0;
}

// R^-1 of the camera's upper 3x3 (columns camera_to_world[0..2]) in double, rounded to float, row-major; false when
// singular or not finite
bool invert_rotation(const srt_render_data &rd, float out[9]) {
	double m[3][3]; // m[row][col]
	const srt_float4 *c = rd.camera_to_world;
	for (int k = 0; k < 3; k++) m[0][k] = c[k].x, m[1][k] = c[k].y, m[2][k] = c[k].z;
	const double a = m[1][1] * m[2][2] - m[1][2] * m[2][1], b = m[1][2] * m[2][0] - m[1][0] * m[2][2], d = m[1][0] * m[2][1] - m[1][1] * m[2][0];
	const double det = m[0][0] * a + m[0][1] * b + m[0][2] * d;
	if (!(det != 0.0) || !std::isfinite(det)) return false;
	const double inv[9] = {a / det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det,
	                       b / det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det,
	                       d / det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det};
	for (int k = 0; k < 9; k++) {
		out[k] = (float)inv[k];
		if (!std::isfinite(out[k])) return false;
	}
	return true;
}

// the temporal set-up into the staging set (and `col` / argb when given)
int launch_setup(srt_tracer *t, float4 *col, uint32_t *argb) {
	const size_t px = full_pixels(t);
	float *hist = t->tp_set[t->tp_cur].ptr, *stage = t->tp_set[1 - t->tp_cur].ptr;
	TemporalParams p;
	memset(&p, 0, sizeof p);
	p.width = t->width;
	p.height = t->height;
	p.T = (float)t->dn_T;
	p.P = (float)t->dn_P;
	p.F = (float)t->dn_F;
	p.limit = (float)t->tp.history_limit;
	p.normal_threshold = t->tp.normal_threshold;
	p.depth_threshold = t->tp.depth_threshold;
	p.f_width = (float)t->width;
	p.f_height = (float)t->height;
	const srt_render_data &rd = t->dn_cam, &rh = t->tp_cam;
	const srt_float4 *cw = rd.camera_to_world;
	for (int k = 0; k < 3; k++) {
		const float *col_k[4] = {&cw[0].x, &cw[1].x, &cw[2].x, &cw[3].x};
		p.c0[k] = col_k[0][k], p.c1[k] = col_k[1][k], p.c2[k] = col_k[2][k], p.cam[k] = col_k[3][k];
	}
	p.aspect = rd.aspect_ratio;
	p.fov = rd.fov_scale;
	p.cam_h[0] = rh.camera_to_world[3].x, p.cam_h[1] = rh.camera_to_world[3].y, p.cam_h[2] = rh.camera_to_world[3].z;
	p.aspect_h = rh.aspect_ratio;
	p.fov_h = rh.fov_scale;
	p.mode = TP_NONE;
	if (t->tp_valid) {
		if (same_camera(rd, rh)) p.mode = TP_IDENTITY;
		else if (invert_rotation(rh, p.rinv)) p.mode = TP_PROJECT;
	}
	p.canvas = reinterpret_cast<const float4 *>(t->canvas);
	p.normal_depth = reinterpret_cast<const float4 *>(t->dn_nd.ptr);
	p.albedo_hits = reinterpret_cast<const float4 *>(t->dn_ah.ptr);
	p.moments = t->dn_mom.ptr;
	p.h_cc = reinterpret_cast<const float4 *>(hist);
	p.h_m = reinterpret_cast<const float2 *>(hist + off_m(px));
	p.h_guide = reinterpret_cast<const float4 *>(hist + off_guide(px));
	p.o_cc = reinterpret_cast<float4 *>(stage);
	p.o_m = reinterpret_cast<float2 *>(stage + off_m(px));
	p.o_guide = reinterpret_cast<float4 *>(stage + off_guide(px));
	p.out = col;
	p.argb = argb;
	const dim3 grid((unsigned)((t->width + 15) / 16), (unsigned)((t->height + 15) / 16));
	hipLaunchKernelGGL(srt_temporal_setup_kernel, grid, dim3(256), 0, t->stream, p);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

bool params_ok(const srt_temporal_params &p) {
	for (int k = 0; k < 4; k++)
		if (p.reserved[k]) return false;
	return p.history_limit >= 1 && p.history_limit <= (1 << 20) && p.normal_threshold >= -1.0f && p.normal_threshold <= 1.0f &&
	       std::isfinite(p.depth_threshold) && p.depth_threshold > 0.0f;
}

} // namespace

// ---- host side (srt_internal.h) --------------------------------------------------------------------------------------

void srt_temporal_drop(srt_tracer *t) {
	t->tp_valid = false;
	t->tp_fresh = false;
}

int srt_temporal_setup(srt_tracer *t, float4 *col, uint32_t *argb, const float4 **guide) {
	const int rc = launch_setup(t, col, argb);
	if (rc) return rc;
	const size_t px = full_pixels(t);
	*guide = reinterpret_cast<const float4 *>(t->tp_set[1 - t->tp_cur].ptr + off_guide(px));
	t->tp_fresh = true;
	return SRT_OK;
}

int srt_temporal_commit(srt_tracer *t) {
	if (!t->dn_on || !t->tp_on || t->dn_T == 0 || full_pixels(t) == 0) return SRT_OK; // nothing traced: the history stays
	if (!t->tp_fresh) {
		const int rc = launch_setup(t, nullptr, nullptr);
		if (rc) return rc;
	}
	t->tp_cur = 1 - t->tp_cur;
	t->tp_cam = t->dn_cam;
	t->tp_valid = true;
	t->tp_fresh = false;
	return SRT_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------------------------------

int srt_temporal_defaults(srt_temporal_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->enable = 1;
	out->history_limit = 32;
	out->normal_threshold = 0.9f;
	out->depth_threshold = 0.05f;
	return SRT_OK;
}

int srt_set_denoise_temporal(srt_tracer *t, const srt_temporal_params *params) {
	if (!t) return SRT_ERR_INVALID;
	if (!params || !params->enable) {
		if (t->tp_on) srt_temporal_drop(t);
		t->tp_on = false;
		return SRT_OK;
	}
	if (!params_ok(*params))
		return fail(t, SRT_ERR_INVALID, "srt_set_denoise_temporal: history_limit 1..2^20, normal_threshold -1..1, depth_threshold finite and > 0, reserved 0");
	if (!t->dn_on) return fail(t, SRT_ERR_STATE, "srt_set_denoise_temporal: the denoiser is off (srt_set_denoise)");
	if (t->world > 1) return fail(t, SRT_ERR_STATE, "srt_set_denoise_temporal: not available on a partitioned handle (srt_set_partition world > 1)");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	for (int k = 0; k < 2; k++) SRT_HIP(t, t->tp_set[k].reserve(set_floats(px)));
	if (!t->tp_on) srt_temporal_drop(t);
	t->tp = *params;
	t->tp_on = true;
	t->tp_fresh = false; // the staging set was integrated with the old settings
	return SRT_OK;
}

int srt_reset_denoise_history(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	srt_temporal_drop(t);
	return SRT_OK;
}

int srt_read_denoise_history(srt_tracer *t, float *colour_count, float *moments, float *guide, srt_render_data *camera, int *valid) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->tp_set[0].ptr) return fail(t, SRT_ERR_STATE, "srt_read_denoise_history: temporal reprojection was never enabled (srt_set_denoise_temporal)");
	const size_t px = full_pixels(t);
	if (valid) *valid = t->tp_valid ? 1 : 0;
	if (!t->tp_valid) {
		if (colour_count) memset(colour_count, 0, px * 16);
		if (moments) memset(moments, 0, px * 8);
		if (guide) memset(guide, 0, px * 32);
		if (camera) memset(camera, 0, sizeof *camera);
		return SRT_OK;
	}
	SRT_HIP(t, hipSetDevice(t->device));
	const float *h = t->tp_set[t->tp_cur].ptr;
	if (colour_count) SRT_HIP(t, hipMemcpyAsync(colour_count, h, px * 16, hipMemcpyDeviceToHost, t->stream));
	if (moments) SRT_HIP(t, hipMemcpyAsync(moments, h + off_m(px), px * 8, hipMemcpyDeviceToHost, t->stream));
	if (guide) SRT_HIP(t, hipMemcpyAsync(guide, h + off_guide(px), px * 32, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if (camera) *camera = t->tp_cam;
	return SRT_OK;
}
