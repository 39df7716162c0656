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
//   illumination (srt_set_denoise_history_illumination; the ILLUM set-ups; tests/history_illumination_ref.py): a counted
//              tap of the projected 2x2 whose pixel and whose history pixel are both fully covered (cov == 1) enters the sums
//              as c_h (D_p / D_h) per channel, m1_h rl and (m2_h rl) rl with D = max(A, SRT_DEMOD_EPS), rl = lum(D_p) / lum(D_h);
//              the identity tap and every other tap stay in colour. The history's contents are the same either way
// One lane per pixel in 16x16 tiles, like srt_denoise_atrous_kernel; float4 loads, no atomics and no LDS, so runs are
// bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/srt_abi.h"
#include "detmath.h"
#include "device_types.h"

#include "srt_internal.h"
#include "tonemap.h"

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

// object motion (srt_set_denoise_object_motion): per-pixel shape indices of the frame and of the history, and the table of
// SRT_MOTION_WORDS words per shape {state, A (3x4, rows; current world -> history world), B (3x3, rows; normals)}
struct MotionParams {
	const uint32_t *ids, *h_ids;
	const uint32_t *table;
	uint32_t n_shapes;
};

// per-triangle motion (srt_set_denoise_vertex_motion): the frame's triangle index per pixel, the world-vertex tables of the
// frame and of the history (9 floats per instance triangle: P0, P1, P2) and each shape's first row (n_shapes + 1 entries)
struct VertexParams {
	const uint32_t *tris;
	const float *rows, *h_rows;
	const uint32_t *first;
};

// the history clamp (below): the two planes srt_temporal_bounds_kernel made of the frame, and gamma
struct ClampParams {
	const float4 *bounds;
	uint32_t num_pixels;
	float gamma;
};

// A set-up's kernel arguments: p, then mp, vp and cp for the variants that read them. A member the variant lacks is empty and
// takes no room, so the kernel-argument segment holds what the variant reads and nothing else.
template <class T> struct Absent {
	Absent() = default;
	__host__ __device__ Absent(const T &) {}
};
template <int MOTION, bool CLAMP> struct SetupArgs {
	TemporalParams p;
	[[no_unique_address]] std::conditional_t<MOTION >= 1, MotionParams, Absent<MotionParams>> mp;
	[[no_unique_address]] std::conditional_t<MOTION == 2, VertexParams, Absent<VertexParams>> vp;
	[[no_unique_address]] std::conditional_t<CLAMP, ClampParams, Absent<ClampParams>> cp;
};
static_assert(sizeof(SetupArgs<0, false>) == sizeof(TemporalParams) && sizeof(SetupArgs<1, true>) == sizeof(TemporalParams) + sizeof(MotionParams) + sizeof(ClampParams) &&
              sizeof(SetupArgs<2, true>) == sizeof(TemporalParams) + sizeof(MotionParams) + sizeof(VertexParams) + sizeof(ClampParams), "SetupArgs: no room for an absent member");

// The set-up, one instantiation per variant the host launches (launch_setup):
//   MOTION 0 the camera alone; 1 per-shape motion (mp), when object motion is on and a shape of the table is not STATIC; 2 also
//          per-triangle motion (vp), when a shape is DEFORMED
//   ILLUM  a counted tap of the projected 2x2 is rescaled from its own first-hit albedo to this pixel's before it is summed
//   CLAMP  the history colour is clamped into the bounds srt_temporal_bounds_kernel made of the frame (cp)
// With MOTION >= 1, per pixel p with shape index s = ids[p] (tests/temporal_ref.py reproject with a table restates it):
//   s invalid or NO_HISTORY   no history
//   s STATIC                  the camera-only arithmetic (the identity tap for the same camera, else the projection of X), and a
//                             tap whose history shape index is a MOVED / NO_HISTORY shape does not count
//   s MOVED                   X_h = A_s X (rows: ((a0 X.x + a1 X.y) + a2 X.z) + a3), projected into the history camera also
//                             when the cameras are the same, D = |X_h - cam_h|; a tap must carry history shape index s, and
//                             its normal is compared with normalise(B_s N_p) (zero length or not finite: no history)
//   s DEFORMED (MOTION 2)     as MOVED, with the map of include/srt_abi.h ("per-triangle motion"): the point at the same barycentric
//                             place of the same triangle as it stood in the history frame. tests/vertex_motion_ref.py restates it
template <int MOTION, bool ILLUM, bool CLAMP>
__global__ __launch_bounds__(256) void srt_temporal_kernel(const SetupArgs<MOTION, CLAMP> a) {
	const TemporalParams &p = a.p;
	[[maybe_unused]] const auto &mp = a.mp;
	[[maybe_unused]] const auto &vp = a.vp;
	[[maybe_unused]] const auto &cp = a.cp;
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
	float dpr = 0.f, dpg = 0.f, dpb = 0.f, lp = 0.f;
	bool full_p = false;
	if constexpr (ILLUM) {
		// the pixel's divisor as srt_denoise_demodulate_kernel forms it (a NaN channel: eps); only a fully covered pixel's colour
		// is albedo x illumination (hits / F is exactly 1 when every feature sample hit)
		dpr = fmaxf(g1.x, SRT_DEMOD_EPS), dpg = fmaxf(g1.y, SRT_DEMOD_EPS), dpb = fmaxf(g1.z, SRT_DEMOD_EPS);
		lp = lum(dpr, dpg, dpb);
		full_p = g1.w == 1.0f;
	}

	// ---- reprojection ----
	float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sh = 0.f, s1 = 0.f, s2 = 0.f;
	// the pixel's shape s and its state: a static shape keeps the camera-only arithmetic, a moved one maps X through A_s and
	// compares the taps' normals with normalise(B_s N_p). MOTION 0 leaves all of it as it is set here
	uint32_t sid = 0xffffffffu;
	const float *mrow = nullptr;
	float bnx = nx, bny = ny, bnz = nz;
	bool live = p.mode != TP_NONE && g1.w > 0.f && finite3(cc), moved = false, deformed = false;
	float p0x = 0.f, p0y = 0.f, p0z = 0.f, q0x = 0.f, q0y = 0.f, q0z = 0.f, e1x = 0.f, e1y = 0.f, e1z = 0.f, e2x = 0.f, e2y = 0.f, e2z = 0.f;
	float f1x = 0.f, f1y = 0.f, f1z = 0.f, f2x = 0.f, f2y = 0.f, f2z = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f, det = 1.f;
	if constexpr (MOTION >= 1) {
		if (live) {
			sid = mp.ids[i];
			live = sid < mp.n_shapes;
			if (live) {
				const uint32_t *row = mp.table + (size_t)sid * SRT_MOTION_WORDS;
				const uint32_t state = row[0];
				mrow = reinterpret_cast<const float *>(row + 1);
				live = state != SRT_MOTION_NO_HISTORY;
				moved = state == SRT_MOTION_MOVED;
				if (moved) {
					const float *b = mrow + 12;
					const float tx = (b[0] * nx + b[1] * ny) + b[2] * nz, ty = (b[3] * nx + b[4] * ny) + b[5] * nz, tz = (b[6] * nx + b[7] * ny) + b[8] * nz;
					const float len = sqrtf((tx * tx + ty * ty) + tz * tz);
					live = len > 0.f && __builtin_isfinite(len);
					bnx = tx / len, bny = ty / len, bnz = tz / len;
				}
				if constexpr (MOTION == 2) {
					// a deformed model: the pixel's triangle as it stands now (P) and as it stood in the history frame (Q). It projects
					// and takes only its own shape's taps, as a moved shape does; N_h = normalise((nu f1 + nv f2) + c gh)
					deformed = state == SRT_MOTION_DEFORMED;
					if (deformed) {
						moved = true;
						const uint32_t tri = vp.tris[i];
						live = tri < vp.first[sid + 1] - vp.first[sid]; // (0xffffffff: no triangle)
						if (live) {
							const float *P = vp.rows + (size_t)(row[1] + tri) * 9, *Q = vp.h_rows + (size_t)(row[1] + tri) * 9;
							p0x = P[0], p0y = P[1], p0z = P[2];
							q0x = Q[0], q0y = Q[1], q0z = Q[2];
							e1x = P[3] - p0x, e1y = P[4] - p0y, e1z = P[5] - p0z;
							e2x = P[6] - p0x, e2y = P[7] - p0y, e2z = P[8] - p0z;
							f1x = Q[3] - q0x, f1y = Q[4] - q0y, f1z = Q[5] - q0z;
							f2x = Q[6] - q0x, f2y = Q[7] - q0y, f2z = Q[8] - q0z;
							a11 = (e1x * e1x + e1y * e1y) + e1z * e1z;
							a12 = (e1x * e2x + e1y * e2y) + e1z * e2z;
							a22 = (e2x * e2x + e2y * e2y) + e2z * e2z;
							det = a11 * a22 - a12 * a12;
							const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
							const float hx = f1y * f2z - f1z * f2y, hy = f1z * f2x - f1x * f2z, hz = f1x * f2y - f1y * f2x;
							const float lc = sqrtf((cx * cx + cy * cy) + cz * cz), lh = sqrtf((hx * hx + hy * hy) + hz * hz);
							live = det > 0.f && __builtin_isfinite(det) && lc > 0.f && __builtin_isfinite(lc) && lh > 0.f && __builtin_isfinite(lh);
							const float ne1 = (nx * e1x + ny * e1y) + nz * e1z, ne2 = (nx * e2x + ny * e2y) + nz * e2z;
							const float nu = (a22 * ne1 - a12 * ne2) / det, nv = (a11 * ne2 - a12 * ne1) / det;
							const float cn = (nx * (cx / lc) + ny * (cy / lc)) + nz * (cz / lc);
							const float tx = (nu * f1x + nv * f2x) + cn * (hx / lh), ty = (nu * f1y + nv * f2y) + cn * (hy / lh), tz = (nu * f1z + nv * f2z) + cn * (hz / lh);
							const float len = sqrtf((tx * tx + ty * ty) + tz * tz);
							live = live && len > 0.f && __builtin_isfinite(len);
							bnx = tx / len, bny = ty / len, bnz = tz / len;
						}
					}
				}
			}
		}
	}
	const bool identity = p.mode == TP_IDENTITY && !moved;
	if (live) {
		float D = z;
		int x0 = x, y0 = y;
		float ax = 0.f, ay = 0.f;
		bool any = true;
		if (p.mode == TP_PROJECT || moved) {
			// the camera ray through the pixel's centre (trace_body.inc CAMERA with 0.5 for the jitter; its division through the
			// host's reciprocal is the IEEE quotient)
			const float ndc_x = ((float)x + 0.5f) / p.f_width, ndc_y = ((float)y + 0.5f) / p.f_height;
			const float sx = ((2.f * ndc_x - 1.f) * p.aspect) * p.fov;
			const float sy = (1.f - 2.f * ndc_y) * p.fov;
			const float rx = ((p.c0[0] * sx + p.c1[0] * sy) + p.c2[0] * -1.0f) + p.cam[0] * 0.0f;
			const float ry = ((p.c0[1] * sx + p.c1[1] * sy) + p.c2[1] * -1.0f) + p.cam[1] * 0.0f;
			const float rz = ((p.c0[2] * sx + p.c1[2] * sy) + p.c2[2] * -1.0f) + p.cam[2] * 0.0f;
			const float rs = dm_rsqrtf(rx * rx + ry * ry + rz * rz);
			const float dx = rx * rs, dy = ry * rs, dz = rz * rs;
			float wx = p.cam[0] + z * dx, wy = p.cam[1] + z * dy, wz = p.cam[2] + z * dz;
			bool xh_ok = true;
			if (deformed) { // the same barycentric place on the history's triangle (the affine map of the triangle's plane)
				const float ddx = wx - p0x, ddy = wy - p0y, ddz = wz - p0z;
				const float de1 = (ddx * e1x + ddy * e1y) + ddz * e1z, de2 = (ddx * e2x + ddy * e2y) + ddz * e2z;
				const float u = (a22 * de1 - a12 * de2) / det, v2 = (a11 * de2 - a12 * de1) / det;
				wx = (q0x + u * f1x) + v2 * f2x, wy = (q0y + u * f1y) + v2 * f2y, wz = (q0z + u * f1z) + v2 * f2z;
				xh_ok = __builtin_isfinite(wx) && __builtin_isfinite(wy) && __builtin_isfinite(wz);
			} else if (moved) {
				const float hx = ((mrow[0] * wx + mrow[1] * wy) + mrow[2] * wz) + mrow[3];
				const float hy = ((mrow[4] * wx + mrow[5] * wy) + mrow[6] * wz) + mrow[7];
				const float hz = ((mrow[8] * wx + mrow[9] * wy) + mrow[10] * wz) + mrow[11];
				wx = hx, wy = hy, wz = hz;
			}
			const float ex = wx - p.cam_h[0], ey = wy - p.cam_h[1], ez = wz - p.cam_h[2];
			D = sqrtf(ex * ex + ey * ey + ez * ez);
			const float vx = (p.rinv[0] * ex + p.rinv[1] * ey) + p.rinv[2] * ez;
			const float vy = (p.rinv[3] * ex + p.rinv[4] * ey) + p.rinv[5] * ez;
			const float vz = (p.rinv[6] * ex + p.rinv[7] * ey) + p.rinv[8] * ez;
			const float qx = vx / -vz, qy = vy / -vz;
			const float fx = ((qx / (p.aspect_h * p.fov_h) + 1.f) / 2.f) * p.f_width - 0.5f;
			const float fy = ((1.f - qy / p.fov_h) / 2.f) * p.f_height - 0.5f;
			// in front of the history camera, and a 2x2 that touches the image (this also keeps the conversions in range)
			any = vz < 0.f && fx > -1.f && fx < p.f_width && fy > -1.f && fy < p.f_height;
			any = any && xh_ok;
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
				if (identity && k) break;
				if (qx < 0 || qx >= p.width || qy < 0 || qy >= p.height) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				const float4 hg1 = p.h_guide[2 * j + 1];
				const float4 hc = p.h_cc[j];
				if (!(hg1.w > 0.f) || !finite3(hc)) continue;
				// a moved shape's tap must show that shape; a static one's must not show a shape that has left. (hs at this level and the
				// test on a bare `if constexpr`: a `continue` out of a braced block costs these kernels 18 to 61 instructions)
				[[maybe_unused]] uint32_t hs = 0xffffffffu;
				if constexpr (MOTION >= 1) hs = mp.h_ids[j];
				if constexpr (MOTION >= 1)
					if (moved ? hs != sid : (hs < mp.n_shapes && mp.table[(size_t)hs * SRT_MOTION_WORDS] != SRT_MOTION_STATIC)) continue;
				const float4 hg0 = p.h_guide[2 * j];
				if (!(bnx * hg0.x + bny * hg0.y + bnz * hg0.z >= p.normal_threshold)) continue;
				if (!(fabsf(hg0.w - D) <= p.depth_threshold * D)) continue;
				const float2 hm = p.h_m[j];
				sw += w;
				if constexpr (ILLUM) {
					// r = D_p / D_h per channel, rl = lum(D_p) / lum(D_h); a partly covered pixel or tap stays in colour (it holds sky
					// light no albedo scaled), and so does the identity tap: the pixel itself
					float rr = 1.f, rg = 1.f, rb = 1.f, rl = 1.f;
					if (full_p && hg1.w == 1.0f && !identity) {
						const float dhr = fmaxf(hg1.x, SRT_DEMOD_EPS), dhg = fmaxf(hg1.y, SRT_DEMOD_EPS), dhb = fmaxf(hg1.z, SRT_DEMOD_EPS);
						rr = dpr / dhr, rg = dpg / dhg, rb = dpb / dhb;
						rl = lp / lum(dhr, dhg, dhb);
					}
					sr += w * (hc.x * rr), sg += w * (hc.y * rg), sb += w * (hc.z * rb);
					sh += w * hc.w;
					s1 += w * (hm.x * rl), s2 += w * ((hm.y * rl) * rl);
				} else {
					sr += w * hc.x, sg += w * hc.y, sb += w * hc.z;
					sh += w * hc.w;
					s1 += w * hm.x, s2 += w * hm.y;
				}
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
		float hr = sr / sw, hgc = sg / sw, hb = sb / sw, h1 = s1 / sw, h2 = s2 / sw;
		if constexpr (CLAMP) {
			// the history colour x_h is complete here (gathered, and rescaled under ILLUM): each channel into
			// [mu - gamma sigma, mu + gamma sigma] of this pixel's bounds (sum of weights 0: no clamp). By comparisons, so a NaN on
			// either side moves nothing; when no channel moved every value below is what it is without the clamp
			const float4 b0 = cp.bounds[i];
			if (b0.w > 0.f) {
				const float4 b1 = cp.bounds[cp.num_pixels + i];
				const float er = cp.gamma * b1.x, eg = cp.gamma * b1.y, eb = cp.gamma * b1.z;
				const float lor = b0.x - er, hir = b0.x + er, log_ = b0.y - eg, hig = b0.y + eg, lob = b0.z - eb, hib = b0.z + eb;
				bool mv = false;
				if (hr < lor) hr = lor, mv = true;
				else if (hr > hir) hr = hir, mv = true;
				if (hgc < log_) hgc = log_, mv = true;
				else if (hgc > hig) hgc = hig, mv = true;
				if (hb < lob) hb = lob, mv = true;
				else if (hb > hib) hb = hib, mv = true;
				if (mv) { // the moments follow the colour and keep their variance
					float hv = h2 - h1 * h1;
					hv = hv > 0.f ? hv : 0.f;
					h1 = lum(hr, hgc, hb);
					h2 = hv + h1 * h1;
				}
			}
		}
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

// ---- the history clamp (srt_set_denoise_history_clamp; include/srt_abi.h has the definition, tests/history_clamp_ref.py restates
// it): one launch before the set-up makes per-pixel colour bounds of the frame, and the set-up's clamping form pulls the
// history colour of a pixel into them before it is blended in.
struct BoundsParams {
	int32_t width, height;
	uint32_t num_pixels;
	float T, F;                           // the set-up's divisors
	float sigma_n, sigma_z, inv_sigma_a2; // as the filter's FilterParams
	const float4 *canvas;
	const float4 *normal_depth;
	const float4 *albedo_hits;
	float4 *bounds; // plane 0 {mu.rgb, sum of weights (0: do not clamp)}, plane 1 {sigma.rgb, counting taps}
};

enum { TB_R = 3, TB_HALO = 16 + 2 * TB_R, TB_ROW = 32 }; // the 22x22 halo tile, rows of 32 float4

// Per pixel p with cov > 0 and a finite colour c_p = canvas_p / T: over the 49 taps q = p + (dx, dy), |dx|, |dy| <= 3 (dy outer,
// dx inner) that are inside the image, have cov > 0 and a finite colour, with the spatial variance estimate's geometric weight
// w = exp(-|Zp - Zq| / (sz Zp r + 1e-6)) max(0, Np.Nq)^sn exp(-|Ap - Aq|^2 / sa^2), r = max(|dx|, |dy|) (the centre: 1),
// mu = sum w c / sum w, s = sum w c^2 / sum w, sigma = sqrt(max(0, s - mu^2)) per channel, evaluated on e = c_q - c_p (mu =
// c_p + sum w e / sum w, sigma^2 = sum w e^2 / sum w - (sum w e / sum w)^2: the same numbers without the cancellation of two
// large squares where the colour is bright and the spread small). No atomics, a fixed tap order.
// The tile is three float4 arrays ({c, counts ? 1 : 0}, {N, Z}, {A, -}) with rows of 32 entries = 128 dwords: a 16-B LDS read
// is served in groups of 16 lanes that take 8 pixels of one image row and 4 + 4 of the next (64 banks), and with that stride
// the next row starts on bank 0 again, so pixels 0-3 and 12-15 of one row (banks 0-15, 48-63) and 4-11 of the other (16-47)
// never meet. A tap that does not count costs one read (its marker), the two other arrays hold nothing for it.
__global__ __launch_bounds__(256) void srt_temporal_bounds_kernel(const BoundsParams p) {
	__shared__ float4 t_c[TB_HALO * TB_ROW];
	__shared__ float4 t_g0[TB_HALO * TB_ROW];
	__shared__ float4 t_a[TB_HALO * TB_ROW];
	const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
	const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
	for (int e = threadIdx.x; e < TB_HALO * TB_HALO; e += 256) {
		const int hy = e / TB_HALO, hx = e - hy * TB_HALO;
		const int qx = x0 - TB_R + hx, qy = y0 - TB_R + hy;
		float4 cc = make_float4(0.f, 0.f, 0.f, 0.f);
		if (qx >= 0 && qx < p.width && qy >= 0 && qy < p.height) {
			// the set-up's expressions (srt_temporal_kernel): colour, cov = hits / F, N, Z, A
			const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
			const float4 c = p.canvas[j], ah = p.albedo_hits[j];
			cc = make_float4(c.x / p.T, c.y / p.T, c.z / p.T, 0.f);
			const float hits = ah.w;
			if (hits / p.F > 0.f && finite3(cc)) {
				const float4 nd = p.normal_depth[j];
				float nx = 0.f, ny = 0.f, nz = 0.f;
				const float len = sqrtf(nd.x * nd.x + nd.y * nd.y + nd.z * nd.z);
				if (len > 0.f) nx = nd.x / len, ny = nd.y / len, nz = nd.z / len;
				cc.w = 1.f;
				t_g0[hy * TB_ROW + hx] = make_float4(nx, ny, nz, nd.w / hits);
				t_a[hy * TB_ROW + hx] = make_float4(ah.x / p.F, ah.y / p.F, ah.z / p.F, 0.f);
			}
		}
		t_c[hy * TB_ROW + hx] = cc;
	}
	__syncthreads();
	const int x = x0 + tx, y = y0 + ty;
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	const int ce = (ty + TB_R) * TB_ROW + tx + TB_R;
	const float4 cp = t_c[ce];
	float4 o0 = make_float4(0.f, 0.f, 0.f, 0.f), o1 = o0;
	if (cp.w > 0.f) {
		const float4 g0p = t_g0[ce], ap = t_a[ce];
		const float zs = p.sigma_z * g0p.w;
		const float inv_dz1 = 1.0f / (zs * 1.0f + 1e-6f), inv_dz2 = 1.0f / (zs * 2.0f + 1e-6f), inv_dz3 = 1.0f / (zs * 3.0f + 1e-6f);
		float sw = 0.f, s1r = 0.f, s1g = 0.f, s1b = 0.f, s2r = 0.f, s2g = 0.f, s2b = 0.f;
		int taps = 0;
		for (int dy = -TB_R; dy <= TB_R; dy++) {
			for (int dx = -TB_R; dx <= TB_R; dx++) {
				if (dx == 0 && dy == 0) { // the centre: weight 1
					taps++;
					sw += 1.0f;
					continue; // (its difference from itself adds 0 to every sum)
				}
				const int qe = (ty + TB_R + dy) * TB_ROW + tx + TB_R + dx;
				const float4 cq = t_c[qe];
				if (!(cq.w > 0.f)) continue;
				taps++;
				const float4 g0q = t_g0[qe];
				const float d = g0p.x * g0q.x + g0p.y * g0q.y + g0p.z * g0q.z;
				if (!(d > 0.f)) continue; // max(0, d)^sigma_n = 0: it counts and weighs nothing
				const float4 aq = t_a[qe];
				const float wn = __expf(p.sigma_n * __logf(d));
				const int r = max(abs(dx), abs(dy));
				const float ar = ap.x - aq.x, ag = ap.y - aq.y, ab = ap.z - aq.z;
				const float e = fabsf(g0p.w - g0q.w) * (r == 1 ? inv_dz1 : r == 2 ? inv_dz2 : inv_dz3) + (ar * ar + ag * ag + ab * ab) * p.inv_sigma_a2;
				const float w = wn * __expf(-e);
				sw += w;
				const float er = cq.x - cp.x, eg = cq.y - cp.y, eb = cq.z - cp.z;
				s1r += w * er, s1g += w * eg, s1b += w * eb;
				s2r += w * (er * er), s2g += w * (eg * eg), s2b += w * (eb * eb);
			}
		}
		const float dr = s1r / sw, dg = s1g / sw, db = s1b / sw; // mu - c_p
		const float qr = s2r / sw, qg = s2g / sw, qb = s2b / sw;
		const float mr = cp.x + dr, mg = cp.y + dg, mb = cp.z + db;
		float vr = qr - dr * dr, vg = qg - dg * dg, vb = qb - db * db;
		vr = vr > 0.f ? vr : 0.f, vg = vg > 0.f ? vg : 0.f, vb = vb > 0.f ? vb : 0.f;
		// fewer than 5 counting taps say nothing about a range; a sum that overflowed gives no range either
		const bool use = taps >= 5 && finite3(make_float4(mr, mg, mb, 0.f)) && finite3(make_float4(qr, qg, qb, 0.f));
		o0 = make_float4(mr, mg, mb, use ? sw : 0.f);
		o1 = make_float4(sqrtf(vr), sqrtf(vg), sqrtf(vb), (float)taps);
	}
	p.bounds[i] = o0;
	p.bounds[p.num_pixels + i] = o1;
}

// The world-vertex table of a scene: blockIdx.y = shape (models only), row first[shape] + j = triangle j's P0, P1, P2 in the
// pre-pass's expressions (frame.hip srt_prepass_kernel: mat_by_vec(transform, pos, 1.0f)), so the rows are the tracer's world
// vertices bit for bit, in array order whatever the acceleration stores.
struct VertexTableParams {
	const srt_shape *shapes;
	const srt_triangle *triangles;
	const uint32_t *first; // per shape of this slab: its first row (one entry more: the end of the last)
	float *rows;
	int32_t num_shapes;
};

__global__ __launch_bounds__(256) void srt_vertex_table_kernel(const VertexTableParams p) {
	const int si = blockIdx.y;
	if (si >= p.num_shapes) return;
	const srt_shape *sh = p.shapes + si;
	if (sh->type != SRT_SHAPE_MODEL) return;
	const srt_model *m = &sh->shape.model;
	const srt_float4 *tm = m->transform;
	const uint32_t room = p.first[si + 1] - p.first[si]; // the model's rows (= num_triangles; never past them)
	const uint32_t n = m->num_triangles < room ? m->num_triangles : room;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
		const srt_triangle *t = p.triangles + (m->triangle_index + j);
		float *w = p.rows + (size_t)(p.first[si] + j) * 9;
		for (int k = 0; k < 3; k++) {
			const srt_float3 &v = t->vertices[k].pos;
			w[3 * k + 0] = ((tm[0].x * v.x + tm[1].x * v.y) + tm[2].x * v.z) + tm[3].x * 1.0f;
			w[3 * k + 1] = ((tm[0].y * v.x + tm[1].y * v.y) + tm[2].y * v.z) + tm[3].y * 1.0f;
			w[3 * k + 2] = ((tm[0].z * v.x + tm[1].z * v.y) + tm[2].z * v.z) + tm[3].z * 1.0f;
		}
	}
}

// set offsets, in floats: {colour, count} float4, {m1, m2} float2, guide 2 float4
size_t off_m(size_t px) { return px * 4; }
size_t off_guide(size_t px) { return px * 6; }
size_t set_floats(size_t px) { return px * 14; }

bool same_camera(const srt_render_data &a, const srt_render_data &b) {
	return memcmp(a.camera_to_world, b.camera_to_world, sizeof a.camera_to_world) == 0 &&
	       memcmp(&a.aspect_ratio, &b.aspect_ratio, sizeof(float)) == 0 && memcmp(&a.fov_scale, &b.fov_scale, sizeof(float)) == 0;
}

// the adjugate inverse of m (m[row][col]) in double; false when singular or not finite
bool inv3(const double m[3][3], double out[3][3]) {
	const double a = m[1][1] * m[2][2] - m[1][2] * m[2][1], b = m[1][2] * m[2][0] - m[1][0] * m[2][2], d = m[1][0] * m[2][1] - m[1][1] * m[2][0];
	const double det = m[0][0] * a + m[0][1] * b + m[0][2] * d;
	if (!(det != 0.0) || !std::isfinite(det)) return false;
	out[0][0] = a / det, out[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, out[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
	out[1][0] = b / det, out[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, out[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
	out[2][0] = d / det, out[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, out[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
	for (int r = 0; r < 3; r++)
		for (int c = 0; c < 3; c++)
			if (!std::isfinite(out[r][c])) return false;
	return true;
}

// R^-1 of the camera's upper 3x3 (columns camera_to_world[0..2]): inv3, rounded to float, row-major; false when singular
// or a float is not finite
bool invert_rotation(const srt_render_data &rd, float out[9]) {
	double m[3][3], inv[3][3]; // m[row][col]
	const srt_float4 *c = rd.camera_to_world;
	for (int k = 0; k < 3; k++) m[0][k] = c[k].x, m[1][k] = c[k].y, m[2][k] = c[k].z;
	if (!inv3(m, inv)) return false;
	for (int k = 0; k < 9; k++) {
		out[k] = (float)inv[k / 3][k % 3];
		if (!std::isfinite(out[k])) return false;
	}
	return true;
}

// ---- object motion: the per-shape table (host, double) ----------------------------------------------------------------

struct SceneView { // one scene as srt_update_scene received it
	const srt_shape *shapes;
	size_t n_shapes;
	const void *tris, *mats, *scene;
	size_t tri_bytes, mat_bytes;
};

// srt_tracer::scene_bytes: four sizes, then the shapes, triangles, materials and the scene data
bool view_of(const std::vector<uint8_t> &bytes, SceneView &v) {
	if (bytes.size() < 32) return false;
	size_t nb[4];
	memcpy(nb, bytes.data(), 32);
	const uint8_t *b = bytes.data() + 32;
	v.shapes = reinterpret_cast<const srt_shape *>(b);
	v.n_shapes = nb[0] / sizeof(srt_shape);
	v.tris = b + nb[0], v.tri_bytes = nb[1];
	v.mats = b + nb[0] + nb[1], v.mat_bytes = nb[2];
	v.scene = b + nb[0] + nb[1] + nb[2];
	return true;
}

// n rows of SRT_MOTION_WORDS words: `state` and the identity maps
void identity_rows(uint32_t *rows, size_t n, uint32_t state) {
	const float f[21] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
	for (size_t k = 0; k < n; k++) {
		uint32_t *row = rows + k * SRT_MOTION_WORDS;
		row[0] = state;
		memcpy(row + 1, f, sizeof f);
	}
}

// Xh = lin Xc + tr and the normal map nrm, rounded to float; false when a float is not finite
bool store_row(uint32_t *row, const double lin[3][3], const double tr[3], const double nrm[3][3]) {
	float f[21];
	for (int r = 0; r < 3; r++) {
		for (int c = 0; c < 3; c++) f[4 * r + c] = (float)lin[r][c], f[12 + 3 * r + c] = (float)nrm[r][c];
		f[4 * r + 3] = (float)tr[r];
	}
	for (int k = 0; k < 21; k++)
		if (!std::isfinite(f[k])) return false;
	row[0] = SRT_MOTION_MOVED;
	memcpy(row + 1, f, sizeof f);
	return true;
}

bool sphere_row(const srt_sphere &h, const srt_sphere &c, uint32_t *row) {
	const double rh = h.radius, rc = c.radius;
	if (!(rh > 0.0) || !(rc > 0.0) || !std::isfinite(rh) || !std::isfinite(rc)) return false;
	const double s = rh / rc, ph[3] = {h.position.x, h.position.y, h.position.z}, pc[3] = {c.position.x, c.position.y, c.position.z};
	double lin[3][3] = {{s, 0, 0}, {0, s, 0}, {0, 0, s}}, nrm[3][3] = {{rc / rh, 0, 0}, {0, rc / rh, 0}, {0, 0, rc / rh}}, tr[3];
	for (int k = 0; k < 3; k++) tr[k] = ph[k] - s * pc[k];
	return store_row(row, lin, tr, nrm);
}

bool plane_row(const srt_plane &h, const srt_plane &c, uint32_t *row) {
	double u[3] = {h.normal.x, h.normal.y, h.normal.z}, v[3] = {c.normal.x, c.normal.y, c.normal.z};
	const double lu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), lv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	if (!(lu > 0.0) || !(lv > 0.0) || !std::isfinite(lu) || !std::isfinite(lv)) return false;
	for (int k = 0; k < 3; k++) u[k] /= lu, v[k] /= lv;
	const double k3[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
	const double cs = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
	if (!(cs > -1.0 + 1e-12)) return false;
	const double K[3][3] = {{0, -k3[2], k3[1]}, {k3[2], 0, -k3[0]}, {-k3[1], k3[0], 0}};
	double R[3][3], Rt[3][3], tr[3]; // R: history -> current
	for (int r = 0; r < 3; r++)
		for (int q = 0; q < 3; q++) {
			double k2 = 0.0;
			for (int j = 0; j < 3; j++) k2 += K[r][j] * K[j][q];
			R[r][q] = (r == q ? 1.0 : 0.0) + K[r][q] + k2 / (1.0 + cs);
		}
	for (int r = 0; r < 3; r++)
		for (int q = 0; q < 3; q++) Rt[r][q] = R[q][r];
	const double ph[3] = {h.position.x, h.position.y, h.position.z}, pc[3] = {c.position.x, c.position.y, c.position.z};
	for (int r = 0; r < 3; r++) tr[r] = ph[r] - (Rt[r][0] * pc[0] + Rt[r][1] * pc[1] + Rt[r][2] * pc[2]);
	return store_row(row, Rt, tr, Rt);
}

// the affine part of `transform` (columns 0..2 and the translation, as the kernels' mat_by_vec reads it)
bool model_row(const srt_model &h, const srt_model &c, uint32_t *row) {
	double Lh[3][3], Lc[3][3], Lci[3][3], Lhi[3][3], lin[3][3], fwd[3][3], nrm[3][3], tr[3];
	for (int k = 0; k < 3; k++) {
		Lh[0][k] = h.transform[k].x, Lh[1][k] = h.transform[k].y, Lh[2][k] = h.transform[k].z;
		Lc[0][k] = c.transform[k].x, Lc[1][k] = c.transform[k].y, Lc[2][k] = c.transform[k].z;
	}
	const double th[3] = {h.transform[3].x, h.transform[3].y, h.transform[3].z}, tc[3] = {c.transform[3].x, c.transform[3].y, c.transform[3].z};
	for (int k = 0; k < 3; k++)
		if (!std::isfinite(th[k]) || !std::isfinite(tc[k])) return false;
	if (!inv3(Lc, Lci) || !inv3(Lh, Lhi)) return false;
	for (int r = 0; r < 3; r++)
		for (int q = 0; q < 3; q++) {
			lin[r][q] = (Lh[r][0] * Lci[0][q] + Lh[r][1] * Lci[1][q]) + Lh[r][2] * Lci[2][q]; // current -> history
			fwd[r][q] = (Lc[r][0] * Lhi[0][q] + Lc[r][1] * Lhi[1][q]) + Lc[r][2] * Lhi[2][q]; // history -> current
		}
	for (int r = 0; r < 3; r++) {
		tr[r] = th[r] - ((lin[r][0] * tc[0] + lin[r][1] * tc[1]) + lin[r][2] * tc[2]);
		for (int q = 0; q < 3; q++) nrm[r][q] = fwd[q][r];
	}
	return store_row(row, lin, tr, nrm);
}

// the rules of include/srt_abi.h: false = drop the history; else `table` gets SRT_MOTION_WORDS words per shape
// `deform` (per-triangle motion): the triangle arrays need only have the same count; a model whose range differs in a byte
// is DEFORMED {state, its first row in the vertex tables, zeros}, bytes outside every range are not compared
bool motion_table(const SceneView &h, const SceneView &c, uint32_t *table, bool *any_moved, bool deform, bool *any_deformed) {
	*any_moved = false;
	*any_deformed = false;
	if (h.n_shapes != c.n_shapes || h.tri_bytes != c.tri_bytes || h.mat_bytes != c.mat_bytes) return false;
	if (memcmp(h.scene, c.scene, sizeof(srt_scene_data)) != 0) return false;
	if (h.mat_bytes && memcmp(h.mats, c.mats, h.mat_bytes) != 0) return false;
	if (!deform && h.tri_bytes && memcmp(h.tris, c.tris, h.tri_bytes) != 0) return false;
	for (size_t k = 0; k < c.n_shapes; k++) {
		const srt_shape &a = h.shapes[k], &b = c.shapes[k];
		if (a.type != b.type || a.material != b.material) return false;
		if (a.type == SRT_SHAPE_MODEL) {
			const srt_model &ma = a.shape.model, &mb = b.shape.model;
			// (bounding_min / bounding_max are the world box of the transformed vertices: they move with the transform)
			if (ma.triangle_index != mb.triangle_index || ma.num_triangles != mb.num_triangles) return false;
			// (a range outside the array: srt_update_scene refuses such a scene)
			if (deform && ((uint64_t)mb.triangle_index + mb.num_triangles) * sizeof(srt_triangle) > c.tri_bytes) return false;
		}
	}
	uint64_t first_row = 0;
	for (size_t k = 0; k < c.n_shapes; k++) {
		const srt_shape &a = h.shapes[k], &b = c.shapes[k];
		uint32_t *row = table + k * SRT_MOTION_WORDS;
		if (deform && a.type == SRT_SHAPE_MODEL) {
			const srt_model &mb = b.shape.model;
			const size_t off = (size_t)mb.triangle_index * sizeof(srt_triangle), len = (size_t)mb.num_triangles * sizeof(srt_triangle);
			const uint64_t row0 = first_row;
			first_row += mb.num_triangles;
			if (first_row > 0xffffffffull) return false;
			if (len && memcmp(static_cast<const uint8_t *>(h.tris) + off, static_cast<const uint8_t *>(c.tris) + off, len) != 0) {
				memset(row, 0, SRT_MOTION_WORDS * sizeof(uint32_t));
				row[0] = SRT_MOTION_DEFORMED;
				row[1] = (uint32_t)row0;
				*any_moved = true;
				*any_deformed = true;
				continue;
			}
		}
		if (memcmp(&a, &b, sizeof a) == 0) {
			identity_rows(row, 1, SRT_MOTION_STATIC);
			continue;
		}
		bool ok = false;
		if (a.type == SRT_SHAPE_SPHERE) ok = sphere_row(a.shape.sphere, b.shape.sphere, row);
		else if (a.type == SRT_SHAPE_PLANE) ok = plane_row(a.shape.plane, b.shape.plane, row);
		else if (a.type == SRT_SHAPE_MODEL) ok = model_row(a.shape.model, b.shape.model, row);
		if (!ok) identity_rows(row, 1, SRT_MOTION_NO_HISTORY);
		*any_moved = true;
	}
	return true;
}

// every shape of the current scene STATIC (after a commit, or without a history)
void static_table(srt_tracer *t) {
	SceneView v;
	const size_t n = view_of(t->scene_bytes, v) ? v.n_shapes : 0;
	t->om_table.resize(n * SRT_MOTION_WORDS);
	identity_rows(t->om_table.data(), n, SRT_MOTION_STATIC);
	t->om_any_moved = false;
	t->om_any_deformed = false;
}

// per-triangle motion: the rows of scene `bytes` (vm_first, on the host and on the device) and room for both tables. A
// table that had to grow holds nothing (the history it belonged to is dropped with the triangle count)
int vertex_layout(srt_tracer *t, const std::vector<uint8_t> &bytes) {
	SceneView v;
	const size_t n = view_of(bytes, v) ? v.n_shapes : 0;
	std::vector<uint32_t> first(n + 1, 0u);
	uint64_t rows = 0;
	for (size_t k = 0; k < n; k++) {
		first[k] = (uint32_t)rows;
		if (v.shapes[k].type == SRT_SHAPE_MODEL) rows += v.shapes[k].shape.model.num_triangles;
		if (rows > 0xffffffffull) return fail(t, SRT_ERR_INVALID, "per-triangle motion: more than 2^32 - 1 instance triangles");
	}
	first[n] = (uint32_t)rows;
	if (first == t->vm_first && t->vm_first_dev.ptr && t->vm_rows[0].cap >= rows * 9 && t->vm_rows[1].cap >= rows * 9) return SRT_OK; // the layout stands
	t->vm_first.swap(first);
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // a set-up still on the stream reads the old rows
	SRT_HIP(t, t->vm_first_dev.reserve(n + 1));
	for (int k = 0; k < 2; k++) {
		const float *before = t->vm_rows[k].ptr;
		SRT_HIP(t, t->vm_rows[k].reserve((size_t)rows * 9));
		if (t->vm_rows[k].ptr != before) t->vm_ver[k] = 0;
	}
	SRT_HIP(t, hipMemcpyAsync(t->vm_first_dev.ptr, t->vm_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

// one instantiation's launch: of the four structs it passes on those its kernel takes
template <int MOTION, bool ILLUM, bool CLAMP>
void launch_variant(hipStream_t stream, dim3 grid, const TemporalParams &p, const MotionParams &mp, const VertexParams &vp, const ClampParams &cp) {
	const SetupArgs<MOTION, CLAMP> a = {p, mp, vp, cp};
	hipLaunchKernelGGL((srt_temporal_kernel<MOTION, ILLUM, CLAMP>), grid, dim3(256), 0, stream, a);
}

using SetupLaunch = decltype(&launch_variant<0, false, false>);
const SetupLaunch setup_launch[3][2][2] = { // [motion_level][illum][clamp]
	{{launch_variant<0, false, false>, launch_variant<0, false, true>}, {launch_variant<0, true, false>, launch_variant<0, true, true>}},
	{{launch_variant<1, false, false>, launch_variant<1, false, true>}, {launch_variant<1, true, false>, launch_variant<1, true, true>}},
	{{launch_variant<2, false, false>, launch_variant<2, false, true>}, {launch_variant<2, true, false>, launch_variant<2, true, true>}},
};

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
	p.limit = (float)t->dn.tp.history_limit;
	p.normal_threshold = t->dn.tp.normal_threshold;
	p.depth_threshold = t->dn.tp.depth_threshold;
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
	const SetupPlan plan = plan_setup(t->dn, t->tp_valid, t->om_any_moved, t->om_any_deformed);
	p.mode = TP_NONE;
	if (t->tp_valid) {
		if (same_camera(rd, rh)) p.mode = (plan.motion_level == 0 || invert_rotation(rh, p.rinv)) ? TP_IDENTITY : TP_NONE; // a moved shape projects
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
	MotionParams mp = {};
	VertexParams vp = {};
	ClampParams cp = {};
	if (plan.motion_level >= 1) {
		mp.ids = t->om_ids[t->om_cur].ptr;
		mp.h_ids = t->om_ids[1 - t->om_cur].ptr;
		mp.table = t->om_table_dev.ptr;
		mp.n_shapes = (uint32_t)(t->om_table.size() / SRT_MOTION_WORDS);
	}
	if (plan.motion_level == 2) { // a deformed model: its pixels look their triangles up in the two vertex tables
		vp.tris = t->vm_tri[t->om_cur].ptr;
		vp.rows = t->vm_rows[t->om_cur].ptr;
		vp.h_rows = t->vm_rows[1 - t->om_cur].ptr;
		vp.first = t->vm_first_dev.ptr;
	}
	if (plan.clamp) {
		BoundsParams bp;
		bp.width = t->width;
		bp.height = t->height;
		bp.num_pixels = (uint32_t)px;
		bp.T = p.T;
		bp.F = p.F;
		bp.sigma_n = t->dn.p.sigma_normal;
		bp.sigma_z = t->dn.p.sigma_depth;
		bp.inv_sigma_a2 = plan_filter(t->dn).inv_sigma_a2;
		bp.canvas = p.canvas;
		bp.normal_depth = p.normal_depth;
		bp.albedo_hits = p.albedo_hits;
		bp.bounds = reinterpret_cast<float4 *>(t->tp_bounds.ptr);
		hipLaunchKernelGGL(srt_temporal_bounds_kernel, grid, dim3(256), 0, t->stream, bp);
		SRT_HIP(t, hipGetLastError());
		t->tp_bounds_ran = true;
		cp.bounds = bp.bounds;
		cp.num_pixels = bp.num_pixels;
		cp.gamma = t->dn.clamp_gamma;
	}
	setup_launch[plan.motion_level][plan.illum][plan.clamp](t->stream, grid, p, mp, vp, cp);
	SRT_HIP(t, hipGetLastError());
	t->last_setup = plan;
	return SRT_OK;
}

// the key of a staging set made now
StagingKey key_now(const srt_tracer *t) { return staging_key(t->dn, t->tp_valid, t->om_any_moved, t->om_any_deformed, t->dn_serial); }

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
	t->tp_staged.reset();
}

int srt_temporal_setup(srt_tracer *t, float4 *col, uint32_t *argb, TemporalStaged *staged) {
	const int rc = launch_setup(t, col, argb);
	if (rc) return rc;
	const size_t px = full_pixels(t);
	const float *stage = t->tp_set[1 - t->tp_cur].ptr;
	staged->guide = reinterpret_cast<const float4 *>(stage + off_guide(px));
	staged->cc = reinterpret_cast<const float4 *>(stage);
	staged->m = reinterpret_cast<const float2 *>(stage + off_m(px));
	t->tp_staged = key_now(t);
	return SRT_OK;
}

int srt_temporal_commit(srt_tracer *t) {
	if (!t->dn.on || !t->dn.temporal || t->dn_T == 0 || full_pixels(t) == 0) return SRT_OK; // nothing traced: the history stays
	if (!(t->tp_staged == key_now(t))) {
		// no filter since the last trace, or one whose staging launches were not those of the settings now: the set is made here. With the
		// history feedback on that is the filter's own front, pass 1 included (denoise.hip), so that the history never depends on whether a filter ran
		const int rc = plan_filter(t->dn).feedback ? srt_denoise_feedback_front(t) : launch_setup(t, nullptr, nullptr);
		if (rc) return rc;
	}
	t->tp_cur = 1 - t->tp_cur;
	t->tp_cam = t->dn_cam;
	t->tp_valid = true;
	t->tp_staged.reset();
	if (t->dn.object_motion) {
		if (t->om_mixed) { // traced with more than one scene: no single set of maps leads back to this frame
			srt_temporal_drop(t);
		} else {
			t->om_cur = 1 - t->om_cur; // the frame's shape indices become the history's (with them its triangle indices and vertex table)
			t->om_hist_scene = t->scene_bytes;
		}
		static_table(t);
	}
	return SRT_OK;
}

int srt_motion_update_scene(srt_tracer *t, const std::vector<uint8_t> &bytes, int rc) {
	if (rc != SRT_OK || bytes.empty()) {
		srt_temporal_drop(t);
		return SRT_OK;
	}
	if (t->dn_T > 0 && bytes != t->scene_bytes) t->om_mixed = true; // samples of the old scene are on the canvas
	if (t->dn.vertex_motion && bytes != t->scene_bytes) t->vm_scene_ver++;      // the next feature pass writes this scene's vertex table
	SceneView h, c;
	view_of(bytes, c);
	t->om_table.assign(c.n_shapes * SRT_MOTION_WORDS, 0u);
	t->om_any_moved = false;
	t->om_any_deformed = false;
	if (t->tp_valid && !(view_of(t->om_hist_scene, h) && motion_table(h, c, t->om_table.data(), &t->om_any_moved, t->dn.vertex_motion, &t->om_any_deformed))) srt_temporal_drop(t);
	if (!t->tp_valid) {
		identity_rows(t->om_table.data(), c.n_shapes, SRT_MOTION_STATIC);
		t->om_any_moved = false;
		t->om_any_deformed = false;
	}
	if (t->dn.vertex_motion) {
		const int vrc = vertex_layout(t, bytes);
		if (vrc) return vrc;
	}
	if (t->om_any_moved) { // with the scene upload; a set-up still running on the stream reads the old table first
		SRT_HIP(t, hipSetDevice(t->device));
		SRT_HIP(t, t->om_table_dev.reserve(t->om_table.size()));
		SRT_HIP(t, hipMemcpyAsync(t->om_table_dev.ptr, t->om_table.data(), t->om_table.size() * 4, hipMemcpyHostToDevice, t->stream));
		SRT_HIP(t, hipStreamSynchronize(t->stream));
	}
	return SRT_OK;
}

int srt_vertex_table_sync(srt_tracer *t) {
	const int cur = t->om_cur;
	if (t->vm_ver[cur] == t->vm_scene_ver) return SRT_OK; // this table already holds the scene being traced
	const size_t n_shapes = t->vm_first.empty() ? 0 : t->vm_first.size() - 1;
	const uint32_t rows = n_shapes ? t->vm_first[n_shapes] : 0u;
	// (the layout is that of the last srt_update_scene's arrays; when that call failed the device holds another scene: no table)
	if (rows && t->scene_set && (size_t)t->sd.num_shapes == n_shapes && t->vm_rows[cur].cap >= (size_t)rows * 9) {
		uint32_t max_tris = 0;
		for (size_t k = 0; k < n_shapes; k++) max_tris = std::max(max_tris, t->vm_first[k + 1] - t->vm_first[k]);
		unsigned gx = (max_tris + 255u) / 256u;
		if (gx > 4096u) gx = 4096u;
		for (size_t base = 0; base < n_shapes; base += 65535) { // blockIdx.y = shape index, in slabs as the pre-pass
			VertexTableParams vt;
			vt.shapes = t->shapes.ptr + base;
			vt.triangles = t->triangles.ptr;
			vt.first = t->vm_first_dev.ptr + base;
			vt.rows = t->vm_rows[cur].ptr;
			const size_t cnt = n_shapes - base;
			vt.num_shapes = (int32_t)(cnt > 65535 ? 65535 : cnt);
			hipLaunchKernelGGL(srt_vertex_table_kernel, dim3(gx, (unsigned)vt.num_shapes), dim3(256), 0, t->stream, vt);
		}
		SRT_HIP(t, hipGetLastError());
	}
	t->vm_ver[cur] = t->vm_scene_ver;
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
		if (t->dn.temporal) srt_temporal_drop(t);
		t->dn.temporal_off(); // with the modes of the set-up and object motion
		return SRT_OK;
	}
	if (!params_ok(*params))
		return fail(t, SRT_ERR_INVALID, "srt_set_denoise_temporal: history_limit 1..2^20, normal_threshold -1..1, depth_threshold finite and > 0, reserved 0");
	if (!t->dn.on) return fail(t, SRT_ERR_STATE, "srt_set_denoise_temporal: the denoiser is off (srt_set_denoise)");
	if (t->world > 1) return fail(t, SRT_ERR_STATE, "srt_set_denoise_temporal: not available on a partitioned handle (srt_set_partition world > 1)");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	for (int k = 0; k < 2; k++) SRT_HIP(t, t->tp_set[k].reserve(set_floats(px)));
	if (!t->dn.temporal) srt_temporal_drop(t);
	t->dn.tp = *params;
	t->dn.temporal = true;
	return SRT_OK;
}

int srt_set_denoise_history_illumination(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	if (enable && !t->dn.temporal)
		return fail(t, SRT_ERR_STATE, "srt_set_denoise_history_illumination: temporal reprojection is off (srt_set_denoise_temporal)");
	t->dn.illum = enable != 0;
	return SRT_OK;
}

int srt_last_setup_history_illumination(srt_tracer *t) { return t && t->last_setup.illum ? 1 : 0; }

int srt_set_denoise_history_clamp(srt_tracer *t, float gamma) {
	if (!t) return SRT_ERR_INVALID;
	if (!(gamma == 0.0f) && !(std::isfinite(gamma) && gamma > 0.0f && gamma <= 64.0f))
		return fail(t, SRT_ERR_INVALID, "srt_set_denoise_history_clamp: gamma 0 (off) or finite in (0, 64]");
	if (gamma == 0.0f) gamma = 0.0f; // (-0: off)
	if (gamma > 0.0f) {
		if (!t->dn.temporal) return fail(t, SRT_ERR_STATE, "srt_set_denoise_history_clamp: temporal reprojection is off (srt_set_denoise_temporal)");
		SRT_HIP(t, hipSetDevice(t->device));
		SRT_HIP(t, t->tp_bounds.reserve(full_pixels(t) * 8)); // the two planes, on the first enable
	}
	t->dn.clamp_gamma = gamma;
	return SRT_OK;
}

int srt_last_setup_history_clamp(srt_tracer *t) { return t && t->last_setup.clamp ? 1 : 0; }

int srt_set_denoise_history_feedback(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	if (enable && !t->dn.temporal)
		return fail(t, SRT_ERR_STATE, "srt_set_denoise_history_feedback: temporal reprojection is off (srt_set_denoise_temporal)");
	t->dn.feedback = enable != 0;
	return SRT_OK;
}

int srt_last_filter_history_feedback(srt_tracer *t) { return t && t->last_filter.feedback ? 1 : 0; }

int srt_read_denoise_history_bounds(srt_tracer *t, float *mean_weight, float *sigma_taps) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->tp_bounds.ptr || !t->tp_bounds_ran) return fail(t, SRT_ERR_STATE, "srt_read_denoise_history_bounds: the history clamp has never run on this handle (srt_set_denoise_history_clamp)");
	const size_t px = full_pixels(t);
	SRT_HIP(t, hipSetDevice(t->device));
	if (mean_weight) SRT_HIP(t, hipMemcpyAsync(mean_weight, t->tp_bounds.ptr, px * 16, hipMemcpyDeviceToHost, t->stream));
	if (sigma_taps) SRT_HIP(t, hipMemcpyAsync(sigma_taps, t->tp_bounds.ptr + px * 4, px * 16, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_set_denoise_object_motion(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	if (!enable) {
		if (t->dn.object_motion) srt_temporal_drop(t);
		t->dn.object_motion = t->dn.vertex_motion = false; // per-triangle motion is a part of it
		return SRT_OK;
	}
	if (!t->dn.temporal) return fail(t, SRT_ERR_STATE, "srt_set_denoise_object_motion: temporal reprojection is off (srt_set_denoise_temporal)");
	if (t->dn.object_motion) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	for (int k = 0; k < 2; k++) {
		SRT_HIP(t, t->om_ids[k].reserve(px));
		SRT_HIP(t, hipMemsetAsync(t->om_ids[k].ptr, 0xff, px * 4, t->stream));
	}
	srt_temporal_drop(t);
	t->dn.object_motion = true;
	t->om_mixed = t->dn_T > 0; // what is on the canvas was traced without shape indices
	static_table(t);
	return SRT_OK;
}

int srt_read_denoise_shape_ids(srt_tracer *t, uint32_t *current, uint32_t *history) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->om_ids[0].ptr) return fail(t, SRT_ERR_STATE, "srt_read_denoise_shape_ids: object motion was never enabled (srt_set_denoise_object_motion)");
	const size_t px = full_pixels(t);
	SRT_HIP(t, hipSetDevice(t->device));
	if (current) SRT_HIP(t, hipMemcpyAsync(current, t->om_ids[t->om_cur].ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
	if (history) {
		if (t->tp_valid) SRT_HIP(t, hipMemcpyAsync(history, t->om_ids[1 - t->om_cur].ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
		else memset(history, 0xff, px * 4);
	}
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_read_denoise_motion(srt_tracer *t, uint32_t *table, size_t capacity_shapes, size_t *n_shapes, int *any_moved) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->dn.object_motion) return fail(t, SRT_ERR_STATE, "srt_read_denoise_motion: object motion is off (srt_set_denoise_object_motion)");
	const size_t n = t->om_table.size() / SRT_MOTION_WORDS;
	if (n_shapes) *n_shapes = n;
	if (any_moved) *any_moved = (t->tp_valid && t->om_any_moved) ? 1 : 0;
	if (table) {
		if (capacity_shapes < n) return fail(t, SRT_ERR_INVALID, "srt_read_denoise_motion: the table has more shapes than capacity_shapes");
		if (n) memcpy(table, t->om_table.data(), n * SRT_MOTION_WORDS * 4);
		if (!t->tp_valid) identity_rows(table, n, SRT_MOTION_STATIC);
	}
	return SRT_OK;
}

// srt_motion_table_host (deform false) and srt_motion_table_deform_host (true)
static int motion_table_host(bool deform, const srt_shape *h_shapes, size_t h_n_shapes, const srt_triangle *h_triangles, size_t h_n_triangles,
                             const srt_material *h_materials, size_t h_n_materials, const srt_scene_data *h_scene,
                             const srt_shape *c_shapes, size_t c_n_shapes, const srt_triangle *c_triangles, size_t c_n_triangles,
                             const srt_material *c_materials, size_t c_n_materials, const srt_scene_data *c_scene, uint32_t *table, int *keep) {
	if (!h_scene || !c_scene || !keep || (c_n_shapes && !table)) return SRT_ERR_INVALID;
	if ((h_n_shapes && !h_shapes) || (c_n_shapes && !c_shapes) || (h_n_triangles && !h_triangles) || (c_n_triangles && !c_triangles) ||
	    (h_n_materials && !h_materials) || (c_n_materials && !c_materials))
		return SRT_ERR_INVALID;
	const SceneView h = {h_shapes, h_n_shapes, h_triangles, h_materials, h_scene, h_n_triangles * sizeof(srt_triangle), h_n_materials * sizeof(srt_material)};
	const SceneView c = {c_shapes, c_n_shapes, c_triangles, c_materials, c_scene, c_n_triangles * sizeof(srt_triangle), c_n_materials * sizeof(srt_material)};
	bool any = false, any_deformed = false;
	try {
		std::vector<uint32_t> rows(c_n_shapes * SRT_MOTION_WORDS);
		*keep = motion_table(h, c, rows.data(), &any, deform, &any_deformed) ? 1 : 0;
		if (*keep && !rows.empty()) memcpy(table, rows.data(), rows.size() * 4);
	} catch (...) {
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_motion_table_host(const srt_shape *h_shapes, size_t h_n_shapes, const srt_triangle *h_triangles, size_t h_n_triangles,
                          const srt_material *h_materials, size_t h_n_materials, const srt_scene_data *h_scene,
                          const srt_shape *c_shapes, size_t c_n_shapes, const srt_triangle *c_triangles, size_t c_n_triangles,
                          const srt_material *c_materials, size_t c_n_materials, const srt_scene_data *c_scene, uint32_t *table, int *keep) {
	return motion_table_host(false, h_shapes, h_n_shapes, h_triangles, h_n_triangles, h_materials, h_n_materials, h_scene,
	                         c_shapes, c_n_shapes, c_triangles, c_n_triangles, c_materials, c_n_materials, c_scene, table, keep);
}

int srt_motion_table_deform_host(const srt_shape *h_shapes, size_t h_n_shapes, const srt_triangle *h_triangles, size_t h_n_triangles,
                                 const srt_material *h_materials, size_t h_n_materials, const srt_scene_data *h_scene,
                                 const srt_shape *c_shapes, size_t c_n_shapes, const srt_triangle *c_triangles, size_t c_n_triangles,
                                 const srt_material *c_materials, size_t c_n_materials, const srt_scene_data *c_scene, uint32_t *table, int *keep) {
	return motion_table_host(true, h_shapes, h_n_shapes, h_triangles, h_n_triangles, h_materials, h_n_materials, h_scene,
	                         c_shapes, c_n_shapes, c_triangles, c_n_triangles, c_materials, c_n_materials, c_scene, table, keep);
}


int srt_set_denoise_vertex_motion(srt_tracer *t, int enable) {
	if (!t) return SRT_ERR_INVALID;
	if (!enable) {
		if (t->dn.vertex_motion) srt_temporal_drop(t);
		t->dn.vertex_motion = false;
		return SRT_OK;
	}
	if (!t->dn.object_motion) return fail(t, SRT_ERR_STATE, "srt_set_denoise_vertex_motion: object motion is off (srt_set_denoise_object_motion)");
	if (t->dn.vertex_motion) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t px = full_pixels(t);
	for (int k = 0; k < 2; k++) {
		SRT_HIP(t, t->vm_tri[k].reserve(px));
		SRT_HIP(t, hipMemsetAsync(t->vm_tri[k].ptr, 0xff, px * 4, t->stream));
	}
	const int rc = vertex_layout(t, t->scene_bytes);
	if (rc) return rc;
	t->vm_scene_ver++; // whatever the tables hold, the next feature pass writes the current scene's
	srt_temporal_drop(t);
	t->dn.vertex_motion = true;
	t->om_mixed = t->dn_T > 0; // what is on the canvas was traced without triangle indices
	static_table(t);
	return SRT_OK;
}

int srt_read_denoise_triangle_ids(srt_tracer *t, uint32_t *current, uint32_t *history) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->vm_tri[0].ptr) return fail(t, SRT_ERR_STATE, "srt_read_denoise_triangle_ids: per-triangle motion was never enabled (srt_set_denoise_vertex_motion)");
	const size_t px = full_pixels(t);
	SRT_HIP(t, hipSetDevice(t->device));
	if (current) SRT_HIP(t, hipMemcpyAsync(current, t->vm_tri[t->om_cur].ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
	if (history) {
		if (t->tp_valid) SRT_HIP(t, hipMemcpyAsync(history, t->vm_tri[1 - t->om_cur].ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
		else memset(history, 0xff, px * 4);
	}
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_read_denoise_vertex_tables(srt_tracer *t, float *current, float *history, size_t cap_rows, size_t *n_rows) {
	if (!t) return SRT_ERR_INVALID;
	if (!t->vm_tri[0].ptr) return fail(t, SRT_ERR_STATE, "srt_read_denoise_vertex_tables: per-triangle motion was never enabled (srt_set_denoise_vertex_motion)");
	const size_t n = t->vm_first.empty() ? 0 : t->vm_first.back();
	if (n_rows) *n_rows = n;
	if (!current && !history) return SRT_OK;
	if (cap_rows < n) return fail(t, SRT_ERR_INVALID, "srt_read_denoise_vertex_tables: the tables have more rows than cap_rows");
	if (n == 0) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	if (current) SRT_HIP(t, hipMemcpyAsync(current, t->vm_rows[t->om_cur].ptr, n * 36, hipMemcpyDeviceToHost, t->stream));
	if (history) {
		if (t->tp_valid) SRT_HIP(t, hipMemcpyAsync(history, t->vm_rows[1 - t->om_cur].ptr, n * 36, hipMemcpyDeviceToHost, t->stream));
		else memset(history, 0, n * 36);
	}
	SRT_HIP(t, hipStreamSynchronize(t->stream));
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
