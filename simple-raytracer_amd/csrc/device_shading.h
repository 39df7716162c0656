// device_shading.h -- what a path looks up once its closest hit is known: the sky, the hit's normal and, in the textured
// build, its albedo texel and per-triangle material. Used by the trace and feature kernels (kernels.hip); selftest.hip checks
// powi_uniform.
#ifndef SRT_DEVICE_SHADING_H
#define SRT_DEVICE_SHADING_H

#include "device_intersect.h" // SRT_AS_CONST, bvh_tri_in_model

// Albedo textures: set by kernels_tex.hip alone, which compiles kernels.hip a second time.
#ifndef SRT_TEXTURED
#define SRT_TEXTURED 0
#endif

namespace {

// Manual float bilinear, OpenCL 3.0 §8.2 CLAMP_TO_EDGE + LINEAR, normalized coords
__device__ __forceinline__ f3 sample_sky(const float *__restrict__ sky, int W, int H, float fW, float fH, float s, float t) {
	float fu = s * fW - 0.5f;
	float fv = t * fH - 0.5f;
	float cu = dm_clamp(fu, -1.0f, fW);
	float cv = dm_clamp(fv, -1.0f, fH);
	if (!(cu == cu)) cu = 0.0f;
	if (!(cv == cv)) cv = 0.0f;
	float x0f = __builtin_floorf(cu), y0f = __builtin_floorf(cv);
	float a = fu - x0f, b = fv - y0f;
	int x0 = (int)x0f, y0 = (int)y0f;
	int i0 = min(max(x0, 0), W - 1), i1 = min(max(x0 + 1, 0), W - 1);
	int j0 = min(max(y0, 0), H - 1), j1 = min(max(y0 + 1, 0), H - 1);
	const float4 *img = reinterpret_cast<const float4 *>(sky);
	float4 T00 = img[(size_t)j0 * W + i0];
	float4 T10 = img[(size_t)j0 * W + i1];
	float4 T01 = img[(size_t)j1 * W + i0];
	float4 T11 = img[(size_t)j1 * W + i1];
	float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	return mk(dm_bilinear(w00, T00.x, w10, T10.x, w01, T01.x, w11, T11.x), dm_bilinear(w00, T00.y, w10, T10.y, w01, T01.y, w11, T11.y),
	          dm_bilinear(w00, T00.z, w10, T10.z, w01, T01.z, w11, T11.z));
}

// The launch parameters as they lie in the kernel-argument segment, behind a pointer the compiler cannot see through: what
// is read through it is loaded (scalar loads, scalar-cache hits) where it is used instead of living in SGPRs for the whole
// launch. The persistent loop has far more wave-uniform state than SGPRs; parameters only the sky and the camera rays need
// (sun, image size, camera matrix: ~45 dwords) were being spilled to VGPR lanes and read back with a v_readlane each.
__device__ __forceinline__ const SRT_AS_CONST TraceParams *cold_params() {
	const SRT_AS_CONST TraceParams *kp = (const SRT_AS_CONST TraceParams *)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(kp));
	return kp;
}
#define SRT_COLD(p) (*cold_params())

// dm_powi (detmath.h) for a WAVE-UNIFORM exponent 1 <= n <= 32: the same squarings and products in double, in the same
// order, but the exponent's bits steer scalar branches. Written as in detmath.h the compiler turns the loop's `first ? b :
// r * b` and the conditional squaring into selects on 64-bit values: ~45 v_cndmask per call, in runs (which stall on gfx950),
// for what is four squarings and two products when n = 25.
__device__ __forceinline__ float powi_uniform(float x, int n) {
	uint32_t un = (uint32_t)__builtin_amdgcn_readfirstlane(n);
	double b = (double)x;
	while (!(un & 1u)) { // (n >= 1: there is a set bit) squarings below the lowest set bit
		b = b * b;
		un >>= 1;
	}
	double r = b; // detmath's `first` product
	un >>= 1;
	while (un) {
		b = b * b;
		if (un & 1u) r = r * b;
		un >>= 1;
	}
	return (float)r;
}

// render.cl:380-394
__device__ __forceinline__ f3 sky_box(const TraceParams &p_live, f3 dir) {
	const auto &p = SRT_COLD(p_live);
	f3 sun_dir = mk(p.sd.sun_direction.x, p.sd.sun_direction.y, p.sd.sun_direction.z);
	// dm_powf(x, sun_focus) with its (wave-uniform) choice of path made once on the host
	const float lobe_x = dm_max(dot3(dir, neg(sun_dir)), 0.0f);
	float lobe;
	if (p.sun_focus_int > 0) {
		lobe = powi_uniform(lobe_x, p.sun_focus_int); // dm_powf's x == 1 and NaN cases fall out of the products
	} else {
		lobe = dm_powf(lobe_x, p.sd.sun_focus);
	}
	f3 sun = (mk(p.sd.sun_color.x, p.sd.sun_color.y, p.sd.sun_color.z) * lobe) * p.sd.sun_intensity;
	float u = dm_atan2pif(dir.z, dir.x) * 0.5f + 0.5f;
	float v = dir.y * 0.5f + 0.5f;
	return sample_sky((const float *)p.sky, p.sky_w, p.sky_h, p.f_sky_w, p.f_sky_h, u, v) + sun;
}

// the normal of the hit at `pos`, before the front-face flip: a copy of SHADE_WINNER in srt_trace_kernel (global-memory form)
template <bool HAS_MODELS, bool USE_BVH>
__device__ __forceinline__ f3 winner_normal(const TraceParams &p, int best, uint32_t best_tri, f3 pos) {
	const WinnerRec *__restrict__ wr = p.winners + best;
	const int type = wr->type;
	const f3 wv = mk(wr->vx, wr->vy, wr->vz);
	f3 nrm = wv; // a plane's normal as stored
	if (type == SRT_SHAPE_SPHERE) {
		nrm = div3_by_rcp(pos - wv, wr->w, wr->inv_w);
	} else if (HAS_MODELS && type != SRT_SHAPE_PLANE) {
		const srt_model *__restrict__ m = &p.shapes[best].shape.model;
		const float *__restrict__ w = USE_BVH ? p.bvh_blocks + (size_t)(best_tri >> 2) * 32u + (best_tri & 3u) * SRT_BVH_TRI_FLOATS
		                                      : p.wtris + (size_t)(wr->first_wtri + best_tri) * SRT_WTRI_FLOATS;
		const uint32_t tri_in_model = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
		f3 v0 = mk(w[0], w[1], w[2]);
		f3 e1 = mk(w[3], w[4], w[5]);
		f3 e2 = mk(w[6], w[7], w[8]);
		f3 v2 = pos - v0;
		float d00 = dot3(e1, e1), d01 = dot3(e1, e2), d11 = dot3(e2, e2);
		float d20 = dot3(v2, e1), d21 = dot3(v2, e2);
		float den = d00 * d11 - d01 * d01;
		float w0 = (d11 * d20 - d01 * d21) / den;
		float w1 = (d00 * d21 - d01 * d20) / den;
		float w2 = 1.0f - w0 - w1;
		const srt_triangle *__restrict__ tr = p.triangles + (m->triangle_index + tri_in_model);
		f3 n = (ld3(tr->vertices[0].normal) * w2 + ld3(tr->vertices[1].normal) * w0) + ld3(tr->vertices[2].normal) * w1;
		n = mat_by_vec(m->transform, n, 0.0f);
		nrm = normalize3(n);
	}
	return nrm;
}

// ---- DIFFUSE WAVES (DESIGN.md §5 "Diffuse waves") ----
// The NO_SPEC scene classes' bounce (trace_body.inc SHADE_BOUNCE .. SHADE_OPAQUE) on a lane whose material is PLAIN DIFFUSE --
// metallic threshold 0 and transmittance threshold 0, so `random_bits < 0` makes both draws false for every output of the
// generator -- comes to
//     rough_dir = fma(reflect3(dir, nrm) - random_dir, smoothness, random_dir)
//     dir       = fma(rough_dir - random_dir, +0, random_dir)        mask = mask * mcolor        seed three steps on
// and fma(d, +0, x) is x, bit for bit, when d is finite (d * 0 is then an exact +-0) and x is neither a zero (+0 + -0 is +0: the
// sign of a zero component reaches the plane tests' quotients) nor a NaN (kept out for a plain proof; the sum below refuses it).
// A wave whose shading lanes are ALL plain diffuse and whose operands ALL pass diffuse_operands_ok takes random_dir as it is:
// no draws, no reflect3, no mix3. Any other wave runs the per-lane form as it stands.
__device__ __forceinline__ bool plain_diffuse(float metallic_threshold, float transmittance_threshold) {
	return (dm_f2u(metallic_threshold) | dm_f2u(transmittance_threshold)) == 0u;
}
// The guard, per lane. S = the sum of the ten magnitudes (random_dir, dir, nrm, smoothness) <= 2^20, mn = the smallest
// |random_dir component| > 0.
//   * A NaN or an infinity among the ten makes S NaN or +inf and the compare false. A sum of non-negative floats is at least
//     each term (rounding is monotone), so every magnitude is <= 2^20.
//   * v_min3 skips NaNs, but S has refused them already; mn > 0 so refuses exactly a component of +-0 (a denormal passes: f32
//     denormals are on, and fma(d, 0, x) returns a denormal x unchanged).
//   * d is finite: |dot3(dir, nrm)| <= 3 * 2^40 * (1 + 2^-23)^3 < 2^42; doubled < 2^43; times a component of nrm < 2^63;
//     |reflected_dir| < 2^64; |reflected_dir - random_dir| < 2^65; |rough_dir| < 2^85 + 2^20 < 2^86; |d| < 2^87 < 2^128.
// So the identity holds for every lane the guard admits. (tests/test_diffuse_bounce_host.py restates it in numpy.)
__device__ __forceinline__ bool diffuse_operands_ok(f3 random_dir, f3 dir, f3 nrm, float smoothness) {
	const float rx = dm_fabs(random_dir.x), ry = dm_fabs(random_dir.y), rz = dm_fabs(random_dir.z);
	const float mn = __builtin_fminf(__builtin_fminf(rx, ry), rz);
	const float sm = ((((((((rx + ry) + rz) + dm_fabs(dir.x)) + dm_fabs(dir.y)) + dm_fabs(dir.z)) + dm_fabs(nrm.x)) + dm_fabs(nrm.y)) + dm_fabs(nrm.z)) + dm_fabs(smoothness);
	return mn > 0.0f && sm <= 0x1p20f;
}
// (wave-uniform) the two votes over the lanes that are executing
__device__ __forceinline__ bool diffuse_wave_materials(float metallic_threshold, float transmittance_threshold) {
	return !any64(!plain_diffuse(metallic_threshold, transmittance_threshold));
}
__device__ __forceinline__ bool diffuse_wave_operands(f3 random_dir, f3 dir, f3 nrm, float smoothness) {
	return !any64(!diffuse_operands_ok(random_dir, dir, nrm, smoothness));
}
// The short form: the generator steps over the three material draws (the compiler folds the steps into one multiply-add).
__device__ __forceinline__ void bounce_diffuse_wave(f3 random_dir, f3 mcolor, f3 &dir, f3 &mask, uint32_t &seed) {
	seed = seed * 747796405u + 2891336453u;
	seed = seed * 747796405u + 2891336453u;
	seed = seed * 747796405u + 2891336453u;
	dir = random_dir;
	mask = mask * mcolor;
}
// The per-lane form up to the branch on is_transparent, restated for srt_selftest_diffuse_bounce from the NO_SPEC text of
// trace_body.inc (which the kernels keep as it stands; the oracle tests pin that text, the self-test pins the identity). An
// opaque lane gets its new dir and mask; a transparent one is left with rough_dir, which SHADE_GLASS goes on from.
__device__ __forceinline__ bool bounce_nospec_lane(f3 random_dir, f3 nrm, float smoothness, float metallic, float transmittance, f3 mcolor, f3 &dir, f3 &mask, uint32_t &seed) {
	f3 reflected_dir = reflect3(dir, nrm);
	bool is_metallic, is_transparent;
	is_metallic = bernoulli(metallic, true, seed);
	seed = seed * 747796405u + 2891336453u; // random_bits' state step, its output unused
	is_transparent = bernoulli(transmittance, true, seed);
	f3 rough_dir = mix3(random_dir, reflected_dir, smoothness);
	if (!is_transparent) {
		dir = mix3(random_dir, rough_dir, is_metallic ? 1.0f : 0.0f);
		mask = mask * mcolor;
	} else {
		dir = rough_dir;
	}
	return is_transparent;
}

#if SRT_TEXTURED
// ---- albedo textures: include/srt_abi.h states these rules; tests/texture_ref.py copies the expressions below ----
__device__ __forceinline__ int tex_wrap(int x, int n) { // x mod n, never negative
	const int m = x % n;
	return m < 0 ? m + n : m;
}
// The sampler, addressing REPEAT. (u, v) already scaled.
//   NEAREST: pu = u * fW, pv = v * fH; texel (floor(pu) mod W, floor(pv) mod H) as stored.
//   LINEAR:  fu = u * fW - 0.5, fv = v * fH - 0.5; x0 = floor(fu), y0 = floor(fv); a = fu - x0, b = fv - y0; columns x0 mod W and
//            (x0 + 1) mod W, rows likewise; sample_sky's weights and dm_bilinear.
//   A coordinate (pu, pv / fu, fv) that is NaN, infinite or >= 2^30 in magnitude: texel (0, 0) as stored.
__device__ __forceinline__ f3 sample_texture(const TexParams &tx, int texture, int filter, float u, float v) {
	const TexDesc *__restrict__ d = tx.descs + texture;
	const int W = d->w, H = d->h;
	const float4 *__restrict__ img = reinterpret_cast<const float4 *>(tx.texels) + d->offset;
	float fu = u * d->fw, fv = v * d->fh;
	if (filter == SRT_FILTER_LINEAR) {
		fu = fu - 0.5f;
		fv = fv - 0.5f;
	}
	if (!(dm_fabs(fu) < 0x1p30f && dm_fabs(fv) < 0x1p30f)) {
		const float4 T = img[0];
		return mk(T.x, T.y, T.z);
	}
	const float x0f = __builtin_floorf(fu), y0f = __builtin_floorf(fv);
	const int i0 = tex_wrap((int)x0f, W), j0 = tex_wrap((int)y0f, H);
	if (filter != SRT_FILTER_LINEAR) {
		const float4 T = img[(size_t)j0 * W + i0];
		return mk(T.x, T.y, T.z);
	}
	const float a = fu - x0f, b = fv - y0f;
	const int i1 = i0 + 1 == W ? 0 : i0 + 1, j1 = j0 + 1 == H ? 0 : j0 + 1;
	const float4 T00 = img[(size_t)j0 * W + i0];
	const float4 T10 = img[(size_t)j0 * W + i1];
	const float4 T01 = img[(size_t)j1 * W + i0];
	const float4 T11 = img[(size_t)j1 * W + i1];
	const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	return mk(dm_bilinear(w00, T00.x, w10, T10.x, w01, T01.x, w11, T11.x), dm_bilinear(w00, T00.y, w10, T10.y, w01, T01.y, w11, T11.y),
	          dm_bilinear(w00, T00.z, w10, T10.z, w01, T01.z, w11, T11.z));
}

// The albedo of the hit at `pos` on shape `best`: the texel at the hit's UV where the material has a texture bound, else
// `mcolor`. Only lanes with a binding load anything beyond it. The UV per kind of shape (products and sums unfused, in this order):
//   sphere  n = (pos - centre) / radius (SHADE_WINNER's normal before the front-face flip); u = dm_atan2pif(n.z, n.x) * 0.5 + 0.5,
//           v = n.y * 0.5 + 0.5 (the sky's mapping, sky_box)
//   plane   d = pos - position; u = (d.x * T.x + d.y * T.y) + d.z * T.z, v the same with B (PlaneFrame, made by the host);
//           a plane without a frame keeps mcolor
//   model   SHADE_MESH_NORMAL's barycentric weights; uv = (uv0 * w2 + uv1 * w0) + uv2 * w1, without UVs (w0, w1)
template <bool HAS_MODELS, bool USE_BVH>
__device__ __forceinline__ f3 texture_albedo(const TraceParams &p, const TexParams &tx, int best, uint32_t best_tri, f3 pos, int material, f3 mcolor) {
	const srt_material_texture bind = tx.bindings[material];
	if (bind.texture < 0) return mcolor;
	const WinnerRec *__restrict__ wr = p.winners + best;
	const int type = wr->type;
	float u, v;
	if (type == SRT_SHAPE_SPHERE) {
		const f3 n = div3_by_rcp(pos - mk(wr->vx, wr->vy, wr->vz), wr->w, wr->inv_w);
		u = dm_atan2pif(n.z, n.x) * 0.5f + 0.5f;
		v = n.y * 0.5f + 0.5f;
	} else if (type == SRT_SHAPE_PLANE) {
		const float4 *__restrict__ fr = reinterpret_cast<const float4 *>(tx.frames + best);
		const float4 P = fr[0], T = fr[1], B = fr[2];
		if (P.w == 0.0f) return mcolor;
		const f3 d = pos - mk(P.x, P.y, P.z);
		u = (d.x * T.x + d.y * T.y) + d.z * T.z;
		v = (d.x * B.x + d.y * B.y) + d.z * B.z;
	} else if (HAS_MODELS) {
		const srt_model *__restrict__ m = &p.shapes[best].shape.model;
		const float *__restrict__ w = USE_BVH ? p.bvh_blocks + (size_t)(best_tri >> 2) * 32u + (best_tri & 3u) * SRT_BVH_TRI_FLOATS
		                                      : p.wtris + (size_t)(wr->first_wtri + best_tri) * SRT_WTRI_FLOATS;
		const uint32_t tri_in_model = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
		f3 v0 = mk(w[0], w[1], w[2]);
		f3 e1 = mk(w[3], w[4], w[5]);
		f3 e2 = mk(w[6], w[7], w[8]);
		f3 v2 = pos - v0;
		float d00 = dot3(e1, e1), d01 = dot3(e1, e2), d11 = dot3(e2, e2);
		float d20 = dot3(v2, e1), d21 = dot3(v2, e2);
		float den = d00 * d11 - d01 * d01;
		float w0 = (d11 * d20 - d01 * d21) / den;
		float w1 = (d00 * d21 - d01 * d20) / den;
		float w2 = 1.0f - w0 - w1;
		u = w0, v = w1;
		if (tx.tri_uvs) {
			const float *__restrict__ t = tx.tri_uvs + 6ull * (m->triangle_index + tri_in_model);
			u = (t[0] * w2 + t[2] * w0) + t[4] * w1;
			v = (t[1] * w2 + t[3] * w0) + t[5] * w1;
		}
	} else {
		return mcolor;
	}
	return sample_texture(tx, bind.texture, bind.filter, u * bind.scale_u, v * bind.scale_v);
}

// ---- per-triangle materials (include/srt_abi.h) ----
// The material that shades a hit on triangle `tri` (index in the scene's triangle array) of a model whose shape material is
// `material` (>= 0: the hit was decided by the shape): the table's entry where there is a table and the entry is >= 0. The
// host has checked every entry against the scene's material count, unit_materials and SRT_MF_* are computed over the whole
// material array (scene_prep.cpp) and the LDS copy holds all materials, so any index the table holds is consistent with what
// the kernel assumes of `material`. One dword per shaded mesh hit, beside the triangle's normals and UVs.
__device__ __forceinline__ int triangle_material(const TexParams &tx, uint32_t tri, int material) {
	if (!tx.tri_materials) return material; // (uniform over the launch)
	const int tm = tx.tri_materials[tri];
	return tm >= 0 ? tm : material;
}
// the same for the feature pass, which has the hit as (shape, triangle reference): SHADE_MESH_NORMAL's triangle index
template <bool HAS_MODELS, bool USE_BVH>
__device__ __forceinline__ int hit_material(const TraceParams &p, const TexParams &tx, int best, uint32_t best_tri, int material) {
	if (!HAS_MODELS || !tx.tri_materials) return material;
	const int type = p.winners[best].type;
	if (type == SRT_SHAPE_SPHERE || type == SRT_SHAPE_PLANE) return material;
	const uint32_t tri_in_model = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
	return triangle_material(tx, p.shapes[best].shape.model.triangle_index + tri_in_model, material);
}
#endif

} // namespace

#endif
