// ao.hip -- the ambient-occlusion pass behind the ABI (include/srt_abi.h "ambient-occlusion pass"): per pixel, how many of S
// cosine-weighted hemisphere rays from the visible surface meet anything within a radius. A translation unit of its own: the
// kernels here are new, every kernel the library launched before keeps its instruction stream (scripts/kernel_isa_digest.py).
//
//  * srt_ao_surface_kernel<HAS_MODELS, USE_BVH>: the ID pass's launch shape (one lane per pixel, 64 lanes per workgroup), its
//    pixel-centre ray (device_math.h camera_ray) and its refusal and walk (ray_valid.inc, closest_hit.inc: text, DESIGN.md 28,
//    29), then the cast's facing normal. Stores 32 B per pixel: {O, has-surface}, {N, 0} with O = (org + dir t) + N bias.
//  * ao_make_ray: THE ray of (pixel, sample), from the pixel's two words -- the trace's per-lane random unit vector
//    (random_normal3_lane, normalize3) seeded from the item's index, added to the normal and normalised: the cosine law.
//    The trace's bounce flips that vector into the normal's hemisphere first (trace_body.inc "cosine weighted direction"),
//    which narrows the law to 45 degrees about the normal; the pass does not. Both kernels below call it.
//  * srt_ao_kernel<HAS_MODELS, USE_BVH>: one lane per (pixel, sample), item i = q S + s. S divides 64, so a wave holds 64 / S
//    whole pixels, a pixel's lanes are adjacent and its two float4 loads are broadcasts. The lane makes its ray and runs
//    srt_occlusion_kernel's body on it: the runs and blocks with tmin = tmax, the any-hit scan and walk of device_anyhit.h, the
//    ballot after each run that leaves the loop when no active lane is still unoccluded. Lanes past the last item and lanes of
//    pixels without a surface stay for the ballots, inactive. A pixel's count is one popcount of the wave's final ballot under
//    the pixel's S-bit field, stored by its lane s == 0: no atomics, no LDS; the walk's stack is scratch, as the cast's.
//  * srt_ao_rays_kernel: the same item mapping over a window of pixels, storing the ray instead of walking it (srt_ao_rays).
//  * srt_ao_view_kernel: the grey picture from the count plane and the host's 65-entry table.
// The host side's scaffold is query_host.h, shared with the other query units; what needs no HIP is ao_host.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_anyhit.h"
#include "device_shading.h"
#include "ao_host.h"
#include "query_host.h"

struct AoSurfaceParams {
	TraceParams tp;   /* the scene buffers and the camera, as a dispatch's (rd: the frame; f_width .. inv_f_height) */
	float4 *surfaces; /* 2 n float4: pixel first + k at 2 k */
	uint32_t first;   /* the first pixel of the window (the pass: 0) */
	uint32_t n;       /* pixels of the window */
	float bias;
};
struct AoParams {
	TraceParams tp;         /* the scene buffers (rd: unused) */
	const float4 *surfaces; /* 2 float4 per pixel of the frame */
	uint32_t *occluded;     /* a word per pixel */
	uint32_t n_items;       /* pixels * S */
	uint32_t log2_s;
	uint32_t seed;
	float radius;
};
struct AoRaysParams {
	const float4 *surfaces; /* 2 float4 per pixel of the window */
	float4 *rays;           /* n_items srt_ray */
	uint32_t n_items;       /* pixels of the window * S */
	uint32_t first_item;    /* first pixel * S: the index the window's first ray has in the frame */
	uint32_t log2_s;
	uint32_t seed;
	float radius;
};
struct AoViewParams {
	const uint32_t *occluded; /* n words */
	const uint8_t *table;     /* SRT_AO_MAX_SAMPLES + 1 entries */
	uint32_t *argb;           /* n words: bytes A, R, G, B */
	uint32_t n;
	uint32_t background; /* as a picture word */
};

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_ao_surface_kernel(const AoSurfaceParams sp) {
	const TraceParams &p = sp.tp;
	const uint32_t k = blockIdx.x * 64u + threadIdx.x;
	if (k >= sp.n) return; // lanes past the window in the last workgroup store nothing
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	// ---- the pixel centre's ray: srt_id_pass_kernel's ----
	const uint32_t q = sp.first + k;
	const uint32_t width = (uint32_t)p.rd.width;
	const uint32_t py = q / width, px = q - py * width;
	const float2 xy = make_float2((float)px + 0.5f, (float)py + 0.5f);
	f3 org, dir;
	camera_ray(p, xy, org, dir);
	// ---- srt_ray_query_kernel under SRT_RAYS_UNIT_DIRECTIONS with tmax = +inf, as srt_pick casts it ----
	const float tmax = DM_INF_F;
	const uint32_t flags = SRT_RAYS_UNIT_DIRECTIONS;
#include "ray_valid.inc"
	float tmin = DM_INF_F;
	int best = -1;
	uint32_t best_tri = 0;
	if (valid) {
		BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		uint32_t n_tri = 0, n_tri_u = 0;
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
#include "closest_hit.inc"
	}
	// ---- the two words ----
	float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
	if (best >= 0) {
		const f3 pos = org + dir * tmin;
		f3 nrm = winner_normal<HAS_MODELS, USE_BVH>(p, best, best_tri, pos);
		nrm = nrm * (dot3(nrm, dir) < 0.0f ? 1.0f : -1.0f); // the cast's facing normal
		const f3 o = pos + nrm * sp.bias;
		s0.x = o.x, s0.y = o.y, s0.z = o.z, s0.w = 1.0f;
		s1.x = nrm.x, s1.y = nrm.y, s1.z = nrm.z;
	}
	sp.surfaces[2u * k] = s0;
	sp.surfaces[2u * k + 1u] = s1;
}

// The ray of item = q S + s from pixel q's two words: a cosine-weighted direction about N, seeded from the item. A pixel
// without a surface: tmax = NaN over a zero origin and direction, an invalid ray by the cast's rule.
__device__ __forceinline__ void ao_make_ray(float4 s0, float4 s1, uint32_t item, uint32_t base_seed, float radius, float4 &r0, float4 &r1) {
	uint32_t seed = base_seed + item * 0x9E3779B9u;
	const f3 nrm = mk(s1.x, s1.y, s1.z);
	const f3 rd = normalize3(random_normal3_lane(seed));
	const f3 d = normalize3(nrm + rd); // N + a uniform direction of the whole sphere: the cosine law (no hemisphere flip, see the header)
	const bool has = s0.w != 0.0f;
	r0.x = s0.x, r0.y = s0.y, r0.z = s0.z, r0.w = has ? radius : dm_u2f(0x7fc00000u); // (a surfaceless pixel's words are 0)
	r1.x = has ? d.x : 0.0f, r1.y = has ? d.y : 0.0f, r1.z = has ? d.z : 0.0f, r1.w = 0.0f;
}

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_ao_kernel(const AoParams ap) {
	const TraceParams &p = ap.tp;
	const uint32_t i = blockIdx.x * 64u + threadIdx.x;
	const bool in = i < ap.n_items; // lanes past the last item load nothing and vote 0: they stay for the ballots
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	const uint32_t q = i >> ap.log2_s; // a workgroup's first item is a multiple of 64, so of S: a pixel never straddles two waves
	float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
	if (in) s0 = ap.surfaces[2u * q], s1 = ap.surfaces[2u * q + 1u];
	float4 r0, r1;
	ao_make_ray(s0, s1, i, ap.seed, ap.radius, r0, r1);
	// ---- srt_occlusion_kernel under SRT_RAYS_UNIT_DIRECTIONS from here on ----
	const f3 org = mk(r0.x, r0.y, r0.z);
	f3 dir = mk(r1.x, r1.y, r1.z);
	const float tmax = r0.w;
	const uint32_t flags = SRT_RAYS_UNIT_DIRECTIONS;
#include "ray_valid.inc"
	const bool active = in && valid && tmax > 0.0f;
	float tmin = tmax;
	int best = -1;
	if (active) { // (the ballots below are over the lanes in here)
		AnyStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
		auto test_model = [&](float lx, float ly, float lz, float hx, float hy, float hz, uint32_t ref, uint32_t count, int idx) {
			if (best < 0 && test_aabb(lx, ly, lz, hx, hy, hz, org, inv, tmax)) {
				const bool occ = USE_BVH ? walk_bvh_any(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, ref, org, dir, tmax SRT_RC_ARG)
				                         : test_triangles_any(p.wtris, ref, count, org, dir, tmax SRT_RC_ARG);
				if (occ) best = idx;
			}
		};
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
				if (((code >> 2) & 7u) <= 2u) test_spheres<2>(b, org, dir, base, tmin, best);
				else test_spheres<4>(b, org, dir, base, tmin, best);
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
				test_planes2(b, (code >> 2) & 7u, org, dir, base, tmin, best);
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				test_model(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], f2u(b.v[3]), f2u(b.v[7]), base);
				if (((code >> 2) & 7u) > 1u) test_model(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], f2u(b.v[11]), f2u(b.v[15]), base + 1);
			}
		};
		for (int g = 0; g < p.num_runs; g++) {
			float gh[4];
			ld_uniform<4, 16>(reinterpret_cast<const float *>(p.runs + g), gh);
			const uint32_t code = f2u(gh[0]);
			const float *__restrict__ gd = p.run_data + 48 * g;
			test_block(ld_blk16(gd), code & 255u, (int)f2u(gh[1]));
			if ((code >> 8) & 255u) test_block(ld_blk16(gd + 16), (code >> 8) & 255u, (int)f2u(gh[2]));
			if ((code >> 16) & 255u) test_block(ld_blk16(gd + 32), (code >> 16) & 255u, (int)f2u(gh[3]));
			if (!any64(best < 0)) break; // (wave-uniform) nobody is left to ask
		}
	}
	// ---- the answer: the pixel's S bits of the wave's ballot, counted by its first lane ----
	const unsigned long long occluded = ballot64(active && best >= 0);
	const uint32_t samples = 1u << ap.log2_s;
	if (in && (i & (samples - 1u)) == 0u) {
		const unsigned long long field = samples == 64u ? ~0ull : (1ull << samples) - 1ull; // (a shift by 64 is not one)
		const uint32_t count = (uint32_t)__popcll((occluded >> threadIdx.x) & field);
		ap.occluded[q] = s0.w != 0.0f ? count : SRT_HIT_NONE;
	}
}

__global__ __launch_bounds__(64) void srt_ao_rays_kernel(const AoRaysParams rp) {
	const uint32_t j = blockIdx.x * 64u + threadIdx.x;
	if (j >= rp.n_items) return;
	const uint32_t k = j >> rp.log2_s; // the pixel inside the window
	const float4 s0 = rp.surfaces[2u * k], s1 = rp.surfaces[2u * k + 1u];
	float4 r0, r1;
	ao_make_ray(s0, s1, rp.first_item + j, rp.seed, rp.radius, r0, r1);
	rp.rays[2u * j] = r0;
	rp.rays[2u * j + 1u] = r1;
}

__global__ __launch_bounds__(64) void srt_ao_view_kernel(const AoViewParams vp) {
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= vp.n) return;
	const uint32_t c = vp.occluded[q];
	uint32_t word = vp.background;
	if (c <= SRT_AO_MAX_SAMPLES) { // (else: SRT_HIT_NONE)
		const uint32_t g = vp.table[c];
		word = 255u | (g << 8) | (g << 16) | (g << 24);
	}
	vp.argb[q] = word;
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

const char *const kAoRules = "samples one of 1, 2, 4, 8, 16, 32, 64; radius > 0; bias >= 0 and finite; reserved 0; width, height > 0 and width * height * samples < 2^31";

int check_call(srt_tracer *t, const char *who, const srt_render_data *options, const srt_ao_params *params) {
	if (!options || !params) return fail(t, SRT_ERR_INVALID, std::string(who) + ": NULL argument");
	if (ao_check_params(*params, options->width, options->height)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": " + kAoRules);
	return SRT_OK;
}

// the surface records of pixels first .. first + n of options' frame into `surfaces`, on the handle's stream
int enqueue_surfaces(srt_tracer *t, const TraceParams &tp, const srt_ao_params &params, size_t first, size_t n, void *surfaces) {
	AoSurfaceParams sp;
	memset(&sp, 0, sizeof sp);
	sp.tp = tp;
	sp.surfaces = static_cast<float4 *>(surfaces);
	sp.first = (uint32_t)first, sp.n = (uint32_t)n;
	sp.bias = params.bias;
	query_launch(SRT_QUERY_KERNEL(srt_ao_surface_kernel, sp.tp), sp, sp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

} // namespace

extern "C" {

int srt_ao_defaults(srt_ao_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->samples = 16;
	out->radius = INFINITY;
	out->bias = 0.001f;
	out->background = 0xff000000u;
	return SRT_OK;
}

int srt_ao_check_host(const srt_ao_params *p, int width, int height) { return p ? ao_check_params(*p, width, height) : SRT_ERR_INVALID; }

int srt_ao_sizes(size_t out[1]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_ao_params);
	return SRT_OK;
}

int srt_ao_table_host(const srt_ao_params *p, uint8_t table[65]) {
	if (!p || !table) return SRT_ERR_INVALID;
	return ao_grey_table(p->samples, table);
}

int srt_render_ao(srt_tracer *t, const srt_render_data *options, const srt_ao_params *params) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = check_call(t, "srt_render_ao", options, params)) return rc;
	SRT_HIP(t, hipSetDevice(t->device));
	AoState &ao = t->ao;
	const size_t px = (size_t)options->width * (size_t)options->height;
	if (ao.surfaces.cap < 8 * px || ao.occluded.cap < px || ao.table_samples != params->samples) {
		// (a grown buffer replaces one a queued launch may still use, and the table's host copy is rewritten: first use, a larger
		// frame or another sample count)
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		SRT_HIP(t, ao.surfaces.reserve(8 * px));
		SRT_HIP(t, ao.occluded.reserve(px));
		if (ao.table_samples != params->samples) {
			ao.table_samples = 0;
			memset(ao.table_host, 0, sizeof ao.table_host);
			(void)ao_grey_table(params->samples, ao.table_host);
			SRT_HIP(t, ao.table.reserve(sizeof ao.table_host));
			SRT_HIP(t, hipMemcpyAsync(ao.table.ptr, ao.table_host, sizeof ao.table_host, hipMemcpyHostToDevice, t->stream));
			ao.table_samples = params->samples;
		}
	}
	ao.w = ao.h = 0;
	if (const int rc = query_span_begin(t)) return rc;
	AoParams ap;
	memset(&ap, 0, sizeof ap);
	ap.tp = srt_trace_params_for_query(t, options);
	if (const int rc = enqueue_surfaces(t, ap.tp, *params, 0, px, ao.surfaces.ptr)) return rc;
	ap.surfaces = reinterpret_cast<const float4 *>(ao.surfaces.ptr);
	ap.occluded = ao.occluded.ptr;
	ap.n_items = (uint32_t)(px * params->samples);
	ap.log2_s = (uint32_t)ao_samples_log2(params->samples);
	ap.seed = params->seed;
	ap.radius = params->radius;
	query_launch(SRT_QUERY_KERNEL(srt_ao_kernel, ap.tp), ap, ap.n_items, t->stream);
	SRT_HIP(t, hipGetLastError());
	if (const int rc = query_span_end(t)) return rc;
	ao.w = options->width, ao.h = options->height;
	ao.p = *params;
	return SRT_OK;
}

int srt_read_ao(srt_tracer *t, uint32_t *occluded, size_t cap_pixels, int *w, int *h, int *samples) {
	if (!t) return SRT_ERR_INVALID;
	const AoState &ao = t->ao;
	if (ao.w == 0) return fail(t, SRT_ERR_STATE, "srt_read_ao: no ambient-occlusion pass on this handle yet");
	if (w) *w = ao.w;
	if (h) *h = ao.h;
	if (samples) *samples = (int)ao.p.samples;
	if (!occluded) return SRT_OK;
	const size_t px = (size_t)ao.w * (size_t)ao.h;
	if (cap_pixels < px) return fail(t, SRT_ERR_INVALID, "srt_read_ao: the array is smaller than the plane");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemcpyAsync(occluded, ao.occluded.ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_ao_rays(srt_tracer *t, const srt_render_data *options, const srt_ao_params *params, size_t first_pixel, size_t n_pixels, srt_ray *rays_out) {
	if (!t) return SRT_ERR_INVALID;
	if (const int rc = check_call(t, "srt_ao_rays", options, params)) return rc;
	const size_t px = (size_t)options->width * (size_t)options->height;
	if (first_pixel > px || n_pixels > px - first_pixel) return fail(t, SRT_ERR_INVALID, "srt_ao_rays: first_pixel + n_pixels is beyond the frame");
	if (n_pixels == 0) return SRT_OK;
	if (!rays_out) return fail(t, SRT_ERR_INVALID, "srt_ao_rays: rays_out is NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // (a grown buffer replaces one a queued launch may still use)
	const AoStage st = ao_stage(n_pixels, params->samples);
	SRT_HIP(t, t->rq_stage.reserve(st.total));
	uint8_t *const stage = t->rq_stage.ptr;
	if (const int rc = query_span_begin(t)) return rc;
	if (const int rc = enqueue_surfaces(t, srt_trace_params_for_query(t, options), *params, first_pixel, n_pixels, stage + st.surfaces)) return rc;
	AoRaysParams rp;
	memset(&rp, 0, sizeof rp);
	rp.surfaces = reinterpret_cast<const float4 *>(stage + st.surfaces);
	rp.rays = reinterpret_cast<float4 *>(stage + st.rays);
	rp.n_items = (uint32_t)(n_pixels * params->samples);
	rp.first_item = (uint32_t)(first_pixel * params->samples);
	rp.log2_s = (uint32_t)ao_samples_log2(params->samples);
	rp.seed = params->seed;
	rp.radius = params->radius;
	query_launch(srt_ao_rays_kernel, rp, rp.n_items, t->stream);
	SRT_HIP(t, hipGetLastError());
	if (const int rc = query_span_end(t)) return rc;
	SRT_HIP(t, hipMemcpyAsync(rays_out, stage + st.rays, (size_t)rp.n_items * sizeof(srt_ray), hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_resolve_ao_view(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	const AoState &ao = t->ao;
	if (ao.w == 0) return fail(t, SRT_ERR_STATE, "srt_resolve_ao_view: no ambient-occlusion pass on this handle yet");
	if (ao.w != t->width || ao.h != t->height) return fail(t, SRT_ERR_STATE, "srt_resolve_ao_view: the last pass's frame is not the handle's size");
	SRT_HIP(t, hipSetDevice(t->device));
	AoViewParams vp;
	memset(&vp, 0, sizeof vp);
	vp.occluded = ao.occluded.ptr;
	vp.table = ao.table.ptr;
	vp.argb = reinterpret_cast<uint32_t *>(t->argb.ptr); // (width * height * 4 bytes since srt_create, whatever the partition)
	vp.n = (uint32_t)full_pixels(t);
	const uint32_t bg = ao.p.background; // 0xAARRGGBB -> the bytes A, R, G, B in memory
	vp.background = (bg >> 24) | ((bg >> 8) & 0xff00u) | ((bg << 8) & 0xff0000u) | (bg << 24);
	if (const int rc = query_span_begin(t)) return rc;
	query_launch(srt_ao_view_kernel, vp, vp.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	return query_span_end(t);
}

} // extern "C"
