// selection.hip -- the ID pass and the selection overlay (include/srt_abi.h "selection overlay and the ID pass"). A translation
// unit of its own: the kernels here are new, every kernel the library launched before keeps its instruction stream
// (scripts/kernel_isa_digest.py).
//
//  * srt_id_pass_kernel<HAS_MODELS, USE_BVH>: one lane per pixel. The ray through the pixel's centre is srt_pick_rays_kernel's
//    (device_math.h camera_ray), refused and walked as srt_ray_query_kernel refuses and walks it: ray_valid.inc and
//    closest_hit.inc, the text both kernels include -- text, because moving those statements into __device__ functions changed
//    the cast kernels' instruction streams -- and three words stored per pixel: shape, triangle inside its
//    model, material. Nothing is staged: the 64 B ray and the 32 B record of the pick path never exist.
//  * srt_selection_outline_kernel: one workgroup of 256 lanes per 32 x 8 pixel tile. The selection mask of the tile and its
//    halo of R pixels sits in LDS as one 64-bit word per row (32 + 2 R <= 48 columns), each made by one ballot; a workgroup
//    whose words are all zero leaves after one vote having read the ID plane's shape words and nothing else. The distance to
//    the nearest selected pixel comes from shifts and count-leading / count-trailing-zeros on the row words; the alpha comes
//    from the host's table (selection_host.h), so the device computes no square root. The composite over the resolved bytes is
//    part of the same kernel.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_shading.h"
#include "selection_host.h"
#include "query_host.h"

#define SRT_SEL_TILE_W 32
#define SRT_SEL_TILE_H 8
#define SRT_SEL_ROWS (SRT_SEL_TILE_H + 2 * SRT_SELECTION_MAX_WIDTH)

struct IdPassParams {
	TraceParams tp;               /* the scene buffers and the camera, as a dispatch's (rd: the frame; f_width .. inv_f_height) */
	uint32_t *shape, *triangle;   /* n words each */
	int32_t *material;            /* n words */
	const int32_t *tri_materials; /* per-triangle materials of the scene's triangle array, or NULL */
	uint32_t n;                   /* width * height */
};

struct OutlineParams {
	const uint32_t *shape; /* the ID pass's shape plane, w * h words */
	const uint32_t *bits;  /* the selection: bit s of the table for shape s < n_shapes */
	const uint8_t *table;  /* alpha by squared distance, 2 R^2 + 1 entries */
	uint32_t *argb;        /* the resolved picture, w * h words: bytes A, R, G, B */
	uint8_t *alpha;        /* w * h bytes, zeroed before the launch: only touched pixels are written */
	uint32_t n_shapes;
	int32_t w, h, radius;
	uint32_t fill_alpha, fill_word, outline_word; /* the colours as picture words (R, G, B in bytes 1..3) */
};

template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_id_pass_kernel(const IdPassParams ip) {
	const TraceParams &p = ip.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= ip.n) return; // lanes past the frame in the last workgroup store nothing
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	// ---- the pixel centre's ray: srt_pick_rays_kernel's, of xy = (px + 0.5, py + 0.5) ----
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
	// ---- the three words ----
	uint32_t shape = SRT_HIT_NONE, tri = SRT_HIT_NONE;
	int material = -1;
	if (best >= 0) {
		const WinnerRec *__restrict__ wr = p.winners + best;
		shape = (uint32_t)best;
		material = wr->material; // a shape without a material is reported, as the cast reports it
		if (HAS_MODELS && wr->type != SRT_SHAPE_SPHERE && wr->type != SRT_SHAPE_PLANE) {
			tri = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
			if (ip.tri_materials && material >= 0) { // (uniform over the launch) the material the trace shades the hit with
				const int tm = ip.tri_materials[p.shapes[best].shape.model.triangle_index + tri];
				material = tm >= 0 ? tm : material;
			}
		}
	}
	ip.shape[q] = shape;
	ip.triangle[q] = tri;
	ip.material[q] = material;
}

// one byte of the composite: (byte * (255 - a) + colour * a + 127) / 255
__device__ __forceinline__ uint32_t sel_mix(uint32_t byte, uint32_t colour, uint32_t a) { return (byte * (255u - a) + colour * a + 127u) / 255u; }

__global__ __launch_bounds__(256) void srt_selection_outline_kernel(const OutlineParams op) {
	__shared__ unsigned long long rows[SRT_SEL_ROWS]; // bit c of rows[r]: m(x0 - R + c, y0 - R + r); pixels outside the frame are 0
	__shared__ uint32_t vote_any[4], vote_all[4];
	__shared__ uint8_t table[SRT_SELECTION_TABLE_MAX + 3];
	const int R = op.radius;
	const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
	const int x0 = (int)blockIdx.x * SRT_SEL_TILE_W, y0 = (int)blockIdx.y * SRT_SEL_TILE_H;
	// ---- the mask: a wave makes one row word per ballot, lane = column ----
	const int n_rows = SRT_SEL_TILE_H + 2 * R;
	const int gx = x0 - R + lane;
	const bool col_in = lane < SRT_SEL_TILE_W + 2 * R && gx >= 0 && gx < op.w;
	const int tile_w = op.w - x0 < SRT_SEL_TILE_W ? op.w - x0 : SRT_SEL_TILE_W;
	const unsigned long long tile_cols = ((1ull << tile_w) - 1ull) << R; // the tile's columns inside the frame
	unsigned long long any = 0ull;
	bool all = true;
	for (int r = wave; r < n_rows; r += 4) {
		const int gy = y0 - R + r;
		bool m = false;
		if (col_in && gy >= 0 && gy < op.h) {
			const uint32_t s = op.shape[(size_t)gy * (size_t)op.w + (size_t)gx];
			if (s < op.n_shapes) m = ((op.bits[s >> 5] >> (s & 31u)) & 1u) != 0u;
		}
		const unsigned long long word = __ballot(m);
		if (lane == 0) rows[r] = word;
		any |= word;
		if (r >= R && r < R + SRT_SEL_TILE_H && gy < op.h) all = all && (word & tile_cols) == tile_cols;
	}
	if (lane == 0) vote_any[wave] = any != 0ull ? 1u : 0u, vote_all[wave] = all ? 1u : 0u;
	__syncthreads();
	if (!(vote_any[0] | vote_any[1] | vote_any[2] | vote_any[3])) return; // nothing selected near this tile: most of the frame
	const bool all_wg = (vote_all[0] & vote_all[1] & vote_all[2] & vote_all[3]) != 0u;
	const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
	const int px = x0 + tx, py = y0 + ty;
	uint32_t a = op.fill_alpha, colour = op.fill_word;
	if (!all_wg) { // (uniform over the workgroup) else: every pixel of the tile is selected, fill and leave
		const int n_table = 2 * R * R + 1;
		if ((int)threadIdx.x < n_table) table[threadIdx.x] = op.table[threadIdx.x];
		__syncthreads();
		const int c = tx + R; // the pixel's column in the row words
		if (!((rows[ty + R] >> c) & 1ull)) {
			const unsigned long long window = ((2ull << (2 * R)) - 1ull) << tx; // columns c - R .. c + R
			const unsigned long long upto = (2ull << c) - 1ull;               // columns 0 .. c
			int d2 = 1 << 20;
			auto row = [&](int r, int dy2) {
				const unsigned long long word = rows[r] & window;
				if (word == 0ull) return;
				const unsigned long long left = word & upto, right = word >> c;
				int dx = 64;
				if (left) dx = c - (63 - __clzll((long long)left));
				if (right) {
					const int dr = __ffsll((long long)right) - 1;
					dx = dr < dx ? dr : dx;
				}
				const int d = dx * dx + dy2;
				d2 = d < d2 ? d : d2;
			};
			row(ty + R, 0);
			for (int dy = 1; dy <= R; dy++) {
				const int dy2 = dy * dy;
				if (dy2 >= d2) break; // this row and every farther one cannot be closer
				row(ty + R - dy, dy2);
				row(ty + R + dy, dy2);
			}
			a = 0u, colour = op.outline_word;
			if (d2 < n_table) a = table[d2];
		}
	}
	if (a == 0u || px >= op.w || py >= op.h) return; // untouched pixels are not written
	const size_t q = (size_t)py * (size_t)op.w + (size_t)px;
	const uint32_t v = op.argb[q];
	op.argb[q] = (v & 255u) | (sel_mix((v >> 8) & 255u, (colour >> 8) & 255u, a) << 8) | (sel_mix((v >> 16) & 255u, (colour >> 16) & 255u, a) << 16) |
	             (sel_mix(v >> 24, colour >> 24, a) << 24);
	op.alpha[q] = (uint8_t)a;
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
namespace {

uint32_t colour_word(const uint8_t argb[4]) { return ((uint32_t)argb[1] << 8) | ((uint32_t)argb[2] << 16) | ((uint32_t)argb[3] << 24); }

SelectionKey key_of(const srt_tracer *scene, const srt_render_data &rd) {
	SelectionKey k;
	memset(&k, 0, sizeof k); // (compared byte for byte)
	k.scene_rev = scene->scene_rev;
	k.scene = scene;
	k.tri_materials = srt_texture_params(scene).tri_materials;
	memcpy(k.camera_to_world, rd.camera_to_world, sizeof k.camera_to_world);
	k.aspect_ratio = rd.aspect_ratio, k.fov_scale = rd.fov_scale;
	k.width = rd.width, k.height = rd.height;
	return k;
}

// the ID pass of `scene`'s scene under rd's camera and frame into t's planes, on t's stream (both handles live on one device)
int enqueue_id_pass(srt_tracer *t, const srt_tracer *scene, const srt_render_data &rd) {
	SelectionState *s = t->sel;
	const size_t px = (size_t)rd.width * (size_t)rd.height;
	if (s->ids.cap < 3 * px) { // (a grown buffer replaces one a queued launch may still use: first use, or a larger frame)
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		SRT_HIP(t, s->ids.reserve(3 * px));
	}
	s->ids_valid = false;
	IdPassParams ip;
	memset(&ip, 0, sizeof ip);
	ip.tp = srt_trace_params_for_query(scene, &rd);
	ip.shape = s->ids.ptr, ip.triangle = s->ids.ptr + px;
	ip.material = reinterpret_cast<int32_t *>(s->ids.ptr + 2 * px);
	ip.tri_materials = srt_texture_params(scene).tri_materials;
	ip.n = (uint32_t)px;
	query_launch(SRT_QUERY_KERNEL(srt_id_pass_kernel, ip.tp), ip, ip.n, t->stream);
	SRT_HIP(t, hipGetLastError());
	s->ids_w = rd.width, s->ids_h = rd.height;
	s->ids_key = key_of(scene, rd);
	s->ids_valid = true;
	return SRT_OK;
}

// the set as a bit table over the scene's shapes, and the alpha table, on the device when they have changed
int sync_tables(srt_tracer *t, const srt_tracer *scene) {
	SelectionState *s = t->sel;
	if (s->bits_dirty || s->bits_rev != scene->scene_rev) {
		// (the host copy is rewritten: what was enqueued from it has to have left. Only behind srt_set_selection or srt_update_scene,
		// which have waited for the stream themselves)
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		const uint32_t n = scene->scene_set ? (uint32_t)scene->sd.num_shapes : 0u;
		s->bits_host.assign((size_t)(n + 31u) / 32u + 1u, 0u);
		for (uint32_t i : s->shapes)
			if (i < n) s->bits_host[i >> 5] |= 1u << (i & 31u); // an index beyond the scene never matches
		SRT_HIP(t, s->bits.reserve(s->bits_host.size()));
		SRT_HIP(t, hipMemcpyAsync(s->bits.ptr, s->bits_host.data(), s->bits_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
		s->bits_shapes = n, s->bits_rev = scene->scene_rev, s->bits_dirty = false;
	}
	if (s->table_dirty) {
		SRT_HIP(t, s->table.reserve(sizeof s->table_host));
		SRT_HIP(t, hipMemcpyAsync(s->table.ptr, s->table_host, sizeof s->table_host, hipMemcpyHostToDevice, t->stream));
		s->table_dirty = false;
	}
	return SRT_OK;
}

} // namespace

int srt_selection_apply(srt_tracer *t, uint32_t w, uint32_t h, bool picture, uint8_t *argb) {
	SelectionState *s = t->sel;
	if (!s->on) return SRT_OK; // off: nothing, and last_applied / last_id_ran stay 0 (srt_set_selection cleared them)
	s->last_applied = s->last_id_ran = false;
	const srt_tracer *scene = s->scene;
	if (!picture || !scene || !scene->have_last_rd || w == 0 || h == 0) return SRT_OK;
	const srt_render_data &rd = scene->last_rd;
	if ((uint32_t)rd.width != w || (uint32_t)rd.height != h) return SRT_OK; // (the bytes are not the frame the last dispatch traced)
	if (const int rc = sync_tables(t, scene)) return rc;
	const SelectionKey key = key_of(scene, rd);
	if (!s->ids_valid || memcmp(&key, &s->ids_key, sizeof key) != 0) {
		if (const int rc = enqueue_id_pass(t, scene, rd)) return rc;
		s->last_id_ran = true;
	}
	const size_t px = (size_t)w * (size_t)h;
	if (s->alpha.cap < px) {
		SRT_HIP(t, hipStreamSynchronize(t->stream));
		SRT_HIP(t, s->alpha.reserve(px));
	}
	SRT_HIP(t, hipMemsetAsync(s->alpha.ptr, 0, px, t->stream));
	OutlineParams op;
	memset(&op, 0, sizeof op);
	op.shape = s->ids.ptr, op.bits = s->bits.ptr, op.table = s->table.ptr;
	op.argb = reinterpret_cast<uint32_t *>(argb), op.alpha = s->alpha.ptr;
	op.n_shapes = s->bits_shapes;
	op.w = (int32_t)w, op.h = (int32_t)h, op.radius = s->radius;
	op.fill_alpha = s->p.fill_argb[0], op.fill_word = colour_word(s->p.fill_argb), op.outline_word = colour_word(s->p.outline_argb);
	hipLaunchKernelGGL(srt_selection_outline_kernel, dim3((w + SRT_SEL_TILE_W - 1) / SRT_SEL_TILE_W, (h + SRT_SEL_TILE_H - 1) / SRT_SEL_TILE_H), dim3(256), 0,
	                   t->stream, op);
	SRT_HIP(t, hipGetLastError());
	s->alpha_w = (int)w, s->alpha_h = (int)h;
	s->last_applied = true;
	return SRT_OK;
}

int srt_selection_ids_current(srt_tracer *t, const srt_render_data *rd, bool *ran) {
	*ran = false;
	if (rd->width <= 0 || rd->height <= 0) return fail(t, SRT_ERR_INVALID, "area selection: options->width and height must be positive");
	if ((uint64_t)rd->width * (uint64_t)rd->height >= (1ull << 31)) return fail(t, SRT_ERR_INVALID, "area selection: the frame must stay below 2^31 pixels");
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table (a part of the key) as the next dispatch would see it
	const SelectionKey key = key_of(t, *rd);
	if (t->sel->ids_valid && memcmp(&key, &t->sel->ids_key, sizeof key) == 0) return SRT_OK;
	*ran = true;
	return enqueue_id_pass(t, t, *rd);
}

extern "C" {

int srt_selection_defaults(srt_selection_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->enabled = 1;
	out->outline_width = 2.0f;
	out->outline_argb[0] = 255, out->outline_argb[1] = 255, out->outline_argb[2] = 160, out->outline_argb[3] = 0;
	out->fill_argb[0] = 0, out->fill_argb[1] = 255, out->fill_argb[2] = 160, out->fill_argb[3] = 0;
	return SRT_OK;
}

int srt_selection_check_host(const srt_selection_params *p) { return p ? selection_check_params(*p) : SRT_ERR_INVALID; }

int srt_selection_sizes(size_t out[1]) {
	if (!out) return SRT_ERR_INVALID;
	out[0] = sizeof(srt_selection_params);
	return SRT_OK;
}

int srt_selection_alpha_table_host(const srt_selection_params *p, uint8_t *table, size_t cap, int *radius) {
	if (!p || !table) return SRT_ERR_INVALID;
	const int R = selection_alpha_table(*p, table, cap);
	if (R < 0) return SRT_ERR_INVALID;
	if (radius) *radius = R;
	return SRT_OK;
}

int srt_set_selection(srt_tracer *t, const srt_selection_params *p, const uint32_t *shapes, size_t n) {
	if (!t) return SRT_ERR_INVALID;
	SelectionState *s = t->sel;
	if (!p || !p->enabled || n == 0) { // off: the sites launch what they launch without the feature
		if (p && p->enabled != 1 && p->enabled != 0) return fail(t, SRT_ERR_INVALID, "srt_set_selection: enabled is 0 or 1");
		s->on = false;
		s->last_applied = s->last_id_ran = false;
		return SRT_OK;
	}
	if (selection_check_params(*p)) return fail(t, SRT_ERR_INVALID, "srt_set_selection: enabled 0 or 1, 1 <= outline_width <= 8 and finite, reserved 0");
	if (!shapes) return fail(t, SRT_ERR_INVALID, "srt_set_selection: shapes is NULL");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // the tables' host copies may still be on their way
	try {
		s->shapes.assign(shapes, shapes + n);
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
	memset(s->table_host, 0, sizeof s->table_host);
	s->radius = selection_alpha_table(*p, s->table_host, sizeof s->table_host);
	s->p = *p;
	s->scene = t;
	s->bits_dirty = s->table_dirty = true;
	s->on = true;
	return SRT_OK;
}

int srt_render_ids(srt_tracer *t, const srt_render_data *options) {
	if (!t) return SRT_ERR_INVALID;
	if (!options) return fail(t, SRT_ERR_INVALID, "srt_render_ids: options is NULL");
	if (options->width <= 0 || options->height <= 0) return fail(t, SRT_ERR_INVALID, "srt_render_ids: options->width and height must be positive");
	if ((uint64_t)options->width * (uint64_t)options->height >= (1ull << 31)) return fail(t, SRT_ERR_INVALID, "srt_render_ids: the frame must stay below 2^31 pixels");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = srt_texture_sync(t)) return rc; // the per-triangle material table as the next dispatch would see it
	return enqueue_id_pass(t, t, *options);
}

int srt_read_id_pass(srt_tracer *t, uint32_t *shape, uint32_t *triangle, int32_t *material, size_t cap_pixels, int *w, int *h) {
	if (!t) return SRT_ERR_INVALID;
	SelectionState *s = t->sel;
	if (s->ids_w == 0 || !s->ids.ptr) return fail(t, SRT_ERR_STATE, "srt_read_id_pass: no ID pass on this handle yet");
	if (w) *w = s->ids_w;
	if (h) *h = s->ids_h;
	const size_t px = (size_t)s->ids_w * (size_t)s->ids_h;
	if ((shape || triangle || material) && cap_pixels < px) return fail(t, SRT_ERR_INVALID, "srt_read_id_pass: the arrays are smaller than the planes");
	SRT_HIP(t, hipSetDevice(t->device));
	if (shape) SRT_HIP(t, hipMemcpyAsync(shape, s->ids.ptr, px * 4, hipMemcpyDeviceToHost, t->stream));
	if (triangle) SRT_HIP(t, hipMemcpyAsync(triangle, s->ids.ptr + px, px * 4, hipMemcpyDeviceToHost, t->stream));
	if (material) SRT_HIP(t, hipMemcpyAsync(material, s->ids.ptr + 2 * px, px * 4, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_read_selection_alpha(srt_tracer *t, uint8_t *alpha, size_t cap_pixels) {
	if (!t) return SRT_ERR_INVALID;
	SelectionState *s = t->sel;
	if (!alpha) return fail(t, SRT_ERR_INVALID, "srt_read_selection_alpha: alpha is NULL");
	if (s->alpha_w == 0) return fail(t, SRT_ERR_STATE, "srt_read_selection_alpha: no overlaid frame on this handle yet");
	const size_t px = (size_t)s->alpha_w * (size_t)s->alpha_h;
	if (cap_pixels < px) return fail(t, SRT_ERR_INVALID, "srt_read_selection_alpha: alpha is smaller than the frame");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemcpyAsync(alpha, s->alpha.ptr, px, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_last_resolve_selected(const srt_tracer *t, int *applied, int *id_pass_ran) {
	if (!t) return SRT_ERR_INVALID;
	if (applied) *applied = t->sel->last_applied ? 1 : 0;
	if (id_pass_ran) *id_pass_ran = t->sel->last_id_ran ? 1 : 0;
	return SRT_OK;
}

} // extern "C"
