// bloom.hip -- bloom for the resolve (include/srt_abi.h srt_set_bloom): the bright part of the exposed frame goes
// down an image pyramid (prefilter + reduce, then reduce per level), comes back up (expand-and-add per level) and is added to the
// frame before the tone map (composite). Everything is enqueued on the handle's stream behind the site's own (plain) resolve,
// whose ARGB image the composite overwrites; with exposure on it takes the place of srt_exposure_resolve_kernel.
// Plain IEEE float + * / in the order include/srt_abi.h writes down (the unit is built with -ffp-contract=off); tests/bloom_ref.py
// restates it and tests/test_gpu_bloom.py holds every level and every byte to that, bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "srt_internal.h"
#include "tonemap.h" // lum (the prefilter), tonemap (the composite)

// ---------------------------------------------------------------------------------
// Tile shapes. Both kernels are 256 lanes (four wave64), load their source tile plus halo into LDS once, run the horizontal
// pass LDS -> LDS and the vertical pass LDS -> global. Texels are float4 (alpha 0), so every access is 128-bit.
//
// Banking (ds_read_b128: bank row of 16 slots of 16 B, lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32;
// ds_write_b128: 8 contiguous lanes over 8 slots):
//   reduce   an output tile of 16 x 16, one texel per lane; source tile 34 x 34 (taps 2i-1 .. 2i+2). The source rows are stored
//            with the even columns first and the odd ones from slot SRT_BLOOM_REDUCE_ODD on, so that the four taps of the
//            horizontal pass are unit-stride over the 16 lanes of a row instead of stride 2 (2-way). A row is
//            SRT_BLOOM_REDUCE_SRC_STRIDE = 48 slots (34 used): a read group takes 8 lanes of one row and 8 of the next, which
//            stay on distinct slots only when the row stride is a multiple of 16. The intermediate is 16 wide with stride 16:
//            in the vertical pass a group's lanes are columns {0-3,12-15} of tile row ty and {4-11} of ty + 1, source rows two
//            apart, and 2 x 16 slots is a whole number of bank rows, so the 16 lanes hit 16 distinct slots. (Padding that row
//            to 17 would shift the second half by two slots onto the first.)
//   expand   an output tile of 32 x 32, four texels per lane (rows ty, ty + 8, ..); source tile 18 x 18 (i - 1 .. i + 1 for 16
//            i), stored linearly; the intermediate is 32 wide with stride 32. A read group lies inside one row in both passes
//            (32 lanes per row), its lanes on distinct columns or pairwise on the same address (broadcast).
// ---------------------------------------------------------------------------------
#define SRT_BLOOM_REDUCE_TILE 16
#define SRT_BLOOM_REDUCE_SRC (2 * SRT_BLOOM_REDUCE_TILE + 2)
#define SRT_BLOOM_REDUCE_ODD 20
#define SRT_BLOOM_REDUCE_SRC_STRIDE 48
#define SRT_BLOOM_EXPAND_TILE 32
#define SRT_BLOOM_EXPAND_SRC (SRT_BLOOM_EXPAND_TILE / 2 + 2)

struct BloomReduceParams {
	const float4 *source;  // PREFILTER: the frame (canvas or denoised image); otherwise level k - 1
	float4 *dest;          // level k
	const float *exposure; // PREFILTER: device memory, or NULL for 1.0f (exposure off)
	float divisor, threshold, knee, clamp;
	int sw, sh, dw, dh;
};

struct BloomExpandParams {
	const float4 *up;      // level k + 1 (the composite: level 0), sw x sh
	float4 *dest;          // expand-and-add: level k, dw x dh, read and written by the lane that owns the texel
	const float4 *source;  // the composite: the frame ...
	uint32_t *argb;        // ... and the ARGB image it overwrites
	const float *exposure; // as above
	float divisor;
	float weight; // scatter, or intensity for the composite
	int sw, sh, dw, dh;
};

namespace {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// x = (c / divisor) * e per channel: the colour the site exposes (alpha is loaded with the texel and never used)
__device__ __forceinline__ float4 bloom_exposed(float4 c, float divisor, float e) {
	return make_float4((c.x / divisor) * e, (c.y / divisor) * e, (c.z / divisor) * e, 0.0f);
}

// step 1 of the definition
__device__ __forceinline__ float4 bloom_bright(float4 x, float threshold, float knee, float clamp) {
	const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	const float L = lum(x.x, x.y, x.z);
	if (!(__builtin_isfinite(x.x) && __builtin_isfinite(x.y) && __builtin_isfinite(x.z) && __builtin_isfinite(L)) || !(L > 0.0f)) return none;
	float g = L - threshold;
	if (knee > 0.0f) {
		float s = (L - threshold) + knee;
		const float top = 2.0f * knee;
		s = s < 0.0f ? 0.0f : s > top ? top : s;
		const float q = (s * s) / (4.0f * knee);
		g = q > g ? q : g;
	}
	if (clamp > 0.0f) g = g < clamp ? g : clamp;
	if (!(g > 0.0f)) return none;
	const float k = g / L;
	return make_float4(x.x * k, x.y * k, x.z * k, 0.0f);
}

// ((a + d) + 3 (b + c)) / 8
__device__ __forceinline__ float reduce1(float a, float b, float c, float d) { return ((a + d) + 3.0f * (b + c)) * 0.125f; }
__device__ __forceinline__ float4 reduce4(float4 a, float4 b, float4 c, float4 d) {
	return make_float4(reduce1(a.x, b.x, c.x, d.x), reduce1(a.y, b.y, c.y, d.y), reduce1(a.z, b.z, c.z, d.z), 0.0f);
}
// 0.75 near + 0.25 far
__device__ __forceinline__ float4 expand4(float4 n, float4 f) {
	return make_float4(0.75f * n.x + 0.25f * f.x, 0.75f * n.y + 0.25f * f.y, 0.75f * n.z + 0.25f * f.z, 0.0f);
}

} // namespace

// Step 2: one workgroup per 16 x 16 tile of level k. PREFILTER: the source is the frame and step 1 runs on the way into LDS
template <bool PREFILTER>
__global__ __launch_bounds__(256) void srt_bloom_reduce_kernel(const BloomReduceParams p) {
	__shared__ float4 src[SRT_BLOOM_REDUCE_SRC][SRT_BLOOM_REDUCE_SRC_STRIDE];
	__shared__ float4 hor[SRT_BLOOM_REDUCE_SRC][SRT_BLOOM_REDUCE_TILE];
	const int ox0 = (int)blockIdx.x * SRT_BLOOM_REDUCE_TILE, oy0 = (int)blockIdx.y * SRT_BLOOM_REDUCE_TILE;
	float e = 1.0f;
	if (PREFILTER && p.exposure) e = *p.exposure;
	// tile column c, row r <-> source texel (2 ox0 - 1 + c, 2 oy0 - 1 + r), clamped to the edge: every read is inside the image
	for (int idx = (int)threadIdx.x; idx < SRT_BLOOM_REDUCE_SRC * SRT_BLOOM_REDUCE_SRC; idx += 256) {
		const int r = idx / SRT_BLOOM_REDUCE_SRC, c = idx - r * SRT_BLOOM_REDUCE_SRC;
		const int sx = clampi(2 * ox0 - 1 + c, p.sw - 1), sy = clampi(2 * oy0 - 1 + r, p.sh - 1);
		float4 v = p.source[(size_t)sy * (size_t)p.sw + (size_t)sx];
		if (PREFILTER) v = bloom_bright(bloom_exposed(v, p.divisor, e), p.threshold, p.knee, p.clamp);
		else v.w = 0.0f;
		src[r][(c >> 1) + ((c & 1) ? SRT_BLOOM_REDUCE_ODD : 0)] = v;
	}
	__syncthreads();
	// horizontal: output column tx of the tile takes tile columns 2 tx .. 2 tx + 3
	for (int idx = (int)threadIdx.x; idx < SRT_BLOOM_REDUCE_SRC * SRT_BLOOM_REDUCE_TILE; idx += 256) {
		const int r = idx / SRT_BLOOM_REDUCE_TILE, tx = idx % SRT_BLOOM_REDUCE_TILE;
		hor[r][tx] = reduce4(src[r][tx], src[r][SRT_BLOOM_REDUCE_ODD + tx], src[r][tx + 1], src[r][SRT_BLOOM_REDUCE_ODD + tx + 1]);
	}
	__syncthreads();
	const int tx = (int)threadIdx.x % SRT_BLOOM_REDUCE_TILE, ty = (int)threadIdx.x / SRT_BLOOM_REDUCE_TILE;
	const int ox = ox0 + tx, oy = oy0 + ty;
	if (ox < p.dw && oy < p.dh) p.dest[(size_t)oy * (size_t)p.dw + (size_t)ox] = reduce4(hor[2 * ty][tx], hor[2 * ty + 1][tx], hor[2 * ty + 2][tx], hor[2 * ty + 3][tx]);
}

// Steps 3 and 4: one workgroup per 32 x 32 tile of the destination. COMPOSITE: the destination is the frame's ARGB image
template <bool COMPOSITE>
__global__ __launch_bounds__(256) void srt_bloom_expand_kernel(const BloomExpandParams p) {
	__shared__ float4 src[SRT_BLOOM_EXPAND_SRC][SRT_BLOOM_EXPAND_SRC];
	__shared__ float4 hor[SRT_BLOOM_EXPAND_SRC][SRT_BLOOM_EXPAND_TILE];
	const int dx0 = (int)blockIdx.x * SRT_BLOOM_EXPAND_TILE, dy0 = (int)blockIdx.y * SRT_BLOOM_EXPAND_TILE;
	const int sx0 = dx0 / 2 - 1, sy0 = dy0 / 2 - 1;
	// tile column c, row r <-> source texel (sx0 + c, sy0 + r), clamped to the edge
	for (int idx = (int)threadIdx.x; idx < SRT_BLOOM_EXPAND_SRC * SRT_BLOOM_EXPAND_SRC; idx += 256) {
		const int r = idx / SRT_BLOOM_EXPAND_SRC, c = idx - r * SRT_BLOOM_EXPAND_SRC;
		const int sx = clampi(sx0 + c, p.sw - 1), sy = clampi(sy0 + r, p.sh - 1);
		float4 v = p.up[(size_t)sy * (size_t)p.sw + (size_t)sx];
		v.w = 0.0f;
		src[r][c] = v;
	}
	__syncthreads();
	// horizontal: destination column x of the tile is source i = x / 2, tile column i + 1; the far tap is i - 1 (x even) or i + 1
	for (int idx = (int)threadIdx.x; idx < SRT_BLOOM_EXPAND_SRC * SRT_BLOOM_EXPAND_TILE; idx += 256) {
		const int r = idx / SRT_BLOOM_EXPAND_TILE, x = idx % SRT_BLOOM_EXPAND_TILE;
		const int i = (x >> 1) + 1;
		hor[r][x] = expand4(src[r][i], src[r][(x & 1) ? i + 1 : i - 1]);
	}
	__syncthreads();
	float e = 1.0f;
	if (COMPOSITE && p.exposure) e = *p.exposure;
	const int x = (int)threadIdx.x % SRT_BLOOM_EXPAND_TILE, gx = dx0 + x;
	for (int y = (int)threadIdx.x / SRT_BLOOM_EXPAND_TILE; y < SRT_BLOOM_EXPAND_TILE; y += 256 / SRT_BLOOM_EXPAND_TILE) {
		const int gy = dy0 + y;
		if (gx >= p.dw || gy >= p.dh) continue;
		const int j = (y >> 1) + 1;
		const float4 v = expand4(hor[j][x], hor[(y & 1) ? j + 1 : j - 1][x]);
		const size_t at = (size_t)gy * (size_t)p.dw + (size_t)gx;
		if (COMPOSITE) {
			const float4 c = bloom_exposed(p.source[at], p.divisor, e);
			p.argb[at] = tonemap(c.x + p.weight * v.x, c.y + p.weight * v.y, c.z + p.weight * v.z);
		} else {
			const float4 d = p.dest[at];
			p.dest[at] = make_float4(d.x + p.weight * v.x, d.y + p.weight * v.y, d.z + p.weight * v.z, 0.0f);
		}
	}
}

namespace {

int check_params(const srt_bloom_params &p) {
	for (float v : {p.threshold, p.knee, p.intensity, p.scatter, p.clamp})
		if (!std::isfinite(v)) return SRT_ERR_INVALID;
	if (!(p.threshold >= 0.0f)) return SRT_ERR_INVALID;
	if (!(p.knee >= 0.0f && p.knee <= p.threshold)) return SRT_ERR_INVALID;
	if (!(p.intensity >= 0.0f && p.intensity <= 16.0f)) return SRT_ERR_INVALID;
	if (!(p.scatter >= 0.0f && p.scatter <= 1.0f)) return SRT_ERR_INVALID;
	if (!(p.clamp >= 0.0f)) return SRT_ERR_INVALID;
	if (p.levels < 1 || p.levels > SRT_BLOOM_MAX_LEVELS) return SRT_ERR_INVALID;
	if (p.reserved != 0) return SRT_ERR_INVALID;
	return SRT_OK;
}

// the sizes of the levels of a w x h frame and their first texel in the pyramid; -> the effective level count
int plan_levels(int w, int h, int levels, int lw[SRT_BLOOM_MAX_LEVELS], int lh[SRT_BLOOM_MAX_LEVELS], size_t first[SRT_BLOOM_MAX_LEVELS + 1]) {
	int n = 0;
	first[0] = 0;
	while (n < levels) {
		w = (w + 1) / 2, h = (h + 1) / 2;
		lw[n] = w, lh[n] = h;
		first[n + 1] = first[n] + (size_t)w * (size_t)h;
		n++;
		if (w == 1 && h == 1) break;
	}
	return n;
}

dim3 tiles(int w, int h, int tile) { return dim3((unsigned)((w + tile - 1) / tile), (unsigned)((h + tile - 1) / tile)); }

} // namespace

bool srt_bloom_begin(srt_tracer *t, bool picture, size_t num_pixels) {
	BloomState *bl = t->bl;
	bl->last_bloomed = bl->on && picture && num_pixels != 0;
	return bl->last_bloomed;
}

int srt_bloom_resolve(srt_tracer *t, const float *source, float divisor, const float *exposure, uint32_t w, uint32_t h, uint8_t *argb) {
	BloomState *bl = t->bl;
	const srt_bloom_params &bp = bl->p;
	int lw[SRT_BLOOM_MAX_LEVELS], lh[SRT_BLOOM_MAX_LEVELS];
	size_t first[SRT_BLOOM_MAX_LEVELS + 1];
	const int n = plan_levels((int)w, (int)h, bp.levels, lw, lh, first);
	SRT_HIP(t, bl->pyramid.reserve(first[n] * 4)); // (grows only when a larger frame than the one it was made for comes by)
	float4 *pyr = reinterpret_cast<float4 *>(bl->pyramid.ptr);
	const float4 *frame = reinterpret_cast<const float4 *>(source);
	for (int k = 0; k < n; k++) {
		BloomReduceParams rp;
		rp.source = k ? pyr + first[k - 1] : frame;
		rp.dest = pyr + first[k];
		rp.exposure = exposure;
		rp.divisor = divisor, rp.threshold = bp.threshold, rp.knee = bp.knee, rp.clamp = bp.clamp;
		rp.sw = k ? lw[k - 1] : (int)w, rp.sh = k ? lh[k - 1] : (int)h;
		rp.dw = lw[k], rp.dh = lh[k];
		if (k) hipLaunchKernelGGL(srt_bloom_reduce_kernel<false>, tiles(rp.dw, rp.dh, SRT_BLOOM_REDUCE_TILE), dim3(256), 0, t->stream, rp);
		else hipLaunchKernelGGL(srt_bloom_reduce_kernel<true>, tiles(rp.dw, rp.dh, SRT_BLOOM_REDUCE_TILE), dim3(256), 0, t->stream, rp);
	}
	BloomExpandParams ep;
	ep.source = frame;
	ep.argb = reinterpret_cast<uint32_t *>(argb);
	ep.exposure = exposure;
	ep.divisor = divisor;
	for (int k = n - 2; k >= 0; k--) {
		ep.up = pyr + first[k + 1], ep.dest = pyr + first[k];
		ep.weight = bp.scatter;
		ep.sw = lw[k + 1], ep.sh = lh[k + 1], ep.dw = lw[k], ep.dh = lh[k];
		hipLaunchKernelGGL(srt_bloom_expand_kernel<false>, tiles(ep.dw, ep.dh, SRT_BLOOM_EXPAND_TILE), dim3(256), 0, t->stream, ep);
	}
	ep.up = pyr, ep.dest = nullptr;
	ep.weight = bp.intensity;
	ep.sw = lw[0], ep.sh = lh[0], ep.dw = (int)w, ep.dh = (int)h;
	hipLaunchKernelGGL(srt_bloom_expand_kernel<true>, tiles(ep.dw, ep.dh, SRT_BLOOM_EXPAND_TILE), dim3(256), 0, t->stream, ep);
	SRT_HIP(t, hipGetLastError());
	bl->last_w = (int)w, bl->last_h = (int)h, bl->last_levels = n;
	return SRT_OK;
}

extern "C" {

int srt_bloom_defaults(srt_bloom_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->enable = 1;
	out->threshold = 1.0f;
	out->knee = 0.5f;
	out->intensity = 0.1f;
	out->scatter = 0.7f;
	out->clamp = 64.0f;
	out->levels = 6;
	return SRT_OK;
}

int srt_bloom_check_host(const srt_bloom_params *p) { return p ? check_params(*p) : SRT_ERR_INVALID; }

int srt_set_bloom(srt_tracer *t, const srt_bloom_params *p) {
	if (!t) return SRT_ERR_INVALID;
	BloomState *bl = t->bl;
	if (!p || !p->enable) { // off: the sites launch what they launch without the feature
		bl->on = false;
		bl->last_bloomed = false;
		return SRT_OK;
	}
	if (check_params(*p))
		return fail(t, SRT_ERR_INVALID, "srt_set_bloom: threshold >= 0, 0 <= knee <= threshold, 0 <= intensity <= 16, 0 <= scatter <= 1, clamp >= 0, "
		                                "1 <= levels <= 8, all finite, reserved 0");
	SRT_HIP(t, hipSetDevice(t->device));
	// the pyramid of the handle's frame at every level count: about a third of a frame's float4
	int lw[SRT_BLOOM_MAX_LEVELS], lh[SRT_BLOOM_MAX_LEVELS];
	size_t first[SRT_BLOOM_MAX_LEVELS + 1];
	const int n = plan_levels(t->width, t->height, SRT_BLOOM_MAX_LEVELS, lw, lh, first);
	SRT_HIP(t, bl->pyramid.reserve(first[n] * 4));
	bl->p = *p;
	bl->on = true;
	return SRT_OK;
}

int srt_read_bloom(srt_tracer *t, int level, float *rgba_out, size_t cap_pixels, int *w, int *h) {
	if (!t) return SRT_ERR_INVALID;
	BloomState *bl = t->bl;
	if (bl->last_levels == 0) return fail(t, SRT_ERR_STATE, "srt_read_bloom: no bloomed frame on this handle yet");
	if (level < 0 || level >= bl->last_levels) return fail(t, SRT_ERR_INVALID, "srt_read_bloom: level outside the last bloomed frame's pyramid");
	int lw[SRT_BLOOM_MAX_LEVELS], lh[SRT_BLOOM_MAX_LEVELS];
	size_t first[SRT_BLOOM_MAX_LEVELS + 1];
	plan_levels(bl->last_w, bl->last_h, bl->last_levels, lw, lh, first);
	if (w) *w = lw[level];
	if (h) *h = lh[level];
	SRT_HIP(t, hipSetDevice(t->device));
	if (rgba_out) {
		const size_t n = (size_t)lw[level] * (size_t)lh[level];
		if (cap_pixels < n) return fail(t, SRT_ERR_INVALID, "srt_read_bloom: rgba_out is smaller than the level");
		SRT_HIP(t, hipMemcpyAsync(rgba_out, bl->pyramid.ptr + first[level] * 4, n * 16, hipMemcpyDeviceToHost, t->stream));
	}
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	return SRT_OK;
}

int srt_last_resolve_bloomed(const srt_tracer *t, int *bloomed) {
	if (!t || !bloomed) return SRT_ERR_INVALID;
	*bloomed = t->bl->last_bloomed ? 1 : 0;
	return SRT_OK;
}

} // extern "C"
