// area_host.h -- what of area selection (area.hip; include/srt_abi.h "area selection") needs no handle and no HIP: the check of
// an area block, the clip of its rectangle to a frame, and the lasso rule on doubled integer coordinates. The rule's two
// functions are the ones the counting kernel compiles (AREA_HD), so the host mask and the device mask are one statement.
// Behind srt_area_check_host and srt_area_mask_host, and compiled on its own by tests/csrc/area_host_check.cpp.
#ifndef SRT_AREA_HOST_H
#define SRT_AREA_HOST_H

#include <cstddef>
#include <cstdint>

#include "../../include/srt_abi.h"

#ifdef __HIPCC__
#define AREA_HD __host__ __device__ static inline
#else
#define AREA_HD static inline
#endif

#define SRT_AREA_COORD_MAX (1 << 20) /* |vertex coordinate| <= this */

// An edge A -> B (doubled, so even) spans the row of the odd C.y when its ends lie on different sides; equality cannot occur
AREA_HD bool area_edge_spans(int32_t ay, int32_t by, int32_t cy) { return (ay < cy) != (by < cy); }

// A spanning edge counts when C lies strictly on its left going up, strictly on its right going down; C on the edge: not counted.
// |B - A| <= 2^22 and |C.y - A.y| <= 2^22 for a spanning edge, C.x is a pixel of a frame (below 2^32): every product fits int64
AREA_HD bool area_edge_counts(int32_t ax, int32_t ay, int32_t bx, int32_t by, int64_t cx, int32_t cy) {
	const int64_t cross = (int64_t)(bx - ax) * (int64_t)(cy - ay) - (int64_t)(by - ay) * (cx - (int64_t)ax);
	return by > ay ? cross > 0 : cross < 0;
}

// SRT_OK when the coverage calls accept the block
static inline int area_check(const srt_area *a, const int32_t *vertices) {
	if (!a) return SRT_ERR_INVALID;
	if (a->flags != 0u || a->reserved[0] != 0u || a->reserved[1] != 0u) return SRT_ERR_INVALID;
	if (a->x1 < a->x0 || a->y1 < a->y0) return SRT_ERR_INVALID;
	const uint32_t n = a->n_vertices;
	if (n == 0u) return SRT_OK;
	if (n < 3u || n > SRT_AREA_MAX_VERTICES || !vertices) return SRT_ERR_INVALID;
	for (uint32_t i = 0; i < 2u * n; i++)
		if (vertices[i] < -SRT_AREA_COORD_MAX || vertices[i] > SRT_AREA_COORD_MAX) return SRT_ERR_INVALID;
	return SRT_OK;
}

// the rectangle of a checked block inside a w x h frame: c[0..3] = x0, y0, x1, y1 with x0 <= x1, y0 <= y1
static inline void area_clip(const srt_area &a, int32_t w, int32_t h, int32_t c[4]) {
	c[0] = a.x0 < 0 ? 0 : a.x0 > w ? w : a.x0;
	c[1] = a.y0 < 0 ? 0 : a.y0 > h ? h : a.y0;
	c[2] = a.x1 < 0 ? 0 : a.x1 > w ? w : a.x1;
	c[3] = a.y1 < 0 ? 0 : a.y1 > h ? h : a.y1;
	if (c[2] < c[0]) c[2] = c[0];
	if (c[3] < c[1]) c[3] = c[1];
}

// the doubled vertices of a checked block into v2 (2 n words), and the lowest and highest doubled y into yr
static inline void area_double(const int32_t *vertices, uint32_t n, int32_t *v2, int32_t yr[2]) {
	yr[0] = yr[1] = 0;
	for (uint32_t i = 0; i < n; i++) {
		v2[2 * i] = 2 * vertices[2 * i], v2[2 * i + 1] = 2 * vertices[2 * i + 1];
		if (i == 0 || v2[2 * i + 1] < yr[0]) yr[0] = v2[2 * i + 1];
		if (i == 0 || v2[2 * i + 1] > yr[1]) yr[1] = v2[2 * i + 1];
	}
}

// pixel (px, py) against the doubled polygon: the even-odd rule
AREA_HD bool area_inside(const int32_t *v2, uint32_t n, int32_t px, int32_t py) {
	const int64_t cx = 2 * (int64_t)px + 1;
	const int32_t cy = 2 * py + 1;
	bool in = false;
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t j = i + 1u == n ? 0u : i + 1u;
		if (area_edge_spans(v2[2 * i + 1], v2[2 * j + 1], cy) && area_edge_counts(v2[2 * i], v2[2 * i + 1], v2[2 * j], v2[2 * j + 1], cx, cy)) in = !in;
	}
	return in;
}

// M(p) over a w x h frame, one byte per pixel (0 or 1); SRT_ERR_INVALID: the block is refused, w or h not positive, w * h >= 2^31,
// mask NULL or cap < w * h
static inline int area_mask(const srt_area *a, const int32_t *vertices, int32_t w, int32_t h, uint8_t *mask, size_t cap) {
	if (area_check(a, vertices) != SRT_OK || w <= 0 || h <= 0 || !mask) return SRT_ERR_INVALID;
	if ((uint64_t)w * (uint64_t)h >= (1ull << 31) || cap < (size_t)w * (size_t)h) return SRT_ERR_INVALID;
	int32_t c[4], v2[2 * SRT_AREA_MAX_VERTICES], yr[2];
	area_clip(*a, w, h, c);
	area_double(vertices, a->n_vertices, v2, yr);
	for (int32_t y = 0; y < h; y++)
		for (int32_t x = 0; x < w; x++) {
			bool m = x >= c[0] && x < c[2] && y >= c[1] && y < c[3];
			if (m && a->n_vertices) m = area_inside(v2, a->n_vertices, x, y);
			mask[(size_t)y * (size_t)w + (size_t)x] = m ? 1 : 0;
		}
	return SRT_OK;
}

#endif
