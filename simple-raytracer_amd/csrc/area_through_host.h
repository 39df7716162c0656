// area_through_host.h -- what of X-ray area selection (area_through.hip; include/srt_abi.h "area selection, through") needs no
// handle and no HIP: the check of the frame the rays are made for, and the launch grid over the clipped rectangle -- area.hip's
// mapping, a wave per 64 pixels of one row, four rows per workgroup. Compiled on its own by tests/csrc/area_through_host_check.cpp.
#ifndef SRT_AREA_THROUGH_HOST_H
#define SRT_AREA_THROUGH_HOST_H

#include "area_host.h"

// SRT_OK when a w x h frame can be covered: both positive, fewer than 2^31 pixels (as srt_render_ids checks its frame)
static inline int area_through_frame_check(int32_t w, int32_t h) {
	if (w <= 0 || h <= 0) return SRT_ERR_INVALID;
	if ((uint64_t)w * (uint64_t)h >= (1ull << 31)) return SRT_ERR_INVALID;
	return SRT_OK;
}

struct AreaThroughGrid {
	int32_t c[4];        /* the rectangle clipped to the frame: x0, y0, x1, y1 */
	uint32_t col_groups; /* ceil((x1 - x0) / 64) */
	uint32_t row_groups; /* ceil((y1 - y0) / 4) */
	uint32_t blocks;     /* col_groups * row_groups; 0: the clipped rectangle is empty, nothing is launched */
};

// the grid of a checked block over a checked w x h frame. blocks < 2^31: a workgroup holds at least one pixel of the frame in
// its first lane, and the frame is below 2^31 pixels
static inline void area_through_grid(const srt_area &a, int32_t w, int32_t h, AreaThroughGrid *g) {
	area_clip(a, w, h, g->c);
	g->col_groups = g->row_groups = g->blocks = 0u;
	if (g->c[0] < g->c[2] && g->c[1] < g->c[3]) {
		g->col_groups = (uint32_t)(((int64_t)g->c[2] - g->c[0] + 63) / 64);
		g->row_groups = (uint32_t)(((int64_t)g->c[3] - g->c[1] + 3) / 4);
		g->blocks = g->col_groups * g->row_groups;
	}
}

#endif
