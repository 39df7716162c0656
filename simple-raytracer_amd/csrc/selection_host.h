// selection_host.h -- what of the selection overlay (selection.hip; include/srt_abi.h "selection overlay") needs no handle and
// no HIP: the parameter check and the outline's alpha table. Behind srt_selection_check_host and
// srt_selection_alpha_table_host, and compiled on its own by tests/csrc/selection_host_check.cpp.
#ifndef SRT_SELECTION_HOST_H
#define SRT_SELECTION_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/srt_abi.h"

// SRT_OK when srt_set_selection accepts the block
static inline int selection_check_params(const srt_selection_params &p) {
	if (p.enabled != 0 && p.enabled != 1) return SRT_ERR_INVALID;
	if (!std::isfinite(p.outline_width) || p.outline_width < 1.0f || p.outline_width > (float)SRT_SELECTION_MAX_WIDTH) return SRT_ERR_INVALID;
	for (int32_t r : p.reserved)
		if (r != 0) return SRT_ERR_INVALID;
	return SRT_OK;
}

// R = ceil(width + 0.5) - 1 of a checked width: 1..8
static inline int selection_radius(float width) { return (int)std::ceil((double)width + 0.5) - 1; }

// table[d2] = floor(clamp(width + 0.5 - sqrt(d2), 0, 1) * outline alpha + 0.5), d2 = 0 .. 2 R^2; returns R, or -1 when the
// block is refused or cap < 2 R^2 + 1
static inline int selection_alpha_table(const srt_selection_params &p, uint8_t *table, size_t cap) {
	if (selection_check_params(p) != SRT_OK || !table) return -1;
	const int R = selection_radius(p.outline_width);
	const size_t n = (size_t)(2 * R * R + 1);
	if (cap < n) return -1;
	const double w = (double)p.outline_width, a = (double)p.outline_argb[0];
	for (size_t d2 = 0; d2 < n; d2++) {
		double c = w + 0.5 - std::sqrt((double)d2);
		c = c < 0.0 ? 0.0 : c > 1.0 ? 1.0 : c;
		table[d2] = (uint8_t)std::floor(c * a + 0.5);
	}
	return R;
}

#endif
