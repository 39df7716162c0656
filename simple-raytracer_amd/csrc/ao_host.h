// ao_host.h -- what of the ambient-occlusion pass (ao.hip; include/srt_abi.h "ambient-occlusion pass") needs no handle and no
// HIP: the parameter check and the view's grey table. Behind srt_ao_check_host and srt_ao_table_host; a host program can include
// it on its own.
#ifndef SRT_AO_HOST_H
#define SRT_AO_HOST_H

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/srt_abi.h"

// log2 of a sample count the pass takes (1, 2, 4, ... 64), else -1
static inline int ao_samples_log2(uint32_t samples) {
	for (int k = 0; k <= 6; k++)
		if (samples == (1u << k)) return k;
	return -1;
}

// SRT_OK when srt_render_ao accepts the block for a frame of width x height
static inline int ao_check_params(const srt_ao_params &p, int64_t width, int64_t height) {
	if (ao_samples_log2(p.samples) < 0) return SRT_ERR_INVALID;
	if (!(p.radius > 0.0f)) return SRT_ERR_INVALID; // (a NaN compares false; +inf passes)
	if (!std::isfinite(p.bias) || !(p.bias >= 0.0f)) return SRT_ERR_INVALID;
	for (uint32_t r : p.reserved)
		if (r != 0u) return SRT_ERR_INVALID;
	if (width <= 0 || height <= 0 || width >= ((int64_t)1 << 31) || height >= ((int64_t)1 << 31)) return SRT_ERR_INVALID;
	// width * height * samples < 2^31, without overflow: width * height < 2^62 fits, and it is compared before it is scaled
	const uint64_t px = (uint64_t)width * (uint64_t)height;
	if (px >= ((uint64_t)1 << 31) || px * (uint64_t)p.samples >= ((uint64_t)1 << 31)) return SRT_ERR_INVALID;
	return SRT_OK;
}

// table[c] = floor(255 * (1 - c / S) + 0.5), c = 0 .. S, in double; the entries past S are 0. SRT_ERR_INVALID: samples refused
static inline int ao_grey_table(uint32_t samples, uint8_t table[SRT_AO_MAX_SAMPLES + 1]) {
	if (ao_samples_log2(samples) < 0 || !table) return SRT_ERR_INVALID;
	for (uint32_t c = 0; c <= SRT_AO_MAX_SAMPLES; c++)
		table[c] = c <= samples ? (uint8_t)std::floor(255.0 * (1.0 - (double)c / (double)samples) + 0.5) : (uint8_t)0;
	return SRT_OK;
}

#endif
