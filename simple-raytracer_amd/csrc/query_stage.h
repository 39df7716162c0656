// query_stage.h -- the layout of the queries' one staging allocation (srt_internal.h rq_stage), for the host forms of
// ray_query.hip and occlusion.hip: byte offsets of every region any of those calls uses, and the total to reserve, from the
// call's n alone. No HIP and no handle: tests/csrc/host_units_check.cpp includes it by itself.
//
//   [0, 32 n)       rays      n srt_ray: every call
//   [32 n, 64 n)    hits      n srt_ray_hit (srt_cast_rays, srt_pick)   | the same bytes:
//                   segs      n srt_segment (srt_occluded_segments, srt_segment_rays) | no call has hits and segments
//   [64 n, ...)     xy        n points of 8 bytes (srt_pick)            | the same bytes:
//                   occluded, invalid   ceil(n / 64) words of 8 bytes each (srt_occluded_rays, srt_occluded_segments) | no call has points and masks
// srt_nearest_points (nearest.hip) uses the first two regions under names of its own (NearestStage below):
//   [0, 16 n)       points    n srt_point_query: half of `rays`
//   [32 n, 64 n)    nearest   n srt_nearest: the bytes of `hits`
#ifndef SRT_QUERY_STAGE_H
#define SRT_QUERY_STAGE_H

#include <stddef.h>

struct QueryStage {
	size_t rays, hits, segs, xy, occluded, invalid; // byte offsets
	size_t total;                                    // bytes
};

// srt_ao_rays (ao.hip) lays the same allocation out for n_pixels pixels of `samples` rays each:
//   [0, 32 n_pixels samples)   rays       the call's answer
//   [.., + 32 n_pixels)        surfaces   two float4 per pixel, what the ray kernel reads
struct AoStage {
	size_t rays, surfaces; // byte offsets
	size_t total;          // bytes
};
static inline AoStage ao_stage(size_t n_pixels, size_t samples) { // n_pixels * samples < 2^31 (the call's own check)
	AoStage s;
	s.rays = 0;
	s.surfaces = 32 * n_pixels * samples;
	s.total = s.surfaces + 32 * n_pixels;
	return s;
}

static inline size_t query_mask_words(size_t n) { return (n + 63u) / 64u; }

static inline QueryStage query_stage(size_t n) { // n < 2^31 (the calls' own check): nothing here overflows 64 bits
	const size_t mask = 8 * query_mask_words(n);
	QueryStage s;
	s.rays = 0;
	s.hits = s.segs = 32 * n;
	s.xy = s.occluded = 64 * n;
	s.invalid = s.occluded + mask;
	s.total = 64 * n + (8 * n > 2 * mask ? 8 * n : 2 * mask);
	return s;
}

// srt_cast_rays_multi and srt_pick_through (multi_hit.hip) lay the same allocation out for n rays of k records each:
//   [0, 32 n)               rays     n srt_ray
//   [32 n, 32 n + 32 n k)   hits     n k srt_ray_hit
//   [.., + 4 n)             counts   n words
//   [.., + 8 n)             xy       n points of 8 bytes (srt_pick_through), 8-byte aligned
struct MultiStage {
	size_t rays, hits, counts, xy; // byte offsets
	size_t total;                  // bytes
};
static inline MultiStage multi_stage(size_t n, size_t k) { // n < 2^31, k <= 8 (the calls' own checks)
	MultiStage s;
	s.rays = 0;
	s.hits = 32 * n;
	s.counts = s.hits + 32 * n * k;
	s.xy = s.counts + 8 * ((n + 1) / 2);
	s.total = s.xy + 8 * n;
	return s;
}

struct NearestStage {
	size_t points, nearest; // byte offsets inside query_stage(n).total
};
static inline NearestStage nearest_stage(size_t n) {
	const QueryStage s = query_stage(n);
	NearestStage ns;
	ns.points = s.rays;
	ns.nearest = s.hits;
	return ns;
}

#endif
