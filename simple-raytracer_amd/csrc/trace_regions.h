// trace_regions.h -- where the trace kernel's instructions are executed (development aid): the region list and the markers
// that device_intersect.h, kernels.hip and trace_body.inc place.
#ifndef SRT_TRACE_REGIONS_H
#define SRT_TRACE_REGIONS_H

#include "device_types.h" // SRT_REGION_MAX

// SRT_REGION(NAME) marks the start of a stretch of the trace kernel that runs as often as its first statement. In the
// product build it expands to nothing; scripts/isa_phase_mix.py reads the markers' source lines and assigns every
// instruction of the compiled kernel (by its line-table entry) to the region it was written in. A -DSRT_REGION_COUNT
// build counts, per region, how often a wave ran it and with how many lanes (two LDS words per region, summed per wave
// into its counter line; srt_debug_region_counters): static instruction mix x measured frequency = the executed mix.
#define SRT_REGION_LIST(X)                                                                                                             \
	X(PROLOGUE) X(LOOP_HEAD) X(EXTEND_SETUP) X(EXTEND_GROUP) X(EXTEND_SUSPEND)                                                       \
	X(EXTEND_SPHERES2_0) X(EXTEND_SPHERES2_1) X(EXTEND_SPHERES2_2) X(EXTEND_SPHERES4_0) X(EXTEND_SPHERES4_1) X(EXTEND_SPHERES4_2)   \
	X(EXTEND_PLANES_0) X(EXTEND_PLANES_1) X(EXTEND_PLANES_2) X(EXTEND_MODEL_0) X(EXTEND_MODEL_1) X(EXTEND_MODEL_2)                   \
	X(EXTEND_TRI_LOOP) X(EXTEND_TRI_EXACT) X(EXTEND_TRI_DIV) X(EXTEND_BVH_STEP) X(EXTEND_BVH_SPILL) X(EXTEND_BVH_PUSH2) X(EXTEND_BVH_PUSH3) X(EXTEND_BVH_POP) X(EXTEND_FINISH) X(SKY_PUSH) X(SKY_RESOLVE) X(SHADE_HEAD) X(SHADE_POP) X(SHADE_WINNER)   \
	X(SHADE_MESH_NORMAL) X(SHADE_MATERIAL) X(SHADE_BOUNCE) X(SHADE_OPAQUE) X(SHADE_GLASS) X(SHADE_REFRACT) X(SHADE_TAIL) X(PARK)     \
	X(HANDIN) X(HANDIN_ORPHAN) X(REFILL_HEAD) X(REFILL_SCANQ) X(REFILL_POOL) X(REFILL_UNPARK) X(REFILL_LOOP) X(REFILL_OPEN) X(REFILL_FLUSH) X(REFILL_CURSOR)         \
	X(REFILL_TAKE) X(CAMERA) X(LOOP_TAIL) X(EPILOGUE)
enum SrtRegion {
#define SRT_REGION_ENUM(n) R_##n,
	SRT_REGION_LIST(SRT_REGION_ENUM)
#undef SRT_REGION_ENUM
	R_COUNT
};
static_assert(R_COUNT <= SRT_REGION_MAX, "device_types.h SRT_REGION_MAX");
// Scheduling diagnostics (iterations, SHADE phases, stragglers, early write-outs; srt_debug_counters out[5..7]) cost a few
// scalar instructions and a vote per loop iteration: kept out of the product build, on in every development build.
#if defined(SRT_DIAG) || defined(SRT_REGION_COUNT) || defined(SRT_PHASE_CLOCK)
#define SRT_DIAG_ON 1
#else
#define SRT_DIAG_ON 0
#endif
#ifdef SRT_REGION_COUNT
#define SRT_REGION(name) region_hit(region_ctr, R_##name)
#define SRT_REGION_SLOT(name, slot) region_hit(region_ctr, R_##name##_0 + (slot)) // a stretch compiled once per block slot of a group (test_block)
#define SRT_RC_PARAM , uint32_t *region_ctr
#define SRT_RC_ARG , region_ctr
__device__ __forceinline__ void region_hit(uint32_t *ctr, int r) {
	const unsigned long long m = __ballot(1); // the lanes that are here
	if ((int)threadIdx.x == __ffsll((long long)m) - 1) {
		atomicAdd(&ctr[2 * r], 1u);
		atomicAdd(&ctr[2 * r + 1], (uint32_t)__popcll(m));
	}
}
#else
#define SRT_REGION(name)
#define SRT_REGION_SLOT(name, slot)
#define SRT_RC_PARAM
#define SRT_RC_ARG
#endif

#endif
