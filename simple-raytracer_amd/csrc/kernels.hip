// kernels.hip — the trace unit: the persistent path-tracing kernel, its scene-class twin, the denoiser's feature kernels
// and their launch wrappers. The device helpers they are made of live in device_math.h (f3, exact sqrt / division, RNG),
// device_intersect.h (the shape tests, the BVH walk) and device_shading.h (sky, winner normal, textures); the loop itself is
// trace_body.inc. The kernels around a trace launch (ordered reduction, pre-pass, resolve) are frame.hip, the device
// self-tests selftest.hip.
//
// What they compute is the reference's `render` and `average` OpenCL kernels
// (src/render.cl:483-535 and the helpers :114-481); how they compute
// it is CDNA4-first and shares no structure with that file:
//
//  * srt_trace_kernel: ONE WORK-ITEM PER (PIXEL, SAMPLE) PATH, persistent waves. The
//    reference's three nested loops (samples x bounces x shapes) are flattened into a
//    single loop over path SEGMENTS; a lane whose path ends (sky miss, bounce limit,
//    show_normals) pulls the next item of the wave's job in the same iteration (ballot +
//    mbcnt compaction), waves pull jobs from one global cursor, so lanes stay busy until
//    the whole dispatch is done and any slice of the frame fills the chip. Each path's
//    radiance is written to HBM (12 B; 25 GB at 1920x1080x1024 spp, what 288 GB are for)
//    and srt_reduce_kernel (frame.hip) sums them per pixel in sample order, which keeps the canvas
//    bit-identical to the reference's serial `color += trace(...)` (render.cl:518).
//  * Phases only a few lanes need at a time are not run masked in every iteration but
//    batched through LDS at full occupancy: camera-ray set-up for a whole sub-job when it
//    is opened, and the sky lookup of escaped paths through a 64-entry ring.
//  * The shape loop index is wave-uniform, so shape records and world-space triangles
//    arrive through SCALAR loads (s_load_dwordx*) into SGPRs and feed VALU ops as
//    scalar operands: no per-lane loads, no LDS traffic and no VGPRs for scene data.
//  * Winner data (normal, material) is fetched once per segment AFTER the loop, per
//    lane, instead of at every improving hit as render.cl:311-312,336-343 do: only the
//    last improving hit survives there, so deferring is exact.
//  * Triangles are pre-transformed to world space once per scene (srt_prepass_kernel)
//    in the reference's operation order, removing 63 of ~115 flops per triangle test.
//  * Model shapes optionally carry a BVH (srt_set_acceleration): a per-lane, stack-based walk over
//    four-wide 128-byte blocks (walk_bvh) replaces the array scan, same triangle test, same tie rule.
//  * No MFMA: nothing here is a contraction. Compiled with -ffp-contract=off; every
//    float op is an IEEE add/mul/div/sqrt or a detmath.h routine so that results match
//    the CPU oracle bit for bit (DESIGN.md "Numerics"). The kernel is VALU-issue bound, so
//    instruction count is what is tuned: shared-reciprocal division, guard-free sqrt where
//    the argument allows, no SLP vectorisation (packed fp32 ops are half rate on gfx950).
#include <hip/hip_runtime.h>

#include "detmath.h"
#include "device_types.h"
#include "device_math.h"
#include "device_intersect.h"
#include "device_shading.h" // (defaults SRT_TEXTURED to 0)

// Albedo textures: kernels_tex.hip compiles this text a second time with SRT_TEXTURED set, under the names
// below and with the texture tables behind the kernels' parameters; what only that build has sits between `#if SRT_TEXTURED`
// and its `#endif` (device_shading.h, trace_body.inc, features_body.inc). With the macro unset this file preprocesses to
// what it was before textures: a template parameter or a shared __device__ function in their place reschedules the
// untextured kernels.
#if SRT_TEXTURED
#define SRT_TRACE_PARAMS TexTraceParams
#define SRT_FEATURE_PARAMS TexFeatureParams
#define srt_trace_kernel srt_trace_tex_kernel
#define srt_features_kernel srt_features_tex_kernel
#define srt_features_ids_kernel srt_features_ids_tex_kernel
#define srt_features_tris_kernel srt_features_tris_tex_kernel
#define srt_launch_trace srt_launch_trace_tex
#define srt_trace_resident_waves_per_cu srt_trace_tex_resident_waves_per_cu
#define srt_launch_features srt_launch_features_tex
#define srt_launch_features_ids srt_launch_features_ids_tex
#define srt_launch_features_tris srt_launch_features_tris_tex
int srt_trace_lds_floats(int has_models, int use_bvh);
#else
#define SRT_TRACE_PARAMS TraceParams
#define SRT_FEATURE_PARAMS FeatureParams
#endif

// ---------------------------------------------------------------------------------
// Trace kernel. 64-thread workgroups = one persistent wave pulling (pixel, sample) items.
// ---------------------------------------------------------------------------------
// The wave alternates between TWO phases that each run on (nearly) all 64 lanes:
//   EXTEND  closest_intersection for every lane that holds a ray;
//   SHADE   the bounce of 64 paths that hit something.
// Rays that escape go to the sky ring (resolved 64 at a time). Rays that hit are shaded
// at once when, together with the paths waiting in the wave's LDS hit queue, they fill
// the wave; the lanes freed by escapes take waiting paths from the queue. Otherwise the hits
// are PARKED in the queue, every lane is free, and all 64 take new camera rays. Either way
// no phase runs for a fraction of the lanes (before: the shading of ~41 hits ran with the
// other lanes masked off in every iteration, and a lane that freed up set up its camera ray
// through an LDS staging slot).
//
// A path that ends stores its 12 bytes of radiance itself (store_radiance below; rounds 1-3 staged sub-jobs of 64 items in
// LDS and wrote whole lines). SUB-JOBS of 64 consecutive items remain the unit in which a wave's chunk is handed to its
// lanes: one scalar division per sub-job places it in the frame, and a lane's pixel is that pixel or the next one.
#ifndef SRT_SUB_PLAIN
#define SRT_SUB_PLAIN 64
#endif
#ifndef SRT_SUB_MODELS
#define SRT_SUB_MODELS 64
#endif
#ifndef SRT_SUB_BVH
#define SRT_SUB_BVH 64 // (round 2 measured 128 faster -- with chunks of 5 sub-jobs: it was the chunk, not the sub-job; trace_plan.h)
#endif
// SHADE runs when hits + queued paths reach this many lanes (64 = always a full wave)
#ifndef SRT_SHADE_MIN
#define SRT_SHADE_MIN 64
#endif
// paths the hit queue holds; when hits + queued paths exceed it they are shaded even if they do not fill the wave. 64: a phase's
// hits can always be parked, so SHADE runs with a full wave except at the end of a launch (round 4, in the LDS the radiance
// staging buffers used to take; with 40, every phase of 41..63 ready paths was shaded as it was: 59.4 lanes per SHADE phase
// and 59.3 rays per EXTEND phase, now 63.9 and 62.8 -- 5.5 % fewer loop iterations for the same rays)
#ifndef SRT_HQ_CAP
#define SRT_HQ_CAP 64
#endif
#ifndef SRT_HQ_CAP_MODELS
#define SRT_HQ_CAP_MODELS 64 // (40 / 48 / 56 / 64 at full size: configs[2] array scan 103.3 / 103.1 / 103.2 / 103.2 ms -- the scan does not care)
#endif
// Array-scan kernels: a model of at least this many triangles ("big", scene_prep.cpp packs it alone in its block) is not
// scanned by the few lanes whose rays happen to enter its box in one EXTEND phase; those rays wait in one of the
// wave's two scan stacks (the host deals the big models out to them) until SRT_SCAN_FULL of them have gathered.
#ifndef SRT_SCAN_SUSPEND_MIN
#define SRT_SCAN_SUSPEND_MIN 128
#endif
// a scan stack is taken back -- by ALL lanes of the wave; the rays they hold meanwhile are parked -- once it holds this many rays
#ifndef SRT_SCAN_FULL
#define SRT_SCAN_FULL 64
#endif
#ifndef SRT_HQ_CAP_BVH
#define SRT_HQ_CAP_BVH 64 // (40 / 48 / 56 / 64: configs[2] BVH 34.9 / 34.6 / 34.6 / 34.3 ms, configs[4] BVH 34.6 / 34.7 / 34.5 / 34.1)
#endif
// entries of the sky ring (<= 64): the ring is resolved when full, one entry per lane
#ifndef SRT_RING_CAP
#define SRT_RING_CAP 64
#endif
// new camera rays are only set up when at least this many lanes are free
#ifndef SRT_REFILL_MIN
#define SRT_REFILL_MIN 32
#endif

// Development aid (-DSRT_PHASE_CLOCK): per-wave cycles spent in each phase of the main loop, summed into the wave's
// counter line (slots 8..15: extend, ring, shade, park, deliver, refill, spare, total); srt_debug_counters reports them.
#ifdef SRT_PHASE_CLOCK
#define SRT_CLK_DECL unsigned long long clk_t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, clk_last = __builtin_amdgcn_s_memtime(), clk_start = clk_last
#define SRT_CLK(i)                                                  \
	do {                                                            \
		const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
		clk_t[i] += now_ - clk_last;                                \
		clk_last = now_;                                            \
	} while (0)
#else
#define SRT_CLK_DECL
#define SRT_CLK(i)
#endif

// Radiances leave the kernel one path at a time: a path that ends stores its 12 bytes itself (round 4). Rounds 1-3 staged the
// 64 radiances of a sub-job in LDS and wrote whole 64-byte lines; that cost 1.5 KB of LDS per wave, a flush per sub-job, two
// votes per hand-in, and a store of its own for the 8 % of paths that outlived their buffer anyway. Without it the hit queue
// holds 64 paths in the same LDS (every SHADE phase runs with a full wave), and the kernel is faster at the same bytes:
// configs[1] 122.5 -> 114.4 ms (profiles/README.md, round 4). The stores are write-through (sc1): nothing stays dirty in an
// L2, so a line whose other items arrive later is not read back for ownership (plain / sc1 / nt at full size with the queue
// of 64: 116.7 / 114.4 / - ms; with the queue of 40: 122.6 / 120.9 / 122.3). Each item is stored exactly once, by whichever wave ends
// its path (the array scan's ray pool hands paths between waves), and read by srt_reduce_kernel after the launch.
namespace {
__device__ __forceinline__ void store_radiance(float *__restrict__ radiance, uint32_t item, f3 c) {
	typedef float f3v __attribute__((ext_vector_type(3)));
	f3v v;
	v.x = c.x, v.y = c.y, v.z = c.z;
	float *g = radiance + 3ull * item;
	asm volatile("global_store_dwordx3 %0, %1, off sc1" : : "v"(g), "v"(v) : "memory");
}

// ---- lane sets as wave-uniform masks (round 4) --------------------------------------------------------------------------------
// Which lanes hold a ray, hit, escaped, ended ... lives in scalar registers as 64-bit masks. A divergent region is entered
// with in_mask(m) (llvm.amdgcn.inverse.ballot: the mask becomes the exec mask as it is), counts are s_bcnt1, ranks v_mbcnt, set
// algebra is scalar. Rounds 1-3 kept per-lane bools across the phases of the main loop: every vote on such a bool is a
// v_cndmask + v_cmp pair, every merge of two of them a chain of scalar mask instructions, and none of it is free -- measured in
// place (scripts/r04_issue_cost.sh, profiles/r04_issue_cost.json) a scalar instruction costs the launch 1.0-1.3 v_add_f32.
__device__ __forceinline__ bool in_mask(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__builtin_popcountll(m); }
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m) { // set bits of m below this lane
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ unsigned long long lanes_below(uint32_t n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); } // lanes 0 .. n-1

// Evaluate the sky for the first n queued escapes (n <= 64), one per lane, and finish their
// paths: mask *= sky; color += mask (render.cl:464-465). Called with all 64 lanes in
// wave-uniform control flow.
__device__ __forceinline__ void resolve_ring(const TraceParams &p, const float *__restrict__ ring, uint32_t n, int lane SRT_RC_PARAM) {
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	if ((uint32_t)lane < n) {
		SRT_REGION(SKY_RESOLVE);
		constexpr uint32_t RC = SRT_RING_CAP;
		const f3 d = mk(ring[0 * RC + lane], ring[1 * RC + lane], ring[2 * RC + lane]);
		f3 m = mk(ring[3 * RC + lane], ring[4 * RC + lane], ring[5 * RC + lane]);
		f3 c = mk(ring[6 * RC + lane], ring[7 * RC + lane], ring[8 * RC + lane]);
		const uint32_t item = dm_f2u(ring[9 * RC + lane]);
		m = m * sky_box(p, d);
		c = c + m;
		store_radiance(p.radiance, item, c);
	}
	asm volatile("" ::: "memory");
}
} // namespace

// Waves per SIMD the register allocator is asked for. LDS per wave (sky ring, hit queue, scene records: 7.4 KB in sphere /
// plane scenes) bounds residency at 21 per CU; the sphere kernel's 78 VGPRs would allow a sixth wave per SIMD.
#ifndef SRT_TRACE_WAVES_PER_SIMD
#define SRT_TRACE_WAVES_PER_SIMD 5
#endif
#ifndef SRT_TRACE_WAVES_PER_SIMD_MODELS
#define SRT_TRACE_WAVES_PER_SIMD_MODELS 5
#endif
#ifndef SRT_TRACE_WAVES_PER_SIMD_BVH
#define SRT_TRACE_WAVES_PER_SIMD_BVH 5 // (4: configs[2] 42.0 ms, configs[4] 38.0 ms; 5: 40.8 / 36.5 -- the walk waits for memory, a fifth wave fills the gaps)
#endif

// Fields of a hit-queue entry (hq in the trace kernel): org, dir, mask, color, seed, best, bounce, item, and best_tri in scenes
// with models. srt_trace_lds_floats sizes the queue with it, and -DSRT_REGION_COUNT builds put their counters behind it.
constexpr uint32_t hq_fields(bool has_models) { return has_models ? 17u : 16u; }

// HAS_MODELS = false compiles every AABB / triangle / mesh-normal path out: scenes of
// spheres and planes (BASELINE configs 0, 1, 3) get a leaner kernel; the host picks the
// instantiation from the scene.
//
// SCENE CLASSES. What is the same for every ray of a launch and fixed when the scene is set -- how many groups of shape blocks
// there are, what each block holds, whether every shape has a material, what the materials rule out -- the general kernel
// decides with scalar code in every iteration of its loop: a fifth of its issue slots. The body (trace_body.inc) is
// written once and compiled per class `SC`: GeneralScene leaves every such decision where it was (the ten
// srt_trace_kernel instantiations: their code is what it was before classes existed), OneGroupScene<CODE, NO_SPEC> makes
// them constants. The host names the class of a dispatch (srt_abi.hip scene_class(), device_types.h SRT_SCENE_CLASS_LIST);
// a scene outside every listed class runs the general kernel.
struct GeneralScene {
	static constexpr bool FAST = false, NO_SPEC = false;
	static constexpr uint32_t CODE = 0, AXES = 0;
};
// A sphere / plane scene of ONE group whose header is CODE (device_types.h BlockGroup: per block, type and shape count), staged
// in LDS, shapes 0 .. N - 1 in the blocks in array order, every shape with a material, the materials' probabilities as
// thresholds (unit_materials), num_bounces > 0, show_normals off. NO_SPEC: no material is specular and every colour is plain
// (SRT_MF_NO_SPECULAR | SRT_MF_PLAIN_COLORS). AXES: the scene's plane form (device_types.h "Axis planes"); 0 = the class's own
// kernel, whose planes are general ones.
template <uint32_t CODE_, bool NO_SPEC_, uint32_t AXES_ = 0>
struct OneGroupScene {
	static constexpr bool FAST = true, NO_SPEC = NO_SPEC_;
	static constexpr uint32_t CODE = CODE_, AXES = AXES_;
	static_assert(AXES_ == 0 || srt_axes_buildable(CODE_, AXES_), "an axis twin needs an axis for every plane, and all three axes in use");
};
// one block of a OneGroupScene: test_block of the general kernel with the block's byte of the header a constant
template <uint32_t K>
__device__ __forceinline__ void test_block_of_class(const Blk16 &b, int base, f3 org, f3 dir, float &tmin, int &best) {
	if constexpr ((K & 3u) == SRT_SHAPE_SPHERE + 1u) {
		if constexpr (((K >> 2) & 7u) <= 2u) test_spheres<2>(b, org, dir, base, tmin, best);
		else test_spheres<4>(b, org, dir, base, tmin, best);
	} else if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		test_planes2(b, (K >> 2) & 7u, org, dir, base, tmin, best);
	}
}
// the same block in a phase of fresh camera rays only (device_intersect.h "CAMERA PHASES"): blk = the staged block, cam = its spheres' records
template <uint32_t K>
__device__ __forceinline__ void test_block_of_class_cam(const float4 *__restrict__ blk, const float4 *__restrict__ cam, int base, f3 dir, unsigned long long actm, float &tmin, int &best) {
	if constexpr ((K & 3u) == SRT_SHAPE_SPHERE + 1u) {
		if constexpr (((K >> 2) & 7u) <= 2u) test_spheres_cam<2>(cam, dir, actm, base, tmin, best);
		else test_spheres_cam<4>(cam, dir, actm, base, tmin, best);
	} else if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		test_planes2_cam(blk, (K >> 2) & 7u, dir, base, tmin, best);
	}
}

// A block of an axis twin (device_intersect.h "AXIS PLANES"): blk = the staged block, a = its planes' numerators, pass = the
// phase's guard held for every ray of the wave (wave-uniform). A plane block then runs the folded tests, else today's; a sphere
// block is what it is in the class's own kernel.
__device__ __forceinline__ Blk16 ld_blk16_lds(const float4 *__restrict__ blk) {
	Blk16 b;
	const float4 q0 = blk[0], q1 = blk[1], q2 = blk[2], q3 = blk[3];
	b.v[0] = q0.x, b.v[1] = q0.y, b.v[2] = q0.z, b.v[3] = q0.w, b.v[4] = q1.x, b.v[5] = q1.y, b.v[6] = q1.z, b.v[7] = q1.w;
	b.v[8] = q2.x, b.v[9] = q2.y, b.v[10] = q2.z, b.v[11] = q2.w, b.v[12] = q3.x, b.v[13] = q3.y, b.v[14] = q3.z, b.v[15] = q3.w;
	return b;
}
template <uint32_t K, uint32_t AX>
__device__ __forceinline__ void test_block_of_class_axis(const float4 *__restrict__ blk, bool pass, const float *__restrict__ a, int base, f3 org, f3 dir, float &tmin, int &best) {
	if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		if (__builtin_expect(pass, 1)) test_planes2_axis<AX>(a, (K >> 2) & 7u, dir, base, tmin, best);
		else test_planes2(ld_blk16_lds(blk), (K >> 2) & 7u, org, dir, base, tmin, best); // @rare
	} else {
		test_block_of_class<K>(ld_blk16_lds(blk), base, org, dir, tmin, best);
	}
}
template <uint32_t K, uint32_t AX>
__device__ __forceinline__ void test_block_of_class_axis_cam(const float4 *__restrict__ blk, const float4 *__restrict__ cam, bool pass, int base, f3 dir, unsigned long long actm, float &tmin, int &best) {
	if constexpr ((K & 3u) == SRT_SHAPE_PLANE + 1u) {
		if (__builtin_expect(pass, 1)) {
			const float a[2] = {reinterpret_cast<const float *>(blk + 1)[3], reinterpret_cast<const float *>(blk + 3)[3]}; // the prologue's (cam_axis_numerators)
			test_planes2_axis<AX>(a, (K >> 2) & 7u, dir, base, tmin, best);
		} else {
			test_planes2_cam(blk, (K >> 2) & 7u, dir, base, tmin, best); // @rare
		}
	} else {
		test_block_of_class_cam<K>(blk, cam, base, dir, actm, tmin, best);
	}
}

template <bool COUNT_TRIS, bool USE_LDS, bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64, USE_BVH ? SRT_TRACE_WAVES_PER_SIMD_BVH : HAS_MODELS ? SRT_TRACE_WAVES_PER_SIMD_MODELS : SRT_TRACE_WAVES_PER_SIMD) void srt_trace_kernel(const SRT_TRACE_PARAMS p) {
	using SC = GeneralScene;
#include "trace_body.inc"
}

// The scene classes are built where the general kernel is the product's own: not in the textured twin, not in the
// instrumented builds (their counters and clocks describe the general kernel), not with the development knobs, and with
// the sky ring one wave wide (SKY_PUSH's one-round form).
#if !SRT_TEXTURED && !SRT_DIAG_ON && !defined(SRT_DUMMY_KIND) && !defined(SRT_DEV_KNOBS) && SRT_RING_CAP == 64
#define SRT_SCENE_CLASSES 1
// (six waves per SIMD asked of the register allocator: at most 80 VGPRs, the general sphere kernel's allocation, so that the
// 21 waves per CU the LDS allows stay resident -- with five, the specular class took 81)
template <uint32_t CODE, bool NO_SPEC, uint32_t PLANE_FORM>
__global__ __launch_bounds__(64, 6) void srt_trace_scene_kernel(const TraceParams p) {
	constexpr bool COUNT_TRIS = false, USE_LDS = true, HAS_MODELS = false, USE_BVH = false;
	using SC = OneGroupScene<CODE, NO_SPEC, PLANE_FORM>;
#include "trace_body.inc"
}
#else
#define SRT_SCENE_CLASSES 0
#endif

// ---------------------------------------------------------------------------------
// Denoiser guide buffers (device_types.h FeatureParams; the filter is csrc/denoise.hip). One lane = one pixel, its first
// feature_samples camera rays one after the other: the trace kernel's seed, jitter and camera matrix (trace_body.inc CAMERA), its
// closest_intersection (EXTEND there: the same block order and the same tests, so the same closest hit) and its winner
// normal (SHADE_WINNER). Not wave-coherent and not persistent: under SRT_ACCEL_NONE a big model costs every pixel's ray
// a brute-force scan of the model's triangles once per feature sample (DESIGN.md "Denoiser"); with a hierarchy each lane
// walks it with a stack of its own.
// ---------------------------------------------------------------------------------
template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_features_kernel(const SRT_FEATURE_PARAMS fp) {
#define SRT_FEATURES_IDS 0
#include "features_body.inc"
#undef SRT_FEATURES_IDS
}

// the same, and the shape index per pixel for the temporal stage's object motion (temporal.hip)
template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_features_ids_kernel(const SRT_FEATURE_PARAMS fp, uint32_t *__restrict__ shape_ids) {
#define SRT_FEATURES_IDS 1
#include "features_body.inc"
#undef SRT_FEATURES_IDS
}

// the same, and the hit triangle's index inside its model for the temporal stage's per-triangle motion (temporal.hip)
template <bool HAS_MODELS, bool USE_BVH>
__global__ __launch_bounds__(64) void srt_features_tris_kernel(const SRT_FEATURE_PARAMS fp, uint32_t *__restrict__ shape_ids, uint32_t *__restrict__ tri_ids) {
#define SRT_FEATURES_IDS 2
#include "features_body.inc"
#undef SRT_FEATURES_IDS
}

// ---------------------------------------------------------------------------------
// launch wrappers (host)
// ---------------------------------------------------------------------------------
#if !SRT_TEXTURED // what the host asks of the tunables above, once for both compilations (the other fence left: the scene-class kernels above)
int srt_trace_waves_per_simd(int has_models, int use_bvh) {
	return !has_models ? SRT_TRACE_WAVES_PER_SIMD : use_bvh ? SRT_TRACE_WAVES_PER_SIMD_BVH : SRT_TRACE_WAVES_PER_SIMD_MODELS;
}
int srt_scan_suspend_min(void) { return SRT_SCAN_SUSPEND_MIN; }
int srt_sub_job_items(int has_models, int use_bvh) { return !has_models ? SRT_SUB_PLAIN : use_bvh ? SRT_SUB_BVH : SRT_SUB_MODELS; }

int srt_trace_lds_floats(int has_models, int use_bvh) {
	// the sky ring (10 fields), the hit queue
	int n = 10 * SRT_RING_CAP + (int)hq_fields(has_models) * (has_models ? (use_bvh ? SRT_HQ_CAP_BVH : SRT_HQ_CAP_MODELS) : SRT_HQ_CAP);
#ifdef SRT_REGION_COUNT
	n += 2 * SRT_REGION_MAX; // (waves, lanes) per region
#endif
	return n;
}
// whether this build has the scene classes at all (the textured, instrumented and development builds do not)
int srt_trace_has_scene_classes() { return SRT_SCENE_CLASSES; }
#endif

namespace {
typedef void (*TraceKernel)(const SRT_TRACE_PARAMS);
TraceKernel pick_trace_kernel(bool models, bool use_bvh, bool use_lds, bool count_triangles) {
	if (!models) return use_lds ? srt_trace_kernel<false, true, false, false> : srt_trace_kernel<false, false, false, false>;
	if (use_bvh) {
		if (use_lds) return count_triangles ? srt_trace_kernel<true, true, true, true> : srt_trace_kernel<false, true, true, true>;
		return count_triangles ? srt_trace_kernel<true, false, true, true> : srt_trace_kernel<false, false, true, true>;
	}
	if (use_lds) return count_triangles ? srt_trace_kernel<true, true, true, false> : srt_trace_kernel<false, true, true, false>;
	return count_triangles ? srt_trace_kernel<true, false, true, false> : srt_trace_kernel<false, false, true, false>;
}
// winners + materials go to LDS when small enough not to cost occupancy
size_t scene_lds_bytes(const TraceParams &p) {
	return srt_scene_lds_bytes((size_t)p.sd.num_shapes, (size_t)p.num_materials, p.num_models, (size_t)p.num_runs);
}
// the kernel of a launch: its scene class's, or the general instantiation for the scene's kind
TraceKernel pick_trace_kernel(const SRT_TRACE_PARAMS &p, bool use_lds, bool count_triangles) {
#if SRT_SCENE_CLASSES
	switch (p.scene_class) { // (srt_kernel_key: a class's own kernel has plane form 0)
#define SRT_SCENE_CLASS_CASE(number, code, no_spec) \
	case number: return srt_trace_scene_kernel<code, no_spec, 0u>;
		SRT_SCENE_CLASS_LIST(SRT_SCENE_CLASS_CASE)
#undef SRT_SCENE_CLASS_CASE
#define SRT_SCENE_AXIS_CASE(number, code, no_spec, axes) \
	case srt_kernel_key(number, axes): return srt_trace_scene_kernel<code, no_spec, axes>;
		SRT_SCENE_AXIS_LIST(SRT_SCENE_AXIS_CASE)
#undef SRT_SCENE_AXIS_CASE
	default: break;
	}
#endif
	return pick_trace_kernel(p.num_models > 0, p.use_bvh != 0, use_lds, count_triangles);
}
// dynamic LDS of a launch: the scene records, the per-wave queues and, for a scene class, its camera records (device_intersect.h "CAMERA PHASES")
size_t trace_lds_bytes(const SRT_TRACE_PARAMS &p, size_t scene_lds) {
	size_t need = scene_lds + (size_t)srt_trace_lds_floats(p.num_models > 0, p.use_bvh) * sizeof(float);
#if SRT_SCENE_CLASSES
	switch (srt_key_class(p.scene_class)) {
#define SRT_SCENE_CLASS_CASE(number, code, no_spec) \
	case number: need += srt_class_cam_lds_bytes(code); break;
		SRT_SCENE_CLASS_LIST(SRT_SCENE_CLASS_CASE)
#undef SRT_SCENE_CLASS_CASE
	default: break;
	}
#endif
	return need;
}
} // namespace

// Persistent waves (= one-wave workgroups) of this launch configuration that one CU holds at once, as the runtime
// computes it from the kernel's registers and its dynamic LDS; the grid must not exceed CUs x this, or the surplus
// waves would only start -- each with a first chunk of its own -- when others have drained the queue.
int srt_trace_resident_waves_per_cu(const SRT_TRACE_PARAMS &p, bool count_triangles) {
	const size_t scene_lds = scene_lds_bytes(p);
	const size_t need = trace_lds_bytes(p, scene_lds);
	int blocks = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, pick_trace_kernel(p, scene_lds != 0, count_triangles), 64, need) != hipSuccess ||
	    blocks <= 0) {
		(void)hipGetLastError();
		blocks = 4 * srt_trace_waves_per_simd(p.num_models > 0, p.use_bvh);
	}
	return blocks;
}

void srt_launch_trace(SRT_TRACE_PARAMS p, bool count_triangles, int num_waves, void *stream) {
	if (p.total_items == 0 || num_waves <= 0) return;
	dim3 grid((unsigned)num_waves), block(64);
	const size_t scene_lds = scene_lds_bytes(p);
	p.lds_bytes = (uint32_t)scene_lds;
	p.stage_off = (uint32_t)(scene_lds / sizeof(float4));
	const size_t need = trace_lds_bytes(p, scene_lds);
	hipLaunchKernelGGL(pick_trace_kernel(p, scene_lds != 0, count_triangles), grid, block, need, (hipStream_t)stream, p);
}

void srt_launch_features(const SRT_FEATURE_PARAMS &p, void *stream) {
	if (p.num_pixels == 0 || p.feature_samples == 0) return;
	typedef void (*FeatureKernel)(const SRT_FEATURE_PARAMS);
	const bool models = p.tp.num_models > 0, bvh = p.tp.use_bvh != 0;
	const FeatureKernel k = !models ? srt_features_kernel<false, false> : bvh ? srt_features_kernel<true, true> : srt_features_kernel<true, false>;
	hipLaunchKernelGGL(k, dim3((p.num_pixels + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, p);
}

void srt_launch_features_ids(const SRT_FEATURE_PARAMS &p, uint32_t *shape_ids, void *stream) {
	if (p.num_pixels == 0 || p.feature_samples == 0) return;
	typedef void (*FeatureKernel)(const SRT_FEATURE_PARAMS, uint32_t *);
	const bool models = p.tp.num_models > 0, bvh = p.tp.use_bvh != 0;
	const FeatureKernel k = !models ? srt_features_ids_kernel<false, false> : bvh ? srt_features_ids_kernel<true, true> : srt_features_ids_kernel<true, false>;
	hipLaunchKernelGGL(k, dim3((p.num_pixels + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, p, shape_ids);
}

void srt_launch_features_tris(const SRT_FEATURE_PARAMS &p, uint32_t *shape_ids, uint32_t *tri_ids, void *stream) {
	if (p.num_pixels == 0 || p.feature_samples == 0) return;
	typedef void (*FeatureKernel)(const SRT_FEATURE_PARAMS, uint32_t *, uint32_t *);
	const bool models = p.tp.num_models > 0, bvh = p.tp.use_bvh != 0;
	const FeatureKernel k = !models ? srt_features_tris_kernel<false, false> : bvh ? srt_features_tris_kernel<true, true> : srt_features_tris_kernel<true, false>;
	hipLaunchKernelGGL(k, dim3((p.num_pixels + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, p, shape_ids, tri_ids);
}
