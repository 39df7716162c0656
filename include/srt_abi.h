/* srt_abi.h — the C ABI of the MI355X path-tracing library (libsrt_hip.so).
 *
 * It replaces exactly one thing in the reference: the boost.compute/OpenCL dispatch
 * inside `class Tracer` (/root/reference/include/tracer.hpp:26-88,
 * /root/reference/src/tracer.cpp:11-116). Every entry point names the reference
 * member it stands in for. Records are passed as raw bytes in the layouts of
 * srt_types.h. Plain pointers and sizes only: no C++ types, no torch types.
 *
 * Status codes: 0 = ok, anything else = failure; srt_last_error() returns the text
 * (the C++ wrapper simple-raytracer_amd/host/tracer.hpp turns it into an exception,
 * as boost.compute throws in the reference, src/tracer.cpp:20-26).
 *
 * Threading: a handle is NOT thread-safe (the reference drives its Tracer from the
 * SDL main thread only). All device work of a handle is ordered on one HIP stream.
 */
#ifndef SRT_ABI_H
#define SRT_ABI_H

#include "srt_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srt_tracer srt_tracer; /* opaque */

enum {
	SRT_OK = 0,
	SRT_ERR_INVALID = 1, /* bad argument */
	SRT_ERR_HIP = 2,     /* a HIP runtime call failed (no device, OOM, launch error) */
	SRT_ERR_STATE = 3    /* call order violated (e.g. render before a skybox exists) */
};

/* Deterministic work counters of the trace kernel, summed over all render calls since
 * the last srt_reset_counters(). Schedule independent; equal to the oracle's. */
typedef struct srt_counters {
	uint64_t paths;      /* (pixel, sample) pairs traced */
	uint64_t rays;       /* closest-hit queries = path segments (render.cl:404) */
	uint64_t sky;        /* segments that escaped to the sky (render.cl:463-467) */
	uint64_t tri_tests;  /* triangle tests executed (render.cl:331) */
	uint64_t tri_pass_u; /* triangle tests that passed the u-range check (render.cl:260) */
	uint64_t nan_pixels; /* pixels whose colour of a dispatch was NaN */
	uint64_t watchdog;   /* waves that left the work loop through its spin bound; must be 0 */
} srt_counters;

/* ---- life cycle ------------------------------------------------------------- */

/* Tracer::Tracer(width, height) — src/tracer.cpp:11-68. Selects HIP device
 * `device_index`, creates the stream, the float3 canvas (16 B/pixel) and the ARGB8
 * output buffer. width/height are fixed for the life of the handle (no resize). */
int srt_create(int width, int height, int device_index, srt_tracer **out);

/* ~Tracer (implicit in the reference). */
void srt_destroy(srt_tracer *t);

/* Text of the last failure on this handle (or of srt_create when t == NULL). */
const char *srt_last_error(const srt_tracer *t);

/* ---- inputs ------------------------------------------------------------------ */

/* The skybox upload of src/tracer.cpp:42-55, minus the PNG decode: `rgba` is the
 * RGBA32F image stb would have produced (row 0 = bottom after the vertical flip),
 * width*height*4 floats. Sampled like CL_ADDRESS_CLAMP_TO_EDGE | CL_FILTER_LINEAR with
 * normalized coordinates (src/tracer.cpp:47-48) in exact float arithmetic. */
int srt_set_skybox(srt_tracer *t, const float *rgba, int width, int height);

/* Tracer::update_scene — src/tracer.cpp:70-96. Copies the three arrays (any may be
 * empty: an empty scene renders pure sky) and latches *scene (SceneData reaches the
 * kernel only here, never in render). scene->num_shapes is overwritten by n_shapes,
 * as src/tracer.cpp:94 does. Also runs the world-space triangle pre-pass. */
int srt_update_scene(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles,
                     size_t n_triangles, const srt_material *materials, size_t n_materials,
                     const srt_scene_data *scene);

/* Acceleration structure for model shapes (new; the reference's first "future plan",
 * README.md:41). Takes effect at the NEXT srt_update_scene.
 *   SRT_ACCEL_NONE (default): every triangle of a model whose box the ray enters is tested
 *       in array order, as render.cl:329-345 -- the parity mode.
 *   SRT_ACCEL_BVH: srt_update_scene builds one bounding-volume hierarchy per model instance
 *       (host, binned SAH) and rays walk it instead of the array. Same triangle test, same
 *       first-in-array-order rule for hits of equal distance, conservative (padded) boxes:
 *       the canvas equals SRT_ACCEL_NONE's except where a grazing ray's rounding error puts
 *       an accepted hit outside its triangle's padded box (not observed on the test scenes;
 *       tests/test_gpu_bvh.py). Spheres, planes and each model's own AABB test are untouched. */
#define SRT_ACCEL_NONE 0
#define SRT_ACCEL_BVH 1
int srt_set_acceleration(srt_tracer *t, int mode);
/* out = {nodes, leaves, depth, host time spent on the hierarchies in microseconds, models built,
 * models re-used, models refitted} for the current scene (zeros without SRT_ACCEL_BVH or without
 * models). A model whose triangles are byte-identical to one of the previous srt_update_scene keeps
 * its hierarchy: as it is when its transform did not change either (camera, material, other-shape
 * edits cost no build), with new boxes around the same tree when it moved (a refit, ~10x cheaper
 * than a build). */
int srt_acceleration_info(const srt_tracer *t, uint64_t out[7]);

/* Host-only (no device needed): the hierarchy srt_update_scene builds under SRT_ACCEL_BVH for ONE
 * model shape, for inspection and tests. `model->type` must be SRT_SHAPE_MODEL and its triangle
 * range must lie inside `triangles[0 .. n_triangles)`. Writes at most nodes_cap nodes and
 * order_cap indices (order[r] = index inside the model of the triangle stored in record r;
 * leaves refer to records) and always sets *n_nodes to the number of nodes of the hierarchy;
 * either output may be NULL to only query that number. */
int srt_bvh_build_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, srt_bvh_node *nodes_out,
                       size_t nodes_cap, uint32_t *order_out, size_t order_cap, size_t *n_nodes);

/* Host-only: the WIDE form of that hierarchy, the one the kernel walks (layout: csrc/device_types.h; block indices
 * relative to the model's first block; an inner block: dwords 0-2 the origin of its grid, 3 the grid's exponents and the
 * number of children, 4-9 the children's boxes as bytes, 10 their tags, 11 the index of child 0 -- siblings lie side by side). blocks_out receives at most blocks_cap blocks
 * of 32 dwords (leaf blocks are zero here: the device writes their triangles), dest_out[r] = (leaf block << 2) | slot of record r (records as in
 * srt_bvh_build_host's order). *root = the root reference (0xffffffff for a model without triangles), *stack_need =
 * the most children a walk can have waiting at once (never above the kernel's stack of 64: a hierarchy that would
 * need more is rebuilt balanced, *balanced = 1; force_balanced != 0 asks for that form directly). */
int srt_bvh_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, int force_balanced, uint32_t *blocks_out,
                      size_t blocks_cap, uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, int *balanced);

/* Host-only: order[r] = index inside the model of the triangle in record r of the hierarchy srt_bvh_wide_host hands out for
 * the same arguments (srt_bvh_build_host's order is that of the SAH form only; the balanced form has its own). Writes at
 * most order_cap indices; the hierarchy has num_triangles records. */
int srt_bvh_wide_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, int force_balanced,
                            uint32_t *order_out, size_t order_cap);

/* Host-only: the wide hierarchy of `built` (exactly srt_bvh_wide_host's) refitted IN PLACE for `moved`: the topology it was
 * folded with is kept -- root, stack need, dest, order, every block's tags, first and child count, the number of blocks --
 * and every inner block's origin, exponents and byte boxes (dwords 0-9) are recomputed around the moved triangles. `moved`
 * must have `built`'s triangle_index and num_triangles; only its transform may differ (SRT_ERR_INVALID otherwise). Blocks
 * as srt_bvh_wide_host hands them out: relative to the model, leaf blocks zero. This is what SRT_REFIT_DEVICE (below)
 * computes on the device, bit for bit. */
int srt_bvh_refit_wide_host(const srt_shape *built, const srt_shape *moved, const srt_triangle *triangles, size_t n_triangles,
                            int force_balanced, uint32_t *blocks_out, size_t blocks_cap, size_t *n_blocks, uint32_t *root);

/* Who refits the hierarchy of a model that only MOVED between two srt_update_scene calls (same triangle bytes, another
 * transform). SRT_REFIT_HOST, the default: the host recomputes the boxes, folds and quantises them again and uploads the
 * result, as ever. SRT_REFIT_DEVICE: the host keeps the hierarchy's topology and uploads it as it is; kernels on the
 * handle's stream, behind the pre-pass, recompute the triangles' boxes, the leaf blocks' boxes and, level by level from
 * the leaves up, every inner block's byte boxes -- the bytes srt_bvh_refit_wide_host gives. Because the fold is kept where
 * the host path re-folds, the two hierarchies can differ in shape after a rotation; the walk's result does not depend on
 * the visiting order, so the canvas is the same. Takes effect at the next srt_update_scene; accepted and without effect
 * under SRT_ACCEL_NONE. The group form sets every member. */
#define SRT_REFIT_HOST 0
#define SRT_REFIT_DEVICE 1
int srt_set_acceleration_refit(srt_tracer *t, int mode);
/* out = {models refitted on the device by the last srt_update_scene, inner blocks they requantised, refit launches
 * enqueued, 0}. A model counts whenever its blocks were uploaded from a hierarchy whose boxes the host no longer keeps
 * current, also in a call in which it did not move itself. srt_acceleration_info's out[6] counts the models that moved,
 * whoever refitted them. */
int srt_acceleration_refit_info(const srt_tracer *t, uint64_t out[4]);
/* With srt_set_kernel_timers on: the device time of the last srt_update_scene's refit launches, first to last, in
 * milliseconds (0 when it enqueued none or the timers were off); under SRT_DEFORM_REFIT (below) the cost launch with its
 * small copies is inside the span. Blocking. */
int srt_last_refit_kernel_ms(srt_tracer *t, float *ms);
/* What becomes of a model whose VERTICES changed between two srt_update_scene calls (a skinned character, a cloth step, a morph
 * target, a sculpt stroke). SRT_DEFORM_REBUILD, the default: its hierarchy is built anew, as ever. SRT_DEFORM_REFIT: a model
 * that finds no hierarchy of byte-identical triangles takes an unclaimed one of the previous call with its triangle_index and
 * num_triangles -- after every model of the call has claimed its byte-identical one -- and keeps that tree: the topology and
 * the records' order stay, every box is recomputed around the new triangles, by SRT_REFIT_HOST or SRT_REFIT_DEVICE exactly as
 * for a model that moved (the transform may change in the same call). Another count or another range still builds. Nothing
 * checks that the mesh's connectivity is what it was: the canvas does not depend on the tree's shape (closest hit, first in
 * array order among equals), only the trace time does. To bound that, every refit under this mode measures the tree:
 *   cost = (sum over inner blocks H(box) * children + sum over leaf blocks H(box) * triangles) / H(root box),
 *   H(b) = dx * dy + dy * dz + dz * dx in double, extents as (double)hi - (double)lo of the padded float boxes
 * -- on the device one more launch behind the refit, summed per wave and read back asynchronously; on the host under
 * SRT_REFIT_HOST. ratio = cost now / cost of the tree as built; unknown (reported as 0, never a reason to rebuild) when a root
 * has H == 0 or a term is not finite. rebuild_ratio: 0 = never rebuild on cost; a finite value > 1 = a model whose vertices
 * changed and whose last known ratio is above it is built anew instead (its ratio is 1 again). SRT_ERR_INVALID for another
 * mode or ratio. Takes effect at the next srt_update_scene; accepted and without effect under SRT_ACCEL_NONE. */
#define SRT_DEFORM_REBUILD 0
#define SRT_DEFORM_REFIT 1
int srt_set_acceleration_deform(srt_tracer *t, int mode, float rebuild_ratio);
/* Of the last srt_update_scene: out = {models whose hierarchy was kept across a change of triangle bytes (they count in
 * srt_acceleration_info's out[6], refitted, not in out[4], built), models built anew because their ratio was above
 * rebuild_ratio (they count in out[4]), cost launches enqueued, 0}; *worst_ratio = the largest known cost ratio among the
 * scene's models, 0 when none is known (always under SRT_DEFORM_REBUILD). Waits for the last update's cost read-back, not for
 * the stream. */
int srt_acceleration_deform_info(srt_tracer *t, uint64_t out[4], double *worst_ratio);
/* Host-only: srt_bvh_refit_wide_host for a model whose triangles changed too. The wide hierarchy of `built` over
 * built_triangles, refitted in place around `now` over now_triangles (both arrays of n_triangles entries; `now` must have
 * `built`'s triangle_index and num_triangles, its transform may differ). With now_triangles == built_triangles these are
 * srt_bvh_refit_wide_host's bytes. What SRT_DEFORM_REFIT with SRT_REFIT_DEVICE leaves on the device, bit for bit. */
int srt_bvh_refit_deformed_wide_host(const srt_shape *built, const srt_triangle *built_triangles, const srt_shape *now,
                                     const srt_triangle *now_triangles, size_t n_triangles, int force_balanced, uint32_t *blocks_out,
                                     size_t blocks_cap, size_t *n_blocks, uint32_t *root);
/* Host-only: the cost (above) of that hierarchy as built and as refitted in place; 0 = unknown (also: a model without
 * triangles). The device's sum takes its terms in another order: it agrees within n_blocks * 2^-53 relative. */
int srt_bvh_wide_cost_host(const srt_shape *built, const srt_triangle *built_triangles, const srt_shape *now,
                           const srt_triangle *now_triangles, size_t n_triangles, int force_balanced, double *cost_built, double *cost_now);
/* Who BUILDS the hierarchy of a model that has none to keep (a new model, another triangle count, other triangle bytes without
 * SRT_DEFORM_REFIT, a rebuild that rebuild_ratio asked for). SRT_BUILD_HOST, the default: the binned-SAH build on the host, as
 * ever. SRT_BUILD_DEVICE: a model of at least min_triangles triangles (0: every model) gets the BALANCED topology of its count
 * -- halves by record index down to leaves of three, a function of the count alone that the host keeps per count -- over the
 * MORTON order of its triangles, which kernels on the handle's stream compute before the pre-pass: the model's extents, a
 * 30-bit code per triangle, a stable radix sort by (code, index); the refit passes of SRT_REFIT_DEVICE then make every box.
 *   per triangle j: world vertices, unpadded box lo / hi and finiteness as the builder's; c[a] = 0.5f * lo[a] + 0.5f * hi[a]
 *   mlo / mhi: the model's extents over its finite triangles; per axis ext = mhi[a] - mlo[a];
 *   q[a] = ext > 0 and finite ? clamp((int)((c[a] - mlo[a]) * (1024.0f / ext)), 0, 1023) : 0   (float32, unfused, IEEE division)
 *   code: bit 3i+2 = bit i of q[x], 3i+1 of q[y], 3i of q[z]; a non-finite triangle: 0x40000000, behind every finite one
 *   order = the triangles by ascending (code, j)
 * Smaller models keep the host's build. The canvas does not depend on the tree's shape; the trace time does (a median split of a
 * 10-bit Morton order is a worse tree than the SAH's: DESIGN.md has the cost and time ratios). Afterwards such a model is
 * re-used, moved and deformed like any other; the sorted order comes back to the host asynchronously and is waited for at the
 * next srt_update_scene and in srt_acceleration_build_info. A device-built model counts in srt_acceleration_info's out[4]
 * (built); out[3] is the host's time alone. Under SRT_DEFORM_REFIT the cost launch runs behind the build and its value becomes
 * the tree's cost as built. SRT_ERR_INVALID for another mode. Takes effect at the next srt_update_scene; accepted and without
 * effect under SRT_ACCEL_NONE. */
#define SRT_BUILD_HOST 0
#define SRT_BUILD_DEVICE 1
int srt_set_acceleration_build(srt_tracer *t, int mode, uint32_t min_triangles);
/* Of the last srt_update_scene: out = {models built on the device, records sorted, build launches enqueued (extents, codes and
 * the sort's; the refit's are srt_acceleration_refit_info's), 0}. Waits for the sorted order's read-back, not for the stream. */
int srt_acceleration_build_info(srt_tracer *t, uint64_t out[4]);
/* With srt_set_kernel_timers on: the device time from the first build launch of the last srt_update_scene to the last launch of
 * the refit behind it (the pre-pass lies in between), in milliseconds; 0 when nothing was built on the device. Blocking. */
int srt_last_build_kernel_ms(srt_tracer *t, float *ms);
/* Host-only: the Morton order defined above for one model (order[r] = index inside the model of the triangle in record r).
 * Writes at most order_cap indices. */
int srt_bvh_morton_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *order_out, size_t order_cap);
/* Host-only: the wide hierarchy SRT_BUILD_DEVICE leaves on the device, bit for bit: the balanced topology over the Morton order
 * with the boxes of the in-place refit. Blocks, dest, root and stack_need as srt_bvh_wide_host hands them out (relative to the
 * model, leaf blocks zero; stack_need is at most 45); *cost = the hierarchy's cost (above; may be NULL). */
int srt_bvh_morton_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *blocks_out, size_t blocks_cap,
                             uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, double *cost);
/* The ORDER SRT_BUILD_DEVICE lays the balanced topology over. SRT_BUILD_ORDER_MORTON, the default: the Morton order above, launch
 * for launch what SRT_BUILD_DEVICE has always done. SRT_BUILD_ORDER_MEDIAN: the order the host's balanced tree is after, a
 * median split on the widest centroid axis in every range, computed top-down on the device -- more launches (about 80 for 10^5
 * triangles against 14) for a tree close to the host's balanced one instead of 2-3 times the SAH tree's cost (DESIGN.md has the
 * figures). Everything behind the order is the same: the topology cached per count, the refit passes, the cost launch, the
 * read-back. The definition, float32, unfused, in this order, with c = 0.5f * lo + 0.5f * hi of the unpadded box as above:
 *   start from the identity order; for every range [b, e) of the balanced topology with n = e - b > 3, top-down (its halves
 *   are [b, b + n / 2) and [b + n / 2, e)), before its halves are visited:
 *     clo[a], chi[a] = min, max of c[a] over the range's finite triangles (FLT_MAX, -FLT_MAX without any); ext[a] = chi[a] - clo[a]
 *     a = 0; for k = 1, 2: if (ext[k] > ext[a]) a = k
 *     key = 0 where ext[a] is not a positive finite number, else with f = (c[a] - clo[a]) * (65536.0f / ext[a]):
 *           f >= 65535 ? 65535 : (f > 0 ? (uint32_t)(int)f : 0); a non-finite triangle: 0x10000
 *     the range is sorted STABLY by key
 * A model of more than 1,024 << 15 = 33,554,432 triangles keeps the Morton order (the device's composite key has 32 bits).
 * SRT_ERR_INVALID for another value. Takes effect at the next srt_update_scene; accepted and without effect under
 * SRT_BUILD_HOST and SRT_ACCEL_NONE. srt_acceleration_build_info counts the launches actually enqueued, and
 * srt_last_build_kernel_ms spans them. */
#define SRT_BUILD_ORDER_MORTON 0
#define SRT_BUILD_ORDER_MEDIAN 1
int srt_set_acceleration_build_order(srt_tracer *t, int order);
/* Host-only: srt_bvh_morton_order_host and srt_bvh_morton_wide_host for SRT_BUILD_ORDER_MEDIAN -- the order defined above, and
 * the hierarchy the device leaves under it, bit for bit. */
int srt_bvh_median_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *order_out, size_t order_cap);
int srt_bvh_median_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *blocks_out, size_t blocks_cap,
                             uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, double *cost);
/* Tests / inspection: the device's block array as the kernel walks it -- every model's blocks, absolute indices, leaf
 * blocks with their triangles. Blocking. Writes at most blocks_cap blocks of 32 dwords and always sets *n_blocks (0 without
 * SRT_ACCEL_BVH or without models); blocks_out may be NULL to only query. */
int srt_read_bvh_blocks(srt_tracer *t, uint32_t *blocks_out, size_t blocks_cap, size_t *n_blocks);

/* Tracer::clear_canvas — src/tracer.cpp:98-101. With the denoiser on, also its sums and counts. */
int srt_clear_canvas(srt_tracer *t);

/* ---- the hot path -------------------------------------------------------------- */

/* Tracer::render(ticks_stopped, output) — src/tracer.cpp:103-116: launches the trace
 * kernel (canvas += mean radiance of options->num_samples paths per pixel), the
 * resolve kernel (canvas/ticks_stopped -> ACES -> sqrt -> A,R,G,B bytes) and copies
 * width*height*4 bytes to argb_out; returns when they are in host memory.
 * With a row partition set (below) only the owned rows are written, packed. */
int srt_render(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out);

/* srt_render without the final wait (the front-end's step right after the path,
 * src/main.cpp:290-337: the host can prepare the next frame while the GPU finishes this
 * one). Everything is enqueued on the handle's stream, including the copy into argb_out,
 * which must stay valid — and is only valid to read — after srt_synchronize(). Use
 * hipHostMalloc'ed memory for a truly asynchronous copy. Frames still execute in order. */
int srt_render_async(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out);

/* The two halves of srt_render, asynchronous on the handle's stream, for callers
 * that keep results on the device (bench, multi-GPU gather). */
int srt_trace(srt_tracer *t, const srt_render_data *options);      /* `render` kernel, render.cl:483 */
int srt_resolve(srt_tracer *t, uint32_t ticks_stopped);             /* `average` kernel, render.cl:525 */
int srt_synchronize(srt_tracer *t);
/* The `average` kernel over caller-owned device buffers (num_pixels float4 in,
 * num_pixels*4 bytes out), e.g. the gathered full canvas on the root GPU. Async. Always the plain bytes: the handle's
 * exposure (srt_set_exposure) is not applied here, and srt_last_resolve_exposed keeps its value. */
int srt_resolve_external(srt_tracer *t, const void *device_canvas, uint32_t num_pixels, uint32_t ticks_stopped,
                         void *device_argb);

/* Upper bound in bytes for the per-path radiance buffer (12 B per (pixel, sample) of a
 * sample batch). A dispatch whose paths do not fit is run as several batches of samples
 * with the ordered per-pixel sum carried across them: results are identical, only
 * slower. 0 (default) = half of the free HBM at the first srt_trace, at most 96 GiB; the
 * environment variable SRT_RADIANCE_BUDGET_MB overrides that default. */
int srt_set_radiance_budget(srt_tracer *t, size_t bytes);

/* ---- results / introspection ---------------------------------------------------- */

/* Copies the accumulation canvas (owned rows, packed): n_owned_rows*width float4. */
int srt_read_canvas(srt_tracer *t, float *rgba_out);
/* Copies the resolved image (owned rows, packed): n_owned_rows*width*4 bytes. */
int srt_read_argb(srt_tracer *t, uint8_t *argb_out);
int srt_get_counters(srt_tracer *t, srt_counters *out);
/* Select the instrumented trace-kernel variant that also fills tri_tests/tri_pass_u
 * (one extra VALU op per triangle test); results are unchanged. Default off. */
int srt_set_count_triangles(srt_tracer *t, int enable);
int srt_reset_counters(srt_tracer *t);
/* Diagnostics of the trace kernel's scheduling (not part of any result): out[0..4] = rays, sky, paths,
 * tri_tests, tri_pass_u as above; out[5] = the scene-class kernels' EXTEND phases that held fresh camera rays only (they run
 * the camera forms of the tests) << 36 | the rays in those phases, 0 for every other kernel; out[6] = iterations of the
 * waves' main loop; out[7] = SHADE phases executed (sums since the last srt_reset_counters); out[8] = persistent
 * waves per CU and out[9] = workgroups of the most recent trace launch; out[10..17] = per-phase wave cycles
 * (extend, sky ring, shade, park, deliver, refill, loop head, whole kernel) of a -DSRT_PHASE_CLOCK build; in the product
 * build of the array-scan kernels out[10..15] = triangle scans of big models, lanes in them, blocks of 64 rays taken out
 * of the launch-end ray pool, records handed in to it, sum over waves of (blocks taken)^2, blocks the last wave took; in the
 * product build of a scene class's axis twin out[10], out[11] = its EXTEND phases and those that failed the twin's guard; in the
 * product build of the NO_SPEC scene classes (DESIGN.md 5 "Diffuse waves") out[7] is counted too, out[12] = the SHADE phases in
 * which no lane ran the per-lane bounce (every shading lane's material plain diffuse, and the operand guard passed or no lane
 * bounced on at all) and out[13] = the SHADE phases whose lanes were all plain diffuse but failed the operand guard; else 0. */
int srt_debug_counters(srt_tracer *t, uint64_t out[18]);
/* Development builds with -DSRT_REGION_COUNT only (the product build writes nothing and sets *written = 0): for each
 * region of the trace kernel, in the order of SRT_REGION_LIST (csrc/trace_regions.h), {times a wave ran it, lanes that ran it}
 * summed since the last srt_reset_counters; scripts/isa_phase_mix.py multiplies them with the static instruction mix. */
int srt_debug_region_counters(srt_tracer *t, uint64_t *out, int capacity, int *written);
/* Device time of the most recent srt_trace (trace kernel(s) + ordered reduction) and of
 * the most recent resolve, from HIP events recorded on the handle's stream (milliseconds).
 * Synchronises the stream. The render calls (srt_render, srt_render_async, srt_render_pipelined) fuse the resolve into
 * the last reduction and record no timer events unless srt_set_kernel_timers(t, 1) was called (four event records are
 * 10-17 us of a 150 us interactive frame): after them both figures read 0 by default. */
int srt_last_kernel_ms(srt_tracer *t, float *trace_ms, float *resolve_ms);
int srt_set_kernel_timers(srt_tracer *t, int enable);
/* The same for srt_trace_kernel alone: one launch per sample batch of the dispatch. Batches that follow one another
 * (a dispatch of one batch, the usual case): the sum of each launch's own event pair, the ordered reductions between them
 * not counted. Overlapping batches (several batches: even and odd ones trace on two streams so that one batch's tail runs
 * under the next batch): the span from the first launch's start to the last one's end. srt_last_trace_launches says which:
 * the number of srt_trace_kernel launches of the last srt_trace and whether they overlapped. */
int srt_last_trace_kernel_ms(srt_tracer *t, float *kernel_ms);
int srt_last_trace_launches(const srt_tracer *t, int *launches, int *overlapped);
/* Device pointers of the handle's buffers, for zero-copy hand-off (e.g. to a
 * torch.distributed gather): canvas = owned_rows*width*16 B, argb = owned_rows*width*4 B. */
int srt_device_buffers(srt_tracer *t, void **canvas, size_t *canvas_bytes, void **argb, size_t *argb_bytes);
/* Use caller-owned device memory (>= owned_rows*width*16 B) as the canvas, and/or a
 * caller-owned hipStream_t for all launches. NULL restores the handle's own. */
int srt_bind_canvas(srt_tracer *t, void *device_canvas, size_t bytes);
int srt_bind_stream(srt_tracer *t, void *hip_stream);

/* ---- multi-GPU row partition (new; the reference is single-device) -------------- */

/* Rank `rank` of `world` owns the row blocks b with b % world == rank, a block being
 * `rows_per_block` scanlines; the canvas/ARGB buffers hold only those rows, packed in
 * increasing block order. Pixel seeds use the GLOBAL pixel index (render.cl:488,496),
 * so any partition reproduces the single-device image bit for bit. Clears the canvas.
 * world == 1 restores the full image. */
int srt_set_partition(srt_tracer *t, int rank, int world, int rows_per_block);

/* Pure host helpers (no GPU needed) describing that layout. */
int srt_partition_owned_rows(int height, int rank, int world, int rows_per_block);
/* padded_rows = rows every rank sends in an equal-count gather (max over ranks). */
int srt_partition_padded_rows(int height, int world, int rows_per_block);
/* Global y of packed local row `local_row` of `rank`, or -1 when it is padding. */
int srt_partition_global_row(int height, int rank, int world, int rows_per_block, int local_row);
/* Unpermute on the host: gathered = world * padded_rows rows of `row_bytes` each
 * (rank-major); image = height rows. */
int srt_partition_unpermute(const void *gathered, void *image, int height, int world, int rows_per_block,
                            size_t row_bytes);

/* ---- collecting a partitioned frame over RCCL / xGMI (new) ----------------------- */

/* One process per GPU: every rank owns a handle with srt_set_partition(rank, world, ...). Any one
 * rank calls srt_comm_unique_id and ships the 128 bytes to the others by whatever channel the host
 * program has (torch.distributed broadcast, MPI, a file); every rank then calls srt_comm_init
 * (collective: it returns when all ranks have joined). RCCL is loaded on first use. */
#define SRT_COMM_ID_BYTES 128
int srt_comm_unique_id(void *id_out);
int srt_comm_init(srt_tracer *t, const void *id, int rank, int world);
/* The ONE collective of the path, enqueued on the handle's stream after srt_trace: ncclGather of the
 * packed canvases (padded_rows * width float4 per rank) to `root`, where a kernel puts the rows back in
 * image order. Collective: every rank calls it. */
int srt_gather(srt_tracer *t, int root);
/* On the root, after srt_gather: the `average` kernel over the whole gathered image (asynchronous);
 * device pointers of the gathered canvas (height*width float4) and its resolved image; blocking
 * read-back of either (NULL = skip). */
int srt_resolve_gathered(srt_tracer *t, uint32_t ticks_stopped);
int srt_gathered_buffers(srt_tracer *t, void **canvas, void **argb);
int srt_read_gathered(srt_tracer *t, float *canvas_out, uint8_t *argb_out);
/* The root's unpermute step alone, on caller-owned device buffers (gathered: world x padded_rows x width
 * float4, rank-major; image: height x width float4); synchronous. For callers that gather by other
 * means, and for tests. */
int srt_unpermute_device(const void *gathered, void *image, int width, int height, int world, int rows_per_block);
/* The same step for a frame gathered with the denoiser's inputs (srt_group_set_denoise below). Every rank's slot of
 * `gathered` holds four planes of plane = padded_rows * width pixels back to back: its canvas rows, normal_depth and
 * albedo_hits (float4 per pixel each) and moments (one float per pixel, the plane padded to a multiple of four floats, so
 * that every slot starts on 16 bytes): srt_partition_planes_floats() = 12 * plane + round_up(plane, 4) floats per rank
 * (host only; -1 on bad arguments). ONE kernel launch puts all four back in image order: canvas, normal_depth,
 * albedo_hits = height x width float4, moments = height x width floats; synchronous. */
long long srt_partition_planes_floats(int width, int height, int world, int rows_per_block);
int srt_unpermute_planes_device(const void *gathered, void *canvas, void *normal_depth, void *albedo_hits, void *moments, int width, int height,
                                int world, int rows_per_block);

/* One process driving several GPUs -- what a front-end that keeps the reference's single `Tracer`
 * object needs (host/tracer.hpp: Tracer(width, height, n_devices)). The group owns one handle per
 * device (devices == NULL: 0 .. n_devices-1, wrapping around when the node has fewer), partitioned in interleaved
 * blocks of rows_per_block rows, and one communicator (ncclCommInitAll). A list that names a device more than once makes
 * VIRTUAL devices: the members share GPUs, RCCL is not used, and the collection is a device-to-device copy per member
 * where the gather would be -- the N > 1 path on fewer GPUs than members, down to one (tests, rehearsals). Scene
 * (prepared on the host once per srt_group_update_scene), skybox and options are replicated;
 * srt_group_render = trace on every device, one gather to the group's first device, resolve there,
 * blocking read-back of width*height*4 bytes: the image equals the single-device one bit for bit. */
typedef struct srt_group srt_group;
int srt_group_create(int width, int height, int n_devices, const int *devices, int rows_per_block, srt_group **out);
void srt_group_destroy(srt_group *g);
const char *srt_group_last_error(const srt_group *g);
int srt_group_size(const srt_group *g);
srt_tracer *srt_group_tracer(srt_group *g, int i);
int srt_group_set_skybox(srt_group *g, const float *rgba, int width, int height);
/* albedo textures (below): the same call on every member */
int srt_group_set_textures(srt_group *g, const srt_texture_desc *descs, size_t n);
int srt_group_set_material_textures(srt_group *g, const srt_material_texture *bindings, size_t n_materials);
int srt_group_set_triangle_uvs(srt_group *g, const float *uv, size_t n_triangles);
int srt_group_set_triangle_materials(srt_group *g, const int32_t *materials, size_t n_triangles); /* per-triangle materials (below) */
int srt_group_set_acceleration(srt_group *g, int mode);
int srt_group_set_acceleration_refit(srt_group *g, int mode); /* srt_set_acceleration_refit on every member */
int srt_group_set_acceleration_deform(srt_group *g, int mode, float rebuild_ratio); /* srt_set_acceleration_deform on every member */
int srt_group_set_acceleration_build(srt_group *g, int mode, uint32_t min_triangles); /* srt_set_acceleration_build on every member (the scene is prepared once; every member sorts on its own device) */
int srt_group_set_acceleration_build_order(srt_group *g, int order); /* srt_set_acceleration_build_order on every member */
int srt_group_update_scene(srt_group *g, const srt_shape *shapes, size_t n_shapes, const srt_triangle *triangles, size_t n_triangles,
                           const srt_material *materials, size_t n_materials, const srt_scene_data *scene);
int srt_group_clear_canvas(srt_group *g);
int srt_group_trace_and_gather(srt_group *g, const srt_render_data *options); /* asynchronous */
int srt_group_render(srt_group *g, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out);
int srt_group_read_canvas(srt_group *g, float *rgba_out); /* the gathered canvas, height*width float4 */
int srt_group_get_counters(srt_group *g, srt_counters *out); /* summed over the devices */
/* The denoiser (below: srt_set_denoise, srt_set_denoise_temporal) on a group. Semantics, validation and error codes are
 * those of the per-handle calls of the same names; the filtered frame equals the single-device one bit for bit. While it is
 * on, every member accumulates the guide sums and moments of its OWN rows beside its canvas rows, in one allocation; the
 * frame is still collected by one gather per member (52 B per pixel instead of 16) and ONE unpermute launch on the
 * group's first device, where filter, history (two sets, there only) and counts live. srt_group_render resolves through
 * the filter (K = 0: the plain resolve's bytes); srt_group_clear_canvas makes the frame being cleared the history when
 * something was traced and zeroes every member's sums and the counts. Turning the denoiser on, or changing
 * feature_samples, clears the canvas and the sums on every member. The history is dropped by
 * srt_group_reset_denoise_history, srt_group_set_skybox, the three srt_group_set_*texture* calls,
 * srt_group_set_triangle_materials, an
 * srt_group_update_scene with other bytes than the previous one's, and by turning the denoiser or temporal off.
 * srt_group_resolve_denoised: after srt_group_trace_and_gather, asynchronous on the first device. The read-backs block;
 * srt_group_read_denoise_inputs returns what the last srt_group_trace_and_gather / srt_group_render collected.
 * The per-handle rules stand: srt_set_denoise on a member (srt_group_tracer) of a group of more than one still returns
 * SRT_ERR_STATE, and while the group's denoiser is on a member refuses srt_set_partition, srt_bind_canvas and
 * srt_set_denoise (SRT_ERR_STATE). Not carried over: object motion (srt_set_denoise_object_motion), srt_render_pipelined on
 * a member, and the one-process-per-GPU path (srt_gather / srt_resolve_gathered stay plain resolves). */
int srt_group_set_denoise(srt_group *g, const srt_denoise_params *params);
int srt_group_set_denoise_temporal(srt_group *g, const srt_temporal_params *params);
int srt_group_reset_denoise_history(srt_group *g);
int srt_group_resolve_denoised(srt_group *g, uint32_t ticks_stopped);
int srt_group_read_denoised(srt_group *g, float *rgba_out);
int srt_group_read_denoise_inputs(srt_group *g, float *normal_depth, float *albedo_hits, float *moments, uint32_t counts[2]);
int srt_group_read_denoise_history(srt_group *g, float *colour_count, float *moments, float *guide, srt_render_data *camera, int *valid);

/* ---- frame pipeline for the interactive loop (new; src/main.cpp:277-337) ----------- */

/* srt_render with the read-back of frame N overlapped with the trace of frame N+1: the call enqueues
 * frame N (trace, resolve into one of two device images, copy to pinned host memory on a second
 * stream) and hands out frame N-1, waiting only for THAT frame's copy. *frame_delivered = index of the
 * frame written to argb_out (0, 1, ...), or -1 on the first call (argb_out untouched). Frames are the
 * same bytes srt_render would have produced, one call later. srt_pipeline_flush waits for and hands out
 * the newest frame still in flight (-1: none). */
int srt_render_pipelined(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out,
                         long long *frame_delivered);
int srt_pipeline_flush(srt_tracer *t, uint8_t *argb_out, long long *frame_delivered);

/* ---- edge-aware denoiser (new; the reference's "Denoising" plan, README.md:44) -------- */

/* A spatial variance-guided a-trous filter (Schied et al., HPG 2017, without the temporal part). While
 * it is on, srt_trace / srt_render / srt_render_async / srt_render_pipelined also
 *   - trace the first min(feature_samples, num_samples) camera rays of every pixel to their first hit and
 *     add up the front-facing normals, hit distances, material colours (sky: 1,1,1) and hits (guide buffers),
 *   - add (1/n) * sum over the dispatch's paths of lum(radiance)^2 to a per-pixel moments buffer,
 *     lum(c) = 0.2126 r + 0.7152 g + 0.0722 b;
 * and the render calls resolve through the filter instead of the plain resolve. The canvas itself is
 * bit-for-bit what it is with the denoiser off; the filter is outside the parity contract (fast exp / pow).
 * Not available on a partitioned handle (srt_set_partition world > 1) or through srt_resolve_gathered /
 * srt_resolve_external; a device group has calls of its own (srt_group_set_denoise above). */

/* Host-only: K = 5, sigma_luminance = 4, sigma_normal = 128, sigma_depth = 1, sigma_albedo = 0.1,
 * feature_samples = 1, enable = 1. */
int srt_denoise_defaults(srt_denoise_params *out);
/* params NULL or enable == 0: off. Turning it on, or changing feature_samples while on, clears the
 * canvas and all accumulations (guide buffers, moments, the counts below); other changes do not.
 * Device buffers (36 B of sums + 64 B of filter state per pixel) are allocated on the first enable and kept.
 * SRT_ERR_INVALID: a value out of range (iterations 0..8, feature_samples 1..64, sigmas > 0 and finite,
 * reserved != 0). SRT_ERR_STATE: the handle is partitioned (world > 1). */
int srt_set_denoise(srt_tracer *t, const srt_denoise_params *params);
/* The filter over the current canvas with the divisor ticks_stopped, into the handle's ARGB image
 * (srt_read_argb) and the HDR result (srt_read_denoised). Asynchronous, like srt_resolve.
 * SRT_ERR_STATE when the denoiser is off or nothing has been traced since the last clear. */
int srt_resolve_denoised(srt_tracer *t, uint32_t ticks_stopped);
/* The last filter result before tonemapping: width*height float4 = filtered r, g, b and variance. Blocking. */
int srt_read_denoised(srt_tracer *t, float *rgba_out);
/* The filter's inputs since the last clear (blocking; NULL skips an output): normal_depth = width*height
 * float4 {sum of normals over hits, sum of hit distances}; albedo_hits = width*height float4 {sum of
 * albedos over feature rays, hits}; moments = width*height floats; counts = {T dispatches, P = sum of
 * num_samples}. */
int srt_read_denoise_inputs(srt_tracer *t, float *normal_depth, float *albedo_hits, float *moments, uint32_t counts[2]);

/* ---- temporal reprojection for the denoiser (new; SVGF's temporal half) ---------------------------------------------- */

/* Opt-in, between the filter's set-up and its a-trous passes. At each srt_clear_canvas with something traced since the
 * last clear, the frame being cleared (its colour and moments integrated with its own history, their sample count capped
 * at history_limit, its guide buffers and the camera of its last dispatch) becomes the history. The filter of a later
 * frame reprojects the history into its camera (bilinear taps, rejected on normal and distance) and blends it in,
 * weighted by sample counts: c = (P c_cur + h c_hist) / (P + h), the moments likewise, variance from the blended moments
 * over P + h. With temporal on the set-up divides the canvas by the dispatch count T since the clear, not by
 * ticks_stopped (the same in the front-end's loop). A pixel without history gets exactly the spatial set-up's values.
 * The history is dropped by srt_reset_denoise_history, turning temporal on or off, srt_set_denoise turning the denoiser
 * off (which also turns temporal off) or clearing its accumulations, srt_set_skybox, and an srt_update_scene whose
 * arrays or scene data differ in bytes from the previous call's. 112 B of device memory per pixel (two history sets),
 * allocated on the first enable. Full-frame handles only, like the denoiser (a device group: srt_group_set_denoise_temporal). */

/* Host-only: enable = 1, history_limit = 32, normal_threshold = 0.9, depth_threshold = 0.05. */
int srt_temporal_defaults(srt_temporal_params *out);
/* params NULL or enable == 0: off. SRT_ERR_INVALID: history_limit outside 1..2^20, normal_threshold outside [-1, 1],
 * depth_threshold not finite and > 0, reserved != 0. SRT_ERR_STATE: the denoiser is off or the handle is partitioned. */
int srt_set_denoise_temporal(srt_tracer *t, const srt_temporal_params *params);
/* Drop the history: the next frame is filtered as by the spatial denoiser alone. */
int srt_reset_denoise_history(srt_tracer *t);
/* The current history (blocking; NULL skips an output): colour_count = width*height float4 {integrated r, g, b, sample
 * count}; moments = width*height float2 {m1, m2}; guide = width*height x 2 float4 {N, Z}, {A, coverage}; camera = the
 * history frame's render data; *valid = 0 when there is no history (the outputs are then zero).
 * SRT_ERR_STATE when temporal reprojection was never enabled on this handle. */
int srt_read_denoise_history(srt_tracer *t, float *colour_count, float *moments, float *guide, srt_render_data *camera, int *valid);

/* ---- object motion for the temporal stage (new) --------------------------------------------------------------------- */

/* Opt-in, on top of srt_set_denoise_temporal: the history survives an srt_update_scene that only moves shapes. While it is
 * on, the feature pass also stores one shape index per pixel (the first hit of feature sample 0 of the latest dispatch,
 * 0xffffffff: no hit, or a shape without a material), the handle keeps the scene the history frame was traced with, and
 * srt_update_scene compares the new scene with *that* scene: the history is kept when n_shapes, every shape's type and
 * material, the materials, srt_scene_data and the triangle array are the same in bytes and a model keeps its
 * triangle_index and num_triangles. Only a sphere's position / radius, a plane's position / normal and a model's
 * transform (with bounding_min / bounding_max, the world box the front-end derives from it) may differ. Per shape the host then derives (in double, rounded to float) a state and the maps "now -> then":
 *   A (3x4, rows): current world position -> history world position;  B (3x3, rows): current normal -> history normal
 *   sphere  X' = p_c + (r_c / r_h)(X - p_h)          plane  X' = p_c + R (X - p_h), R the minimal rotation n_h -> n_c
 *   model   M_c M_h^-1 (the affine part: columns 0..2 and the translation of `transform`)
 * (history -> current; A is the inverse, B the transpose of the linear part). A pixel of a moved shape looks its history up
 * at the projection of A X into the history camera and accepts only taps that showed the same shape; a pixel of a static
 * shape does what it does without object motion, except that a tap which showed a moved shape does not count. A frame in
 * which nothing moved is bit for bit the frame without object motion. A frame traced with two different scenes (an
 * srt_update_scene with other bytes while samples are on the canvas) does not become a history at the next clear.
 * Lighting is not tracked: a static pixel keeps its history although a moved object's shadow or reflection on it changed;
 * history_limit bounds the lag. 8 B of device memory per pixel, allocated on the first enable. */
enum { SRT_MOTION_STATIC = 0, SRT_MOTION_MOVED = 1, SRT_MOTION_NO_HISTORY = 2 };
#define SRT_MOTION_WORDS 22 /* per shape: state, A[12], B[9] (the floats' bits) */

/* enable != 0: on. SRT_ERR_STATE unless temporal reprojection is on (so never on a partitioned handle). Turning temporal
 * or the denoiser off turns it off. Every change of the switch drops the history. */
int srt_set_denoise_object_motion(srt_tracer *t, int enable);
/* The shape indices (blocking; NULL skips an output; width*height words each): current = what the feature pass wrote since
 * the last clear (undefined before the first dispatch), history = the history frame's (all 0xffffffff without a history).
 * SRT_ERR_STATE when object motion was never enabled on this handle. */
int srt_read_denoise_shape_ids(srt_tracer *t, uint32_t *current, uint32_t *history);
/* The table the next filter would use: *n_shapes rows of SRT_MOTION_WORDS words into table (capacity_shapes rows of room;
 * SRT_ERR_INVALID when fewer than *n_shapes, which is still set), *any_moved != 0 when a row is not STATIC (the moved
 * set-up kernel runs). Without a history every row is STATIC / identity. SRT_ERR_STATE when object motion is off. */
int srt_read_denoise_motion(srt_tracer *t, uint32_t *table, size_t capacity_shapes, size_t *n_shapes, int *any_moved);
/* Host-only (no device): the comparison and the table of the rules above for a history scene and a current scene.
 * *keep = 0: the history would be dropped (table untouched); else table receives n_shapes rows. SRT_ERR_INVALID on NULL
 * arguments (arrays of length 0 may be NULL). */
int srt_motion_table_host(const srt_shape *h_shapes, size_t h_n_shapes, const srt_triangle *h_triangles, size_t h_n_triangles,
                          const srt_material *h_materials, size_t h_n_materials, const srt_scene_data *h_scene,
                          const srt_shape *c_shapes, size_t c_n_shapes, const srt_triangle *c_triangles, size_t c_n_triangles,
                          const srt_material *c_materials, size_t c_n_materials, const srt_scene_data *c_scene, uint32_t *table, int *keep);

/* ---- per-triangle motion for the temporal stage (new) ---------------------------------------------------------------- */

/* Opt-in, on top of srt_set_denoise_object_motion: the history also survives an srt_update_scene that changes the vertices
 * of a model (skinning, cloth, morph targets) as long as the topology stays. While it is on:
 *   keep rule   object motion's, except that the triangle arrays need only have the same count: each model keeps its
 *               triangle_index and num_triangles, the bytes inside a model's range may differ, bytes no model's range
 *               covers are not compared. A model with a differing byte in its range is DEFORMED (whether or not its
 *               transform changed too), and so is every instance over that range; a model whose range is the same bytes is
 *               STATIC, MOVED or NO_HISTORY as without the switch.
 *   table       a DEFORMED row holds the state in word 0, the shape's first row in the vertex tables in word 1, zeros else.
 *   triangles   the feature pass also stores, per pixel, the index inside its model of the triangle feature sample 0 of the
 *               latest dispatch hit (0xffffffff: a miss, a shape without a material, not a model): 4 B per pixel, twice.
 *   vertices    two tables (the frame's, the history's) of 9 floats per instance triangle: P0, P1, P2 = transform * vertex
 *               in the tracer's own expressions, so they are the traced world vertices bit for bit. Model shapes in shape
 *               order, triangle j of a model in row first_row + j. The frame's table is written by one launch before the
 *               first feature pass after an srt_update_scene with other bytes (not at the update: the history keeps the
 *               scene its frame was traced with); srt_clear_canvas's commit swaps the two. 72 B per instance triangle and
 *               table, allocated with the first enable over a scene with triangles.
 *   a pixel     of a DEFORMED shape with triangle t (none, or t >= num_triangles: no history), rows P (frame) and Q
 *               (history) at first_row + t, all float32, unfused, dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z:
 *                 e1 = P1 - P0, e2 = P2 - P0, f1 = Q1 - Q0, f2 = Q2 - Q0, X = the first hit, d = X - P0
 *                 a11 = dot(e1, e1), a12 = dot(e1, e2), a22 = dot(e2, e2), det = a11 a22 - a12 a12 (not > 0 or not
 *                 finite: no history)
 *                 u = (a22 dot(d, e1) - a12 dot(d, e2)) / det, v = (a11 dot(d, e2) - a12 dot(d, e1)) / det (not clamped)
 *                 X_h = (Q0 + u f1) + v f2 (not finite: no history)
 *                 gc = cross(e1, e2) / |cross(e1, e2)|, gh likewise of f1, f2 (a zero or non-finite length: no history)
 *                 nu, nv = the same solve with the pixel's normal N_p for d, c = dot(N_p, gc)
 *                 N_h = normalise((nu f1 + nv f2) + c gh) (a zero or non-finite length: no history)
 *               X_h is projected into the history camera (also for the same camera); a tap counts only when its history
 *               shape index is the pixel's, its normal is compared with N_h and its depth with |X_h - cam_h|, as for a
 *               MOVED shape. Exact for rigid motion and for flat normals under any deformation; under stretch a smooth
 *               normal's tilt is distorted and the test errs towards no history.
 *   a STATIC pixel rejects a tap whose history shape is MOVED or DEFORMED; MOVED and NO_HISTORY pixels are unchanged.
 * With the switch off the library enqueues what it enqueues without it and keeps every drop rule. Another triangle count or
 * another topology drops the history as before; lighting is not tracked (see above). */
enum { SRT_MOTION_DEFORMED = 3 };

/* enable != 0: on. SRT_ERR_STATE unless object motion is on (so never on a partitioned handle). Turning object motion,
 * temporal reprojection or the denoiser off turns it off. Every change of the switch drops the history. */
int srt_set_denoise_vertex_motion(srt_tracer *t, int enable);
/* The triangle indices (blocking; NULL skips an output; width*height words each), as srt_read_denoise_shape_ids.
 * SRT_ERR_STATE when per-triangle motion was never enabled on this handle. */
int srt_read_denoise_triangle_ids(srt_tracer *t, uint32_t *current, uint32_t *history);
/* The world-vertex tables (blocking; NULL skips an output): *n_rows = rows of the current scene, 9 floats each; current = the
 * table as last written (before the first dispatch after an update: the previous contents), history = the history frame's
 * (zeros without a history). SRT_ERR_INVALID when an output is given and cap_rows < *n_rows (still set). SRT_ERR_STATE when
 * per-triangle motion was never enabled on this handle. */
int srt_read_denoise_vertex_tables(srt_tracer *t, float *current, float *history, size_t cap_rows, size_t *n_rows);
/* Host-only: srt_motion_table_host with the keep rule above (what srt_update_scene applies while the switch is on). */
int srt_motion_table_deform_host(const srt_shape *h_shapes, size_t h_n_shapes, const srt_triangle *h_triangles, size_t h_n_triangles,
                                 const srt_material *h_materials, size_t h_n_materials, const srt_scene_data *h_scene,
                                 const srt_shape *c_shapes, size_t c_n_shapes, const srt_triangle *c_triangles, size_t c_n_triangles,
                                 const srt_material *c_materials, size_t c_n_materials, const srt_scene_data *c_scene, uint32_t *table, int *keep);

/* ---- albedo demodulation for the filter (new; SVGF's own: filter illumination, not colour) ------------------------------ */

/* Opt-in. With it on and iterations K >= 1 the a-trous passes run over the illumination I = colour / albedo instead of the
 * colour, and the last pass multiplies the albedo back: a surface whose texels differ from pixel to pixel keeps its pattern
 * and still gets its noise averaged across texels and across coplanar materials. The albedo is the mean first-hit albedo
 * of the guide (the texel where a texture is bound), so no trace kernel, feature kernel or record changes.
 *   demodulate  after whichever set-up ran (spatial, temporal, moved). A pixel with cov > 0 and a finite colour:
 *               D = max(A, SRT_DEMOD_EPS) per channel (a NaN channel: SRT_DEMOD_EPS), I = c / D per channel (IEEE),
 *               V_I = V / lum(D)^2. Any other pixel is left as it is: never a tap, passed through, as without the switch.
 *   passes      the filter's formula (csrc/denoise.hip) over I and V_I WITHOUT the albedo factor: sigma_albedo is ignored in
 *               this mode. The luminance term uses lum(I); prefilter, skip rules and pass-through rules are unchanged.
 *   remodulate  in the last pass, for the pixels that were demodulated: o = I' D_p, V' = V_I' lum(D_p)^2; tonemap(o) is the
 *               ARGB image and {o, V'} what srt_read_denoised returns. A demodulated pixel that got no weight returns
 *               I_p D_p, within rounding of its colour but not bit-equal to it.
 * K = 0: no effect, the plain resolve's bytes. SRT_DEMOD_EPS bounds the amplification at 100x; it is not a tunable.
 * The temporal history keeps holding colour. For diffuse and metallic first hits the colour is exactly albedo x
 * illumination; for specular > 0, glass and emitters the first-hit colour is not the exact factor (the transform is
 * still inverted per pixel, only the smoothness of I is weaker there). With feature_samples < num_samples the guide's
 * mean texel estimates the canvas's: use feature_samples = num_samples on textured scenes. */
#define SRT_DEMOD_EPS 0.01f
/* enable != 0: on. SRT_ERR_STATE unless the denoiser is on (the group call: the group's denoiser). Turning the denoiser off
 * turns it off. Clears nothing and keeps the temporal history; takes effect at the next filter (srt_render*,
 * srt_resolve_denoised, srt_group_render, srt_group_resolve_denoised). */
int srt_set_denoise_demodulation(srt_tracer *t, int enable);
int srt_group_set_denoise_demodulation(srt_group *g, int enable);
/* Which passes the last filter ran: *demodulated = 1 for the demodulated ones (the switch on and K >= 1), else 0. */
int srt_last_filter_demodulated(const srt_tracer *t, int *demodulated);
int srt_group_last_filter_demodulated(const srt_group *g, int *demodulated);

/* ---- spatial variance estimate for pixels with few samples (new; SVGF §4.2) -------------------------------------------- */

/* Opt-in. The set-ups take a pixel's variance from that pixel's own moments: from two samples it is often exactly 0 and
 * otherwise wrong by large factors, and every a-trous pass takes its luminance weight from it. With min_samples > 0 and
 * iterations K >= 1, one more launch between the set-up (whichever ran: spatial, temporal, moved, deformed; under
 * demodulation after the demodulate launch) and the passes replaces the variance of every pixel that has fewer than
 * min_samples samples by an estimate from the moments of its 7x7 neighbourhood, weighted by the filter's geometric weights.
 * All float32, unfused, in the order written; tests/spatial_variance_ref.py restates it.
 *   inputs     per pixel p: the spatial set-up: s_p = P (as a float), m1_p = lum(canvas / T), m2_p = M / T (the expressions of
 *              the set-up kernel, from the same buffers); any temporal set-up: s_p = the staged count min(n, history_limit),
 *              m1_p, m2_p = the staged moments.
 *   qualifies  cov_p > 0, a finite colour and s_p < (float)min_samples. Every other pixel keeps its {colour, variance} bit
 *              for bit.
 *   taps       q = p + (dx, dy), dx, dy in -3..3, dy in the outer loop and dx in the inner one; taps outside the image are
 *              skipped; a tap counts when cov_q > 0, its colour is finite and m1_q, m2_q are finite.
 *   weight     w = exp(-|Zp - Zq| / (sigma_depth Zp r + 1e-6)) max(0, Np.Nq)^sigma_normal exp(-|Ap - Aq|^2 / sigma_albedo^2),
 *              r = max(|dx|, |dy|), with the a-trous kernel's expressions and fast exp / log. No spatial kernel h and no
 *              luminance term; a tap with Np.Nq <= 0 is skipped; the centre tap (when it counts) has weight 1.
 *   result     m1' = sum(w m1_q) / sum(w), m2' = sum(w m2_q) / sum(w), V = max(0, m2' - m1' m1') / s_p (non-finite: 0). Only
 *              the variance is written; the colour is untouched.
 *   demodulation (srt_set_denoise_demodulation on): the estimate is made in illumination space and the albedo factor is
 *              dropped, as the passes drop it: a_q = 1 / lum(D_q), D the demodulate launch's divisor, a tap contributes
 *              m1_q a_q and (m2_q a_q) a_q, and the result is V_I itself (the launch runs after the demodulate launch).
 * K = 0: nothing is launched, the plain resolve's bytes, srt_read_denoised's variance is the set-up's. With the switch off
 * the library enqueues exactly what it enqueues without this interface. The history holds colour and moments, never
 * variance: the switch changes nothing that is staged or committed. When history_limit < min_samples, s_p never reaches
 * min_samples and every pixel is estimated spatially, with divisor s_p: not an error.
 * min_samples = 0: off (the default); 1..2^20: on. SRT_ERR_INVALID above 2^20. SRT_ERR_STATE unless the denoiser is on (the
 * group call: the group's denoiser). Turning the denoiser off turns it off. Clears nothing and keeps the temporal history;
 * takes effect at the next filter, as srt_set_denoise_demodulation does. */
int srt_set_denoise_spatial_variance(srt_tracer *t, uint32_t min_samples);
int srt_group_set_denoise_spatial_variance(srt_group *g, uint32_t min_samples);
/* *ran = 1 when the last filter enqueued the estimate (the switch on and K >= 1), else 0. */
int srt_last_filter_spatial_variance(const srt_tracer *t, int *ran);
int srt_group_last_filter_spatial_variance(const srt_group *g, int *ran);

/* ---- the history reprojected as illumination (new; SVGF reprojects demodulated illumination) ---------------------------- */

/* Opt-in, on top of srt_set_denoise_temporal. The temporal set-up gathers the history's *colour* through a bilinear 2x2:
 * on a textured surface that is a bilinear blur of the texture, once more every frame the camera or an object moves. With
 * the switch on a tap is rescaled from its own first-hit albedo to this pixel's at the moment it is gathered, which is
 * reprojection of illumination. The history's contents do not change (it keeps holding colour; every history pixel
 * already carries its albedo and coverage in its guide), so there is no new device memory and a clear commits what it
 * commits without the switch. All float32, unfused, in the order written; tests/history_illumination_ref.py restates it.
 *   pixel p     D_p = max(A_p, SRT_DEMOD_EPS) per channel (fmaxf: a NaN channel gives SRT_DEMOD_EPS), L_p = lum(D_p),
 *               full_p = (cov_p == 1.0f): every feature sample hit.
 *   tap h       a counted tap (every rejection rule of the set-up unchanged) of a pixel that projects: D_h, L_h likewise
 *               from the history guide. full_p and cov_h == 1.0f: r = D_p / D_h per channel (IEEE), rl = L_p / L_h;
 *               otherwise r = (1, 1, 1), rl = 1 (a partly covered pixel's colour holds sky light that no albedo scaled).
 *   sums        colour += w (c_h r) per channel, m1 += w (m1_h rl), m2 += w ((m2_h rl) rl); the weight and count sums, the
 *               integration, the staged and committed sets, the guide and the tonemap are unchanged.
 *   identity    the one tap of a pixel that does not project (the same camera bit for bit, the shape not moved) is the pixel
 *               itself and is not rescaled: a still camera gives the same bits with the switch on or off.
 * Where D_p and D_h are bit-equal, r is exactly 1: an untextured, fully covered surface of one material gives the colour
 * path's bits. The limits of albedo demodulation carry over: specular > 0, glass and emissive first hits are not exactly
 * albedo x illumination, so a tap from a dark texel of an emitter can be amplified up to 1 / SRT_DEMOD_EPS; and with
 * feature_samples < num_samples the guide's mean texel is an estimate (use feature_samples = num_samples on textured scenes).
 * enable != 0: on. SRT_ERR_STATE unless temporal reprojection is on (so never on a partitioned handle; the group call: the
 * group's temporal reprojection). Turning temporal reprojection or the denoiser off turns it off. Clears nothing and keeps
 * the history; takes effect at the next set-up, a filter's or the one a clear runs before its commit when no filter ran
 * after the last trace (a change of the switch makes the clear run its own set-up, so the history never depends on whether
 * a filter ran). Independent of demodulation, object motion, per-triangle motion and the spatial variance estimate. */
int srt_set_denoise_history_illumination(srt_tracer *t, int enable);
int srt_group_set_denoise_history_illumination(srt_group *g, int enable);
/* 1 when the last temporal set-up (a filter's or a clear's) launched one of the three illumination kernels, else 0 (also for NULL). */
int srt_last_setup_history_illumination(srt_tracer *t);
int srt_group_last_setup_history_illumination(srt_group *g);

/* ---- the history clamped to the frame's local colour range (new; neighbourhood clamping of the reprojected history) ------ */

/* Opt-in, on top of srt_set_denoise_temporal. The temporal set-up accepts a history tap on geometry alone (shape, normal,
 * depth), so what a moved shape lights or shades -- its shadow, its reflection, an emitter's glow -- stays in the history of
 * pixels that did not move and fades over history_limit / P frames. With the clamp on, the history colour of a pixel is pulled
 * into the range the current frame's own samples around that pixel make plausible before it is blended in. All float32,
 * unfused, in the order written; tests/history_clamp_ref.py restates it.
 *   bounds      one launch before the set-up, only when the clamp is on and a valid history exists (without one nothing new
 *               is launched). Pixel p qualifies with cov_p > 0 and a finite colour c_p = canvas_p / T (the set-up's
 *               expressions). Its 49 taps q = p + (dx, dy), |dx|, |dy| <= 3, dy outer, dx inner; a tap counts unless it is
 *               outside the image, has cov 0 or a non-finite colour. The centre has weight 1, another counting tap the spatial
 *               variance estimate's geometric weight from the handle's filter sigmas,
 *               w = exp(-|Zp - Zq| / (sz Zp r + 1e-6)) max(0, Np.Nq)^sn exp(-|Ap - Aq|^2 / sa^2), r = max(|dx|, |dy|)
 *               (Np.Nq <= 0: it counts with weight 0). Per channel mu = sum w c / sum w, s = sum w (c c) / sum w,
 *               sigma = sqrt(max(0, s - mu mu)), evaluated on the differences from the centre (which is the same
 *               quantity, without subtracting two large squares where the colour is bright and the spread small):
 *               e_q = c_q - c_p, d = sum w e / sum w, q = sum w (e e) / sum w, mu = c_p + d, sigma = sqrt(max(0, q - d d)).
 *   planes      0: {mu.rgb, sum w}, 1: {sigma.rgb, number of counting taps}. sum w is stored as 0, "do not clamp", when
 *               fewer than 5 taps count (the centre included: a thin feature's 4 neighbours say nothing about a range) or a
 *               mu or q is not finite; a pixel that does not qualify has both planes 0.
 *   clamp       in the set-up, where a pixel's history colour x_h is complete: after the bilinear gather or the same-camera
 *               tap, and after srt_set_denoise_history_illumination's rescale. With sum w > 0 each channel:
 *               x < mu - gamma sigma: x = mu - gamma sigma; else x > mu + gamma sigma: x = mu + gamma sigma (gamma sigma
 *               rounded first; comparisons, so a NaN moves nothing). No channel moved: nothing else changes and the pixel's
 *               outputs are the switch-off outputs bit for bit. Else the history moments follow and keep their variance:
 *               m1' = lum(x_h'), m2' = max(0, m2_h - m1_h m1_h) + m1' m1'.
 *   unchanged   counts, weights, history_limit, the blend, the staged and committed sets' layout. The clamped value goes
 *               through the blend into what the next clear commits, so a stale value decays on its own; no count is reduced.
 * gamma == 0: off (the default). Finite 0 < gamma <= 64: on; anything else SRT_ERR_INVALID. SRT_ERR_STATE unless temporal
 * reprojection is on (so never on a partitioned handle; the group call: the group's temporal reprojection). Turning temporal
 * reprojection or the denoiser off turns it off. Clears nothing and keeps the history; the two planes (32 B per pixel) are
 * allocated at the first enable and are no part of the history or of a group's gather. Takes effect at the next set-up, a
 * filter's or the one a clear runs before its commit when no filter ran after the last trace (a change of gamma makes the
 * clear run its own set-up: both run the bounds launch and the same clamping kernel, so the history never depends on
 * whether a filter ran). Works under demodulation (the set-up still outputs colour), the spatial variance estimate, history
 * illumination, object and per-triangle motion, K = 0 and frames of several dispatches. */
int srt_set_denoise_history_clamp(srt_tracer *t, float gamma);
int srt_group_set_denoise_history_clamp(srt_group *g, float gamma);
/* 1 when the last temporal set-up (a filter's or a clear's) ran the bounds launch and a clamping set-up, else 0 (also for NULL). */
int srt_last_setup_history_clamp(srt_tracer *t);
int srt_group_last_setup_history_clamp(srt_group *g);
/* For tests: the two planes of the last bounds launch, height*width float4 each (either may be NULL). SRT_ERR_STATE when the
 * clamp has never run on this handle. */
int srt_read_denoise_history_bounds(srt_tracer *t, float *mean_weight, float *sigma_taps);

/* ---- the first a-trous pass fed back into the history (new; SVGF's feedback of the first wavelet iteration) --------------- */

/* Opt-in, on top of srt_set_denoise_temporal. The temporal history holds the integrated colour as the set-up blends it: raw
 * samples, as noisy as the frame. With the switch on the colour that enters the history is the output of the first a-trous
 * pass, so every frame's history has already been averaged over an edge-aware 5x5. All float32, unfused, in the order written;
 * tests/feedback_ref.py restates it.
 *   when        the switch on and iterations K >= 1. K = 0: there is no pass and nothing changes, the plain resolve's bytes and
 *               the switch-off history.
 *   what        pass 1 (k = 0, step 1; after the set-up, and after the demodulate launch and the spatial-variance launch where
 *               those are on) also stores its colour result into the rgb of the staging set's {colour, count} plane: x, y, z
 *               alone, one three-dword store; the count .w is not touched. A pixel's colour is written only when the pixel
 *               entered the filter branch (cov > 0 and a finite input), received weight (sum w > 0) and the three values to
 *               be stored are finite. Every other pixel -- sky, a non-finite colour, no weight, a non-finite result -- keeps
 *               the set-up's integrated colour bit for bit.
 *   demodulation the value stored is colour, as the history always holds: I' D_p per channel with D_p = max(A_p,
 *               SRT_DEMOD_EPS), the expression the last pass remodulates with; for K = 1 the pass is the last one and its
 *               remodulated output is the value.
 *   unchanged   the staged count, {m1, m2} (the moments stay unfiltered, as in SVGF: the next frame's variance comes from
 *               them) and the guide; the set-up kernels, the bounds launch, the blend, history_limit, the commit's swap; the
 *               filter's output image and ARGB bytes of the same frame. With the history clamp off the committed count,
 *               moments and guide of every frame are therefore bit-equal to the switch-off ones; only the colour differs.
 *   the clear   a clear with no filter since the last trace (or with a setter below since the filter) makes the staging set
 *               itself. With the switch on and K >= 1 it runs the filter's front before the commit: the set-up into the
 *               filter image, the demodulate launch if on, the spatial-variance launch if on, pass 1 in its feedback form --
 *               the code a filter runs, so the history never depends on whether a filter ran (the temporal set-up divides by
 *               T: the clear needs no divisor). That run does not write the ARGB image. It uses the filter's two images:
 *               afterwards srt_read_denoised returns SRT_ERR_STATE until the next filter. With the switch off
 *               srt_read_denoised behaves as without this interface.
 *   stale       while the switch is on, every setter that changes what pass 1 computes makes the next clear run that front:
 *               this switch, srt_set_denoise when it changes a sigma or K, srt_set_denoise_demodulation and
 *               srt_set_denoise_spatial_variance (as the illumination and clamp setters already do for the set-up).
 *   repeats     two filters of one frame without a trace between them commit what one commits: the set-up rewrites the
 *               staging set from the history and the canvas before pass 1 overwrites its colour.
 * With the switch off the library enqueues exactly what it enqueues without this interface, and the kernels it launches then
 * keep their instructions. No new device memory. Independent of object motion, per-triangle motion, history illumination
 * and the history clamp (which acts on whatever colour the history holds).
 * enable != 0: on. SRT_ERR_STATE unless temporal reprojection is on (so never on a partitioned handle; the group call: the
 * group's temporal reprojection). Turning temporal reprojection or the denoiser off turns it off. Clears nothing and keeps
 * the history. */
int srt_set_denoise_history_feedback(srt_tracer *t, int enable);
int srt_group_set_denoise_history_feedback(srt_group *g, int enable);
/* 1 when the last pass 1 (a filter's or a clear's) was a feedback instantiation, else 0 (also for NULL, and after a filter
 * with K = 0). */
int srt_last_filter_history_feedback(srt_tracer *t);
int srt_group_last_filter_history_feedback(srt_group *g);

/* ---- albedo textures ----------------------------------------------------------
 * Opt-in: where a material has a texture bound, the colour that multiplies the path's mask (and the denoiser's albedo
 * guide) is the texel at the hit's UV instead of srt_material.color. Nothing else about a material changes and a lookup
 * draws no random numbers. With no texture bound the library launches exactly the kernels it launches without this
 * interface. show_normals ignores textures. Each of the three setters takes effect for later dispatches, does not clear
 * the canvas (the caller clears, as after srt_update_scene) and drops the denoiser's temporal history.
 *
 * UV, all float32, unfused, in the order written; X = the hit position the kernel shades:
 *   sphere  n = (X - centre) / radius;  u = dm_atan2pif(n.z, n.x) * 0.5 + 0.5;  v = n.y * 0.5 + 0.5
 *   plane   u = dot(X - position, T), v = dot(X - position, B), dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; the frame
 *           (srt_plane_frame_host) is made at srt_update_scene in double and rounded to float: a = the world axis on
 *           which |normal| is smallest (ties: x, then y, then z), T = normalise(a x n), B = n x T. A plane whose normal
 *           is zero or not finite has no frame and keeps the material colour.
 *   model   uv = (uv0 * w2 + uv1 * w0) + uv2 * w1 with the shading's barycentric weights (w0, w1 of render.cl:223-241,
 *           w2 = 1 - w0 - w1); without srt_set_triangle_uvs: uv = (w0, w1)
 * then u = u * scale_u, v = v * scale_v and the sampler over the W x H image, addressing REPEAT, fW = (float)W:
 *   NEAREST pu = u * fW, pv = v * fH; column floor(pu) mod W, row floor(pv) mod H (mod never negative); the texel as stored
 *   LINEAR  fu = u * fW - 0.5, fv = v * fH - 0.5; x0 = floor(fu), y0 = floor(fv); a = fu - x0, b = fv - y0; columns
 *           x0 mod W and (x0 + 1) mod W, rows likewise; w00 = (1-a)*(1-b), w10 = a*(1-b), w01 = (1-a)*b, w11 = a*b;
 *           channel = dm_bilinear(w00, T00, w10, T10, w01, T01, w11, T11) (csrc/detmath.h; T10 = column x0+1, row y0)
 *   A coordinate (pu, pv / fu, fv) that is NaN, infinite or not below 2^30 in magnitude: the texel (0, 0) as stored.
 * Texels are expected finite and not negative; they are not checked (as the skybox's are not). */

/* n images (n <= SRT_MAX_TEXTURES), copied; n == 0 (descs may be NULL) removes them all. SRT_ERR_INVALID: NULL texels,
 * width or height < 1 or > 16384, too many images. */
int srt_set_textures(srt_tracer *t, const srt_texture_desc *descs, size_t n);
/* One entry per material, in the material array's order; fewer entries than materials: none for the rest; NULL / 0 unbinds
 * everything. Checked at the next srt_update_scene and at every dispatch: a texture index at or beyond the image count (or
 * below -1), an unknown filter or a scale that is not finite is SRT_ERR_INVALID (entries beyond the scene's materials too
 * are checked). An srt_update_scene that fails one of these checks fails before anything is replaced: the handle keeps
 * its previous scene. */
int srt_set_material_textures(srt_tracer *t, const srt_material_texture *bindings, size_t n_materials);
/* n_triangles x 3 x 2 floats (u, v per vertex), parallel to the triangle array of srt_update_scene; NULL: no UVs.
 * A count that differs from the scene's triangle count is SRT_ERR_INVALID at the next srt_update_scene and at dispatches. */
int srt_set_triangle_uvs(srt_tracer *t, const float *uv, size_t n_triangles);
/* ---- per-triangle materials ----------------------------------------------------
 * Opt-in: one material index per triangle of the scene's triangle array, so that one model shape can carry several
 * materials (an OBJ's `usemtl` groups; host/parser.hpp hands them out). n_triangles int32 values parallel to
 * srt_update_scene's triangle array (as srt_set_triangle_uvs). -1: the triangle keeps its shape's material; m >= 0:
 * materials[m]. NULL / 0 removes them.
 *   which material  a hit on triangle k (index in the scene's triangle array: model.triangle_index + index in the model) of
 *                   a model whose shape material is >= 0 is shaded with materials[tm[k]] when tm[k] >= 0: the reference's
 *                   `closest = shape->material` (render.cl:334) made per triangle. Emission, the three probabilities,
 *                   smoothness, the refraction index, the colour and the texture binding all come from that material, in
 *                   the trace kernel and in the denoiser's albedo guide. show_normals ignores the table.
 *   hit / miss      stays the shape's: a model with material < 0 is a miss whatever its triangles say, and the table has no
 *                   "no material" value. The denoiser's shape ids stay the shape's.
 *   instances       two instances over one triangle range share the table's entries, as they share UVs.
 * The canvas equals that of the same scene with every model split into one model shape per maximal run of consecutive
 * triangles of one effective material (same transform and bounds, the run's triangle range and material, in the model's
 * place in the shape array). The setter behaves as the three texture setters: it takes effect for later dispatches, does
 * not clear the canvas and drops the denoiser's temporal history. A count that differs from the scene's triangle count, or
 * an entry below -1 or not below the scene's material count, is SRT_ERR_INVALID at the next srt_update_scene (which then
 * fails before anything is replaced: the handle keeps its previous scene) and at every dispatch. A table with an entry
 * >= 0 over a scene that has triangles makes the library launch the textured instantiations (srt_last_trace_textured
 * reports 1), with or without a texture bound; a NULL table, a table of only -1 or a scene without triangles launches
 * exactly what is launched without this interface. */
int srt_set_triangle_materials(srt_tracer *t, const int32_t *materials, size_t n_triangles);
/* Host-only: SRT_OK / SRT_ERR_INVALID for a table meeting a scene (count == scene_triangles, every entry in
 * [-1, n_materials)); NULL with n == 0: no table, SRT_OK. */
int srt_triangle_materials_check_host(const int32_t *materials, size_t n, size_t scene_triangles, size_t n_materials);
/* Which kernels the last srt_trace launched: *textured = 1 when the textured instantiations ran (some material of the
 * scene has a texture bound, or a per-triangle material table with an entry >= 0 is set over a scene with triangles --
 * the table is read by those instantiations alone), else 0. */
int srt_last_trace_textured(const srt_tracer *t, int *textured);
/* Which instantiation of the trace kernel the last srt_trace launched: *scene_class = 0 for the general kernels, 1 and up
 * for a kernel compiled for the scene's class (sphere / plane scenes of one block group). The class follows
 * the scene and the options of the dispatch; results do not depend on it. */
int srt_last_trace_class(const srt_tracer *t, int *scene_class);
/* Which twin of that class the last srt_trace launched: *plane_form = 0 for the class's own kernel (and for the general
 * kernels), else the scene's plane form, for which the class has an axis twin (DESIGN.md 5 "Axis planes"): 2 bits per plane
 * slot of the scene's block group in block order (block b, slot i: bits 4b + 2i), 1 / 2 / 3 = the plane's normal is +-e_x /
 * +-e_y / +-e_z. Results do not depend on it. */
int srt_last_trace_plane_form(const srt_tracer *t, int *plane_form);
/* Host-only (no device). The axis code srt_update_scene gives a plane: 1, 2, 3 when the normal has exactly one component
 * equal to +1 or -1 (x, y, z) and two zeros of either sign and every component of the position is at most 2^100 in
 * magnitude, else 0. SRT_ERR_INVALID on a NULL pointer. */
int srt_plane_axis_code_host(const float normal[3], const float position[3], int *code);
/* Host-only (no device). The integer srt_update_scene puts in place of a material probability p (metallic, specular,
 * transmittance): *threshold = the number of generator outputs r in [0, 2^32) with p > (float)r * 2^-32f, so that the kernel's
 * draw is r < *threshold. 0 for p <= 0 and NaN; below 2^32 for every p <= 1 (p = 1: 2^32 - 128, the 128 largest r convert to
 * 1.0); 2^32 for p > 1, which has no 32-bit threshold: a scene with such a probability keeps its float compares and runs the
 * general kernel. SRT_ERR_INVALID on a NULL pointer. */
int srt_bernoulli_threshold_host(float p, uint64_t *threshold);
/* Host-only (no device). The frame of a plane with this normal: returns 1 and writes T, B (3 floats each), or 0 when the
 * plane has none (T, B zeroed). */
int srt_plane_frame_host(const float normal[3], float T[3], float B[3]);
/* Host-only: the checks of the three setters and of their meeting a scene. SRT_OK or SRT_ERR_INVALID. descs may be NULL
 * when only the count matters (n_textures images assumed good); uv_triangles < 0: no UVs set. */
int srt_texture_check_host(const srt_texture_desc *descs, size_t n_textures, const srt_material_texture *bindings, size_t n_bindings,
                           long long uv_triangles, size_t scene_triangles);

/* ---- exposure for the resolve (new; no counterpart in the reference) ----------------------------------------------------
 * The plain resolve is canvas / ticks_stopped -> ACES fit -> sqrt -> bytes, one fixed curve. With exposure enabled every site
 * that resolves -- srt_resolve, srt_render, srt_render_async, srt_render_pipelined / srt_pipeline_flush, srt_resolve_denoised,
 * srt_resolve_gathered, srt_group_render, srt_group_resolve_denoised -- resolves as before and then overwrites its ARGB image
 * with tonemap(c * e) per channel, c the divided colour (with the handle's denoiser on: the image srt_read_denoised hands out)
 * and e the exposure, a float in device memory that the kernel reads there: no call waits for the host, a pipelined frame
 * included. At e == 1 the bytes are the plain resolve's. srt_resolve_external keeps the plain bytes. Off (the default): the
 * library launches what it launches without the feature.
 *
 * MANUAL: e = (float)2^ev, written into the device slot by srt_set_exposure. One more launch per frame.
 * AUTO, once per produced frame, on the handle's stream:
 *   histogram  L = 0.2126 r + 0.7152 g + 0.0722 b of the divided colour (float, unfused). A finite L > 0 goes into
 *              bin = clamp((bits(L) >> 21) - ((127 - 32) << 2), 0, 255): four bins per octave over 2^-32 .. 2^32, denormals in
 *              bin 0. Any other pixel (L zero, negative, inf, NaN) is left out and counted as such. Integer sums: exact.
 *   meter      N = the metered pixels in ascending bin order; kept are those numbered from N * low_permille / 1000 up to, not
 *              including, max(N * high_permille / 1000, that + 1) (integer divisions; a boundary bin contributes its part).
 *              mean = the kept pixels' mean of their bin's centre (bin + 0.5) / 4 - 32, accumulated in double in ascending bin
 *              order; target = clamp(log2(key) - mean, min_ev, max_ev); state = state + (target - state) * adapt when a state
 *              exists, else target; in double, stored as float. N == 0 leaves the state (0 on a fresh handle) and whether
 *              one exists as they are. Then log2_exposure = (float)(state + ev) and e = (float)2^log2_exposure.
 *   resolve    as above.
 * A partitioned handle meters the rows it owns; the gathered frame is metered by srt_resolve_gathered on the root. A group
 * keeps ONE state, on its first device, whichever of its two resolves (gathered, or denoised) a frame goes through.
 * srt_clear_canvas keeps the adaptation state; srt_reset_exposure and disabling forget it (the next metered frame adopts its
 * target). Changing the parameters while enabled keeps it. */
int srt_exposure_defaults(srt_exposure_params *out); /* AUTO, ev 0, key 0.18, 100..950 permille, adapt 1, min_ev -16, max_ev 16 */
/* Host-only: the validation srt_set_exposure applies to an enabled block (ranges as in srt_types.h, every float finite, adapt
 * in (0, 1], reserved 0). SRT_OK or SRT_ERR_INVALID. */
int srt_exposure_check_host(const srt_exposure_params *p);
/* p NULL or enable == 0: off, and the adaptation state is forgotten. SRT_ERR_INVALID as srt_exposure_check_host. Asynchronous. */
int srt_set_exposure(srt_tracer *t, const srt_exposure_params *p);
int srt_group_set_exposure(srt_group *g, const srt_exposure_params *p);
int srt_reset_exposure(srt_tracer *t);
int srt_group_reset_exposure(srt_group *g);
/* Waits for the handle's stream. log2_exposure, exposure: what the last exposed resolve multiplied with (0 and 1 before the
 * feature was ever enabled); hist, counts = {metered pixels, pixels left out}: the last metered frame's (zeros before one; MANUAL
 * meters nothing). Any pointer may be NULL. */
int srt_read_exposure(srt_tracer *t, float *log2_exposure, float *exposure, uint32_t hist[256], uint32_t counts[2]);
int srt_group_read_exposure(srt_group *g, float *log2_exposure, float *exposure, uint32_t hist[256], uint32_t counts[2]);
/* For tests: *exposed = 1 when the last resolving call on the handle (the group: on its first device) ran the exposed resolve. */
int srt_last_resolve_exposed(const srt_tracer *t, int *exposed);
int srt_group_last_resolve_exposed(const srt_group *g, int *exposed);

/* ---- bloom for the resolve (new; no counterpart in the reference) -------------------------------------------------------
 * With bloom enabled every site that resolves a picture (the list above) resolves as before and then overwrites its ARGB image
 * with tonemap(x + intensity * glow), on the handle's stream, without a wait for the host. With exposure on as well the
 * composite takes the place of the exposed resolve; exposure metering keeps reading the un-bloomed colour. Off (the default):
 * the library launches what it launches without the feature. srt_resolve_external keeps the plain bytes. A handle that holds
 * interleaved rows (srt_set_partition with world > 1, a group member) is not a picture: its own resolve is not bloomed and
 * srt_last_resolve_bloomed reports 0; the gathered frame (srt_resolve_gathered, srt_group_render, srt_group_resolve_denoised)
 * is bloomed on the root. A group keeps ONE state, on its first device.
 *
 * The arithmetic is float, unfused, in the order written here; / is correctly rounded. x = (c / divisor) * e per channel is
 * the colour the site exposes: c the canvas and divisor (float)ticks_stopped, or the denoiser's image and 1; e the exposure
 * scalar in device memory with exposure on, else 1.0f. Alpha is never used; a pyramid texel's alpha is 0.
 *   1 prefilter, per pixel: L = 0.2126 x.r + 0.7152 x.g + 0.0722 x.b (left to right). If any of x.r, x.g, x.b, L is not
 *     finite, or !(L > 0), the pixel contributes (0, 0, 0). Otherwise g = L - threshold; if knee > 0: s = clamp((L - threshold)
 *     + knee, 0, 2 * knee), q = (s * s) / (4 * knee), g = max(g, q); if clamp > 0: g = min(g, clamp); if !(g > 0) the pixel
 *     contributes 0, otherwise bright = x * (g / L): one division, three products.
 *   2 reduce, level k - 1 (level 0: the prefiltered frame) to level k: w_k = (w_{k-1} + 1) / 2, h_k = (h_{k-1} + 1) / 2.
 *     Separable, horizontal first into a w_k x h_{k-1} intermediate, then vertical. Destination index i takes source indices
 *     2i-1, 2i, 2i+1, 2i+2, clamped to the edge, as a, b, c, d: ((a + d) + 3.0f * (b + c)) * 0.125f. The effective level
 *     count is `levels`, cut off after the first level that is 1 x 1.
 *   3 expand-and-add, from the top level down: up_last = down_last; up_k = down_k + scatter * expand(up_{k+1}). expand is
 *     separable, horizontal first: destination 2i is 0.75f * s[i] + 0.25f * s[i-1], destination 2i+1 is 0.75f * s[i] +
 *     0.25f * s[i+1], source indices clamped to the edge. In place: one pyramid per handle.
 *   4 composite, at full resolution: out = x + intensity * expand(up_0) per channel; argb = tonemap(out). */
int srt_bloom_defaults(srt_bloom_params *out); /* enable 1, threshold 1, knee 0.5, intensity 0.1, scatter 0.7, clamp 64, levels 6 */
/* Host-only: the validation srt_set_bloom applies to an enabled block (ranges as in srt_types.h, every float finite, reserved 0).
 * SRT_OK or SRT_ERR_INVALID. */
int srt_bloom_check_host(const srt_bloom_params *p);
/* p NULL or enable == 0: off. SRT_ERR_INVALID as srt_bloom_check_host. The first enabling call allocates the handle's pyramid
 * (about a third of a frame's float4). */
int srt_set_bloom(srt_tracer *t, const srt_bloom_params *p);
int srt_group_set_bloom(srt_group *g, const srt_bloom_params *p);
/* Waits for the handle's stream. up_level of the last bloomed frame: *w x *h texels of 4 floats (r, g, b, 0) into rgba_out, of
 * cap_pixels texels; rgba_out NULL: the size only. SRT_ERR_INVALID: level outside 0 .. the frame's effective level count - 1,
 * or cap_pixels too small; SRT_ERR_STATE: no bloomed frame yet. w, h may be NULL. */
int srt_read_bloom(srt_tracer *t, int level, float *rgba_out, size_t cap_pixels, int *w, int *h);
int srt_group_read_bloom(srt_group *g, int level, float *rgba_out, size_t cap_pixels, int *w, int *h);
/* For tests: *bloomed = 1 when the last resolving call on the handle (the group: on its first device) ran the bloom composite. */
int srt_last_resolve_bloomed(const srt_tracer *t, int *bloomed);
int srt_group_last_resolve_bloomed(const srt_group *g, int *bloomed);

/* ---- noise metering and render-until-converged (new; no counterpart in the reference) ----------------------------------
 * With the denoiser on (srt_set_denoise; iterations = 0 is enough) every dispatch adds (1/n) sum lum(radiance)^2 per pixel to
 * the moments plane beside the canvas, and the handle counts the dispatches T and the samples P since the clear. One pass
 * over both gives every pixel a relative standard error of its mean, a 256-bin histogram of it and the number of pixels
 * below a threshold; the host turns the histogram into a noise level and a stopping rule. Off (the default): every call
 * enqueues exactly what it enqueues without the feature. Needs the handle's denoiser on (else SRT_ERR_STATE); not available
 * on a partitioned handle. A group keeps ONE state, on its first device, and meters the gathered planes there.
 *
 * THE DEFINITION (float32, every operation rounded on its own -- no fused multiply-add --, in the order written). For pixel q,
 * with Tf = (float)T, Pf = (float)P:
 *   L  = lum(canvas.r / Tf, canvas.g / Tf, canvas.b / Tf)      lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b
 *   m2 = moments[q] / Tf
 *   the pixel is left out (and counted as such) unless L and m2 are both finite
 *   v  = m2 - L * L;  v = (v > 0) ? v : 0
 *   se = sqrt(v / Pf)                                           the correctly rounded square root
 *   d  = (L > luminance_floor) ? L : luminance_floor
 *   r  = se / d                                                 IEEE division; the pixel is left out if r is not finite
 *   bin = clamp((int)(bits(r) >> 20) - ((127 - 24) << 3), 0, 255)    eight bins per octave over 2^-24 .. 2^8; r == 0 and denormals in bin 0
 *   below += (r <= threshold)
 * hist[256], metered, left_out and below are exact integer sums. The noise level is the upper edge of the bin in which the
 * ascending cumulative count first reaches (metered * permille + 999) / 1000, computed on the host as
 *   level = ldexpf(SRT_NOISE_EIGHTHS[(bin + 1) & 7], ((bin + 1) >> 3) - 24)
 * with the table below (2^(k/8) rounded to float; no exp2 enters the result). The bins cut an octave by mantissa bits, at
 * 1 + k/8, and the level quotes 2^(k/8): the two agree at the octave's ends, and inside the level lies within the bin, up to
 * 6 % below its upper edge. And
 *   converged = metered > 0 && P >= min_samples && (uint64)below * 1000 >= (uint64)permille * metered.
 * Two weaknesses of the estimator: dispatches with different num_samples are weighted equally in m2, so the estimate is exact
 * only when every dispatch since the clear had the same sample count. And a pixel whose rare bright paths have not been
 * sampled yet has a small sample variance and reads as converged: the rule cannot see light it has not found. */
#define SRT_NOISE_EIGHTHS {0x1.000000p+0f, 0x1.172b84p+0f, 0x1.306fe0p+0f, 0x1.4bfdaep+0f, 0x1.6a09e6p+0f, 0x1.8ace54p+0f, 0x1.ae89fap+0f, 0x1.d5818ep+0f}
int srt_noise_defaults(srt_noise_params *out); /* enable 1, threshold 0.05, luminance_floor 0.01, permille 950, min_samples 16, check_every 4 */
/* Host-only: the validation srt_set_noise_meter applies to an enabled block (ranges as in srt_types.h, floats finite, reserved 0).
 * SRT_OK or SRT_ERR_INVALID. */
int srt_noise_check_host(const srt_noise_params *p);
/* Host-only: the percentile, the level and the stopping rule as the read calls apply them to a record: hist[256],
 * counts = {metered, left_out, below}, the T and P of the metering, params' permille and min_samples. */
int srt_noise_evaluate_host(const uint32_t hist[256], const uint32_t counts[3], uint32_t T, uint32_t P, const srt_noise_params *params, srt_noise_result *result);
/* p NULL or enable == 0: off (a metering in flight stays readable). SRT_ERR_INVALID as srt_noise_check_host; SRT_ERR_STATE: the
 * denoiser is off, or the handle is partitioned. The first enabling call allocates the device record and its pinned copies. */
int srt_set_noise_meter(srt_tracer *t, const srt_noise_params *p);
int srt_group_set_noise_meter(srt_group *g, const srt_noise_params *p); /* the group's denoiser must be on (srt_group_set_denoise) */
/* Asynchronous: on the handle's stream, behind what it holds, zeroes the record, launches the meter kernel over the canvas and
 * the moments and copies the record (1,060 bytes) into pinned memory behind an event. SRT_ERR_STATE: the meter or the
 * denoiser is off, or nothing is traced since the clear. */
int srt_meter_noise(srt_tracer *t);
int srt_group_meter_noise(srt_group *g); /* over the planes the last srt_group_trace_and_gather / srt_group_render gathered */
/* The newest metering's result (the calls above, srt_resolve_noise_view, an automatic one). srt_poll_noise never blocks:
 * *ready = 0 while the copy is in flight (result and hist are not written then). srt_read_noise waits for that copy's event
 * only, not for the stream. hist may be NULL. Where nothing was ever metered on the handle srt_poll_noise reports *ready = 0
 * and srt_read_noise returns SRT_ERR_STATE. */
int srt_poll_noise(srt_tracer *t, srt_noise_result *result, uint32_t hist[256], int *ready);
int srt_read_noise(srt_tracer *t, srt_noise_result *result, uint32_t hist[256]);
int srt_group_poll_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256], int *ready);
int srt_group_read_noise(srt_group *g, srt_noise_result *result, uint32_t hist[256]);
/* Asynchronous: meters as srt_meter_noise and, in the same pass, overwrites the handle's ARGB image (srt_read_argb) with a heat
 * map. With bin(x) the bin formula above, bt = bin(threshold) and dd = clamp(bin(r) - bt + 32, 0, 64) a pixel is
 * R = dd * 255 / 64 (integer), G = 255 - R, B = 0; a left-out pixel is R = 255, G = 0, B = 255. Bytes as the resolve packs
 * them: 255 | R << 8 | G << 16 | B << 24. Green is four octaves below the threshold, red four above. */
int srt_resolve_noise_view(srt_tracer *t);
int srt_group_resolve_noise_view(srt_group *g);
int srt_group_read_noise_view(srt_group *g, uint8_t *argb_out); /* blocking: the group's width * height * 4 heat map bytes (one entry point beyond the handle's: a group has no srt_read_argb) */
/* Blocking, like srt_render: traces until a check converges. Dispatch i (from 0) is srt_trace with options->time + i *
 * time_stride (uint32 arithmetic). After every dispatch that makes T % check_every == 0 with P >= min_samples a metering is
 * enqueued (check k); the call then waits for the copy event of check k - 1, and only for that, and stops if that check
 * converged -- so the device always has one interval queued while the host waits, and the stop does not depend on timing:
 * counted from a clear, *dispatches_done = min(T* + check_every, max_dispatches), T* the T of the first converged check. At
 * max_dispatches the outstanding check is waited for and reported; converged = 0 unless it converged. The frame is then
 * resolved as srt_resolve_denoised(t, T) resolves it (the filter when iterations >= 1, exposure and bloom as configured) and
 * read into argb_out. *result is the deciding check's (result->dispatches = T*); all zero, level_bin -1, when no check ran.
 * T and P count from the last clear: dispatches traced before the call count. SRT_ERR_STATE: the meter or the denoiser is off. */
int srt_render_until(srt_tracer *t, const srt_render_data *options, uint32_t time_stride, uint32_t max_dispatches, uint8_t *argb_out,
                     srt_noise_result *result, uint32_t *dispatches_done);
/* Automatic metering: srt_render, srt_render_async and srt_render_pipelined meter the frame behind their resolve when the meter
 * is on and T % check_every == 0, so a front-end only polls. For tests: *ran = 1 when the last of these calls metered. */
int srt_last_meter_ran(const srt_tracer *t, int *ran);
/* For tests: uploads num_pixels float4 of a canvas and num_pixels floats of moments and runs the meter kernel on them as a
 * metering of a frame with these T, P and params would (view_out NULL: the metering instantiation; else the view one, and
 * num_pixels * 4 heat map bytes into view_out). counts_out = {metered, left_out, below}. Blocking. num_pixels 1..2^24. */
int srt_selftest_noise_meter(srt_tracer *t, const float *canvas_host, const float *moments_host, uint32_t num_pixels, uint32_t T, uint32_t P,
                             const srt_noise_params *params, uint32_t hist_out[256], uint32_t counts_out[3], uint8_t *view_out);

/* ---- ray queries (new): closest hits for caller rays, picking ------------------------------------------------------------- */

/* The closest hit of each of n rays in the handle's scene -- its run/block layout, world triangles, hierarchy (built, refitted
 * or device-built, whatever the last srt_update_scene left) and materials -- without rendering: what is under the mouse, where
 * an object dropped along a ray lands, a line of sight (hit.t < tmax). Records: srt_ray, srt_ray_hit (srt_types.h).
 *
 * SAME RAY, SAME HIT. A ray is what the trace kernels' EXTEND gets:
 *   - it starts at its origin, with the intersectors' own self-intersection rule and no tmin of its own;
 *   - the direction is normalised with the kernels' normalize3 (a * rsqrt(dot(a, a)), detmath's rsqrt), unless
 *     SRT_RAYS_UNIT_DIRECTIONS says it is already unit length: the caller's bits are then used as given, because normalising
 *     an already normalised vector can change bits;
 *   - tmax is the value the closest distance starts from (+inf is allowed); a hit is closer than tmax, strictly, by the
 *     kernels' take_if_closer (so tmax <= 0, -0 and -inf included, is a miss that is not traversed);
 *   - ties between shapes go to the first in array order, as in the trace; within a model to the lower triangle index;
 *   - t is a world distance along the unit direction.
 * THE RECORD.
 *   - shape: the index in the array srt_update_scene was given, SRT_HIT_NONE (0xffffffff) for a miss;
 *   - triangle: the index inside its model (under a hierarchy, the leaf record's index), SRT_HIT_NONE for spheres, planes, misses;
 *   - normal: the trace's hit normal (winner_normal) turned to face the ray. SRT_HIT_FRONT is set when the ray met the front
 *     face -- dot(normal as stored, direction) < 0, nothing had to be turned -- and clear when the normal was negated (a back
 *     face: the inside of a sphere, the underside of a plane);
 *   - material: the one the trace would shade with: the per-triangle index where srt_set_triangle_materials gave one that is
 *     not -1, else the shape's;
 *   - a shape WITHOUT a material (index < 0) IS REPORTED, with material = -1 (whatever the per-triangle table says) and
 *     SRT_HIT_HIT set, unlike the trace, which treats it as sky (render.cl:404): a picker must be able to select such a shape;
 *   - a miss: t = +inf, shape = triangle = SRT_HIT_NONE, material = -1, a zero normal, flags 0.
 * HOSTILE RAYS. A ray is invalid if any origin or direction component is not finite, if tmax is NaN, or if the direction is
 * zero or does not normalise to a finite vector of unit length (squared length outside (0.25, 4) after normalize3 -- 1e-30: the
 * squared length underflows; 1e30: it overflows). It is
 * not traversed and gets the miss record with SRT_HIT_INVALID_RAY. The DEVICE decides this: device-resident rays never pass
 * the host. No ray makes the walk run on or read outside the scene's buffers, and the call still returns SRT_OK.
 * STATE. A query reads the scene as the last srt_update_scene left it, ordered on the handle's stream behind the pre-pass,
 * refit and build that update enqueued: a cast after a device refit sees the refitted boxes. It writes nothing but its outputs
 * and a staging buffer of its own (bringing the per-triangle material table up to date, as the next dispatch would, aside):
 * canvas, counters, denoiser planes, exposure and noise state stay as they were, and so does every srt_last_trace_* answer.
 * Before any scene is set every valid ray misses.
 * COUNTS AND ERRORS. n == 0: SRT_OK, no launch. A null pointer with n > 0, unknown flag bits, n >= 2^31, a device pointer not
 * aligned to 16 bytes: SRT_ERR_INVALID. The host forms keep ONE growing staging allocation per handle (72 B per ray of the
 * largest call; the occlusion queries below share it), freed in srt_destroy.
 *
 * srt_cast_rays: host arrays, blocking. srt_cast_rays_device: n srt_ray / n srt_ray_hit in device memory of the handle's
 * device, each 16-byte aligned, asynchronous on the handle's stream (srt_synchronize, or work on the bound stream, follows). */
int srt_cast_rays(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits);
int srt_cast_rays_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *hits_dev);
/* Picking: the hits under n points of the image, xy = {x0, y0, x1, y1, ...} in CONTINUOUS pixel coordinates (x to the right, y
 * down, the pixel (px, py) covers [px, px + 1) x [py, py + 1)), blocking. A small second kernel makes the rays on the device
 * with the statements of the trace's CAMERA phase -- ndc = (x / width, y / height) through the host's reciprocals, the aspect
 * and fov lines, the camera matrix's columns, normalize3, origin camera_to_world[3] -- with the caller's x, y in place of
 * (float)px + random_float(seed); it writes into the staging buffer and the cast follows with unit directions. So
 * xy = (px + 0.5, py + 0.5) is the pixel's centre ray, and xy = ((float)px + r0, (float)py + r1) with the two random floats of a
 * sample is that sample's primary ray bit for bit. `options` supplies only the camera (camera_to_world, aspect_ratio,
 * fov_scale) and the frame size (width, height, both > 0), which need not be the handle's. A partitioned handle or a group
 * member answers for GLOBAL pixel coordinates: every member holds the whole scene. Coordinates outside the frame give the rays
 * the same formulas give (NaN: an invalid ray). */
int srt_pick(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits);
/* On the group's first member: every member holds the scene. */
int srt_group_cast_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, srt_ray_hit *hits);
int srt_group_pick(srt_group *g, const srt_render_data *options, const float *xy, size_t n, srt_ray_hit *hits);
/* With srt_set_kernel_timers on: the device time of the last query's launches (the cast; for srt_pick the ray set-up too), in
 * milliseconds; 0 when the timers were off or nothing was launched. Blocking, as srt_last_kernel_ms. */
int srt_last_ray_query_ms(srt_tracer *t, float *ms);
/* Host-only: out = {sizeof(srt_ray), sizeof(srt_ray_hit)} as the library was built. */
int srt_ray_query_sizes(size_t out[2]);

/* ---- nearest-surface queries (new): the closest scene point to caller points ------------------------------------------------ */

/* For each of n points, the closest point of the handle's scene and how far away it is: snapping a dragged object or a gizmo
 * handle to the nearest face, edge or vertex, clearance checks ("is anything within 0.2 of here"), dropping an object onto
 * whatever is nearest, baking a distance field. Records: srt_point_query, srt_nearest (srt_types.h).
 *
 * THE ANSWER IS A MINIMUM OVER PRIMITIVES, so it does not depend on how the scene is traversed. A primitive is every sphere,
 * every plane and every triangle of every model of the scene the last srt_update_scene left (a model's triangles are searched
 * where its record's bounding box, which the caller supplies, says they are: as the cast trusts it). Each has ONE distance
 * function, below; the record reports the primitive with the smallest `distance`, compared as a float:
 *   - ties go to the lower shape index, then to the lower triangle index inside the model;
 *   - a primitive is taken only when distance < max_distance, strictly, as the cast treats tmax;
 *   - a NaN distance is never taken: a non-finite or collinear triangle may give one, a plane with a zero or non-finite normal
 *     does;
 *   - skip_shape (per call; SRT_HIT_NONE: none) is left out entirely: usually the object being dragged, which would always be
 *     its own nearest.
 * The array scan, the host's SAH hierarchy, the device-built Morton and median hierarchies and a refitted hierarchy therefore
 * give the same 32 bytes.
 * ARITHMETIC. float32, every product, sum, difference, IEEE quotient and correctly rounded square root rounded by itself
 * (nothing fused), in the order written. dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z; cross(a, b) = (a.y * b.z - a.z * b.y,
 * a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); vector forms are per component. q is the query point. One implementation,
 * csrc/nearest_math.h, is compiled into the kernels and into the host exports below.
 *   Sphere (centre c, r = |radius|): v = q - c, len = sqrt(dot3(v, v)), distance = |len - r|. point = c + v * (r / len) when
 *     len > 0, else c + (r, 0, 0). BACK when len < r. Feature 0.
 *   Plane (p, n as stored, not assumed unit): nn = dot3(n, n), k = dot3(q - p, n), distance = |k / sqrt(nn)|,
 *     point = q - n * (k / nn). BACK when k < 0. Feature 0.
 *   Triangle, over the pre-pass's world record {v0, e1, e2} (the bits the kernels hold; v1 and v2 are NOT recomputed from model
 *     space): Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5) with a = v0, ab = e1, ac = e2:
 *       ap = q - a, bp = ap - e1, cp = ap - e2,
 *       d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp),
 *       vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
 *     the first region of this list that holds is taken, and its number is the feature code:
 *       1  vertex v0:  d1 <= 0 and d2 <= 0                          point = a
 *       2  vertex v1:  d3 >= 0 and d4 <= d3                         point = a + e1
 *       4  edge v0v1:  vc <= 0 and d1 >= 0 and d3 <= 0              point = a + e1 * (d1 / (d1 - d3))
 *       3  vertex v2:  d6 >= 0 and d5 <= d6                         point = a + e2
 *       5  edge v0v2:  vb <= 0 and d2 >= 0 and d6 <= 0              point = a + e2 * (d2 / (d2 - d6))
 *       6  edge v1v2:  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    point = (a + e1) + (e2 - e1) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
 *       0  the face:   otherwise; denom = 1 / ((va + vb) + vc)      point = (a + e1 * (vb * denom)) + e2 * (vc * denom)
 *     distance = sqrt(dot3(q - point, q - point)). BACK when dot3(q - point, cross(e1, e2)) < 0. A triangle whose e1 and e2 are
 *     both zero is its vertex v0.
 * THE RECORD.
 *   - found: distance, shape (the index srt_update_scene was given), triangle (inside its model; SRT_HIT_NONE for a sphere or a
 *     plane), point, flags = SRT_NEAREST_FOUND | SRT_NEAREST_BACK if so | feature << SRT_NEAREST_FEATURE_SHIFT;
 *   - material: the cast's rule: the per-triangle index where srt_set_triangle_materials gave one that is not -1, else the
 *     shape's; a shape WITHOUT a material (index < 0) IS REPORTED, with material = -1;
 *   - nothing within max_distance: distance = +inf, shape = triangle = SRT_HIT_NONE, material = -1, a zero point, flags 0.
 * HOSTILE QUERIES, decided on the device. A non-finite point component or a NaN max_distance: the nothing record with
 * SRT_NEAREST_INVALID, and the scene is not traversed. max_distance <= 0 (-0 and -inf included): a valid nothing record, not
 * traversed. No query makes the walk run on or read outside the scene's buffers, and the call still returns SRT_OK. Before any
 * scene is set every query finds nothing.
 * STATE. A query reads the scene as the last srt_update_scene left it, ordered on the handle's stream behind the pre-pass,
 * refit and build that update enqueued: a query after a device refit sees the refitted boxes. It writes nothing but its outputs
 * and the queries' shared staging allocation (bringing the per-triangle material table up to date, as the cast does, aside):
 * canvas, counters, denoiser planes, exposure and noise state stay as they were, and so does every srt_last_trace_* answer.
 * srt_last_ray_query_ms covers the launch.
 * COUNTS AND ERRORS. n == 0: SRT_OK, no launch. A null pointer with n > 0, n >= 2^31, a device pointer not aligned to 16 bytes,
 * a skip_shape that is neither SRT_HIT_NONE nor below the scene's shape count: SRT_ERR_INVALID.
 *
 * srt_nearest_points: host arrays, blocking. srt_nearest_points_device: n srt_point_query / n srt_nearest in device memory of the
 * handle's device, each 16-byte aligned, asynchronous on the handle's stream. srt_group_nearest_points: on the group's first
 * member (every member holds the scene). */
int srt_nearest_points(srt_tracer *t, const srt_point_query *queries, size_t n, uint32_t skip_shape, srt_nearest *out);
int srt_nearest_points_device(srt_tracer *t, const void *queries_dev, size_t n, uint32_t skip_shape, void *out_dev);
int srt_group_nearest_points(srt_group *g, const srt_point_query *queries, size_t n, uint32_t skip_shape, srt_nearest *out);
/* Host-only, no device and no handle: the three distance functions as the kernels compile them (csrc/nearest_math.h). wtri: a
 * world record {v0, e1, e2}; *flags: SRT_NEAREST_BACK if so | feature << SRT_NEAREST_FEATURE_SHIFT (never FOUND: that is the
 * minimum's word). SRT_ERR_INVALID for a NULL argument. */
int srt_nearest_triangle_host(const float wtri[9], const float q[3], float *distance, float point[3], uint32_t *flags);
int srt_nearest_sphere_host(const float centre[3], float radius, const float q[3], float *distance, float point[3], uint32_t *flags);
int srt_nearest_plane_host(const float position[3], const float normal[3], const float q[3], float *distance, float point[3], uint32_t *flags);
/* Host-only: out = {sizeof(srt_point_query), sizeof(srt_nearest)} as the library was built. */
int srt_nearest_sizes(size_t out[2]);

/* ---- occlusion queries (new): any-hit rays and segments with early exit ---------------------------------------------------- */

/* Is anything in the handle's scene closer than tmax along each of n rays -- is B visible from A, does a place have a clear
 * line to the light, which of these sample points see the sun -- answered as one bit per ray. What a cast answers with
 * hit.t < tmax, without the rest of the cast: the walk stops at a ray's first hit instead of looking for the closest, nothing
 * is fetched for a normal or a material, and 32 bytes go in and 2 bits come out per ray. Records: srt_ray, srt_segment.
 *
 * THE ANSWER is a bit mask: ray q is bit q & 63 of 64-bit word q >> 6, ceil(n / 64) words. The bits of the last word past n are
 * written as 0; words past the last are not touched. `invalid` (may be NULL: then it is not written) has the same layout.
 * SAME RAY, SAME ANSWER. Bit q of `occluded` is set exactly when srt_cast_rays of the same ray with the same flags would set
 * SRT_HIT_HIT; the ray contract of "ray queries" above holds unchanged:
 *   - the ray starts at its origin, with the intersectors' own self-intersection rule and no tmin of its own;
 *   - the direction is normalised with the kernels' normalize3 unless SRT_RAYS_UNIT_DIRECTIONS is given;
 *   - tmax is the strict bound: a surface at exactly tmax does not occlude, and tmax <= 0 (-0 and -inf included) is not
 *     traversed: visible;
 *   - a shape WITHOUT a material (index < 0) OCCLUDES, as the cast reports it, unlike the trace, which shows the sky through it;
 *     so does glass: the answer is about geometry, not about light;
 *   - the tests are the cast's own (spheres, planes, the model boxes, Moller-Trumbore, the hierarchy's padded boxes and
 *     slack), against a limit that stays at tmax; which of several occluders is met first is not defined and not reported.
 * HOSTILE RAYS. The cast's validity rules, decided on the DEVICE: an invalid ray is not traversed, is NOT occluded, and has its
 * bit set in `invalid` when that mask is given. No ray makes the walk run on or read outside the scene's buffers, and the call
 * still returns SRT_OK.
 * SEGMENTS. srt_segment {from, end_gap, to, reserved = 0}: a small kernel turns each into an srt_ray in the handle's staging
 * buffer with functions the kernels already have -- d = to - from, direction = normalize3(d), tmax = dot3(d, direction) -
 * end_gap, origin = from -- and the occlusion launch follows with unit directions. end_gap > 0 keeps the end's own surface
 * from occluding a point that lies on it (tmax is then the distance to a point end_gap in front of `to`). from == to (a zero
 * direction), a non-finite component, a negative or non-finite end_gap and a non-zero `reserved` (tmax = NaN) give an invalid
 * ray by the rules above. srt_segment_rays returns exactly those records (blocking), so
 * srt_occluded_rays(srt_segment_rays(segs), SRT_RAYS_UNIT_DIRECTIONS) equals srt_occluded_segments(segs) bit for bit.
 * STATE. As a cast: the scene as the last srt_update_scene left it, ordered on the handle's stream behind that update's
 * pre-pass, refit and build. Outputs are written only to the caller's arrays and to the handle's ONE staging allocation, the
 * ray queries' own (now the largest of 72 B per ray of a cast or pick and 64 B per ray + 16 B per 64 rays of a call here);
 * canvas, counters, denoiser planes, exposure and noise state stay as they were, and so does every srt_last_trace_* answer.
 * Before any scene is set every valid ray is visible. srt_last_ray_query_ms covers these launches too (for the segment form,
 * the ray set-up and the occlusion launch).
 * COUNTS AND ERRORS. n == 0: SRT_OK, no launch. A NULL required pointer with n > 0 (`invalid` alone is optional in the ray
 * forms), unknown flag bits, n >= 2^31, device rays not aligned to 16 bytes or a device mask not aligned to 8: SRT_ERR_INVALID.
 *
 * srt_occluded_rays / srt_occluded_segments: host arrays, blocking. srt_occluded_rays_device: n srt_ray and the mask words in
 * device memory of the handle's device, asynchronous on the handle's stream. */
int srt_occluded_rays(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t flags, uint64_t *occluded, uint64_t *invalid /* may be NULL */);
int srt_occluded_rays_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t flags, void *occluded_dev, void *invalid_dev /* may be NULL */);
int srt_occluded_segments(srt_tracer *t, const srt_segment *segs, size_t n, uint64_t *occluded, uint64_t *invalid /* may be NULL */);
/* The rays the segment form casts, n srt_ray; blocking. */
int srt_segment_rays(srt_tracer *t, const srt_segment *segs, size_t n, srt_ray *rays_out);
/* On the group's first member, as srt_group_cast_rays. */
int srt_group_occluded_rays(srt_group *g, const srt_ray *rays, size_t n, uint32_t flags, uint64_t *occluded, uint64_t *invalid);
int srt_group_occluded_segments(srt_group *g, const srt_segment *segs, size_t n, uint64_t *occluded, uint64_t *invalid);
int srt_group_segment_rays(srt_group *g, const srt_segment *segs, size_t n, srt_ray *rays_out);
/* Host-only: out = {sizeof(srt_segment), the bytes of one mask word (8)} as the library was built. */
int srt_occlusion_sizes(size_t out[2]);

/* Device self-test of the deterministic math (tests only). Walks r = 0, stride, ... over
 * all 2^32 RNG outputs: out[0..2] = mismatch counts of the kernel-local sqrt / log / cos
 * specialisations against their generic definitions (must be 0); out[3..7] = sums of the
 * result bit patterns of detmath's log, cos, sqrt, atan2pi, pow on the device, to be
 * compared with the same sums from the host build of csrc/detmath.h; out[8], out[10] = mismatch
 * counts of the kernel's shared-reciprocal division (both forms: the reciprocal refined on the device, and the host's
 * rounded reciprocal of a sphere's radius with its out-of-range marker 0) and its unguarded Box-Muller square root
 * against IEEE `/` and sqrt (must be 0); out[9] = sum of the result bits of the built-in
 * normalize (detmath's division-free rsqrt), again for comparison with the host build; out[11] = mismatch count of the
 * RNG-scaling shortcuts (log of the raw count, theta from the raw count) against the plain forms
 * (must be 0); out[12] = mismatch count of the kernel's reciprocal-root square root against IEEE sqrt on
 * the floats in [2^-96, inf) (all of them at stride 1; must be 0); out[13] = mismatch count of the camera
 * rays' division by the image size through the host's reciprocal against IEEE `/` (must be 0);
 * out[14] = mismatch count of the kernel's branch-free sign() against detmath's on all bit patterns (must be 0);
 * out[15] = mismatch count of the sun lobe's power with a wave-uniform integer exponent against detmath's dm_powi, exponents
 * 1..32 over the RNG outputs, their negatives and all bit patterns (must be 0). */
int srt_selftest_math(srt_tracer *t, uint32_t stride, uint64_t out[16]);

/* Device self-test of the trace kernel's wave-level votes (tests only): the bounce's three Box-Muller normals (what = 0), its
 * vector-times-sign (what = 1) as the kernel runs them -- one vote per wave, then
 * the fast or the rare form on all its lanes -- against the per-lane forms. Lane i of wave i / 64 reads in[8 * i ..]:
 * {seed} / {vx, vy, vz, d} (float bits), and writes four words of each result to out_new and
 * out_ref ({x, y, z, seed afterwards} / {x, y, z, 0}); *mismatches = the number of words whose bits differ (must be 0 wherever
 * a NaN component comes with a NaN d, as it does in the kernel). waves <= 65536. */
int srt_selftest_rare_lanes(srt_tracer *t, int what, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, uint64_t *mismatches);

/* Device self-test of the axis twins' plane tests (tests only; DESIGN.md 5 "Axis planes"), for the benchmark's plane form
 * (planes y, x | plane z): planes[32] = the two staged plane blocks, {p, 0, n, 0} x 2 each (the fourth slot a filler). Each wave
 * runs what an EXTEND phase of the twin runs for its planes -- the guard, its vote, then the folded tests or the reference's
 * on all lanes -- and, beside it, test_planes2 alone. what = 0: lane i reads in[8 * i ..] = {org, dir, tmin} (float bits);
 * what = 1, as in a camera phase: every lane's origin is cam_org[3] (so the numerators are the same for the whole
 * wave), the lane reads {-, -, -, dir, tmin}. out_new / out_ref: {tmin, best} per lane (best counts from 0; -1: none); fast[w] = 1 when wave w passed the
 * guard; *mismatches = the words of out_new that differ from out_ref (must be 0). waves <= 65536. */
int srt_selftest_plane_forms(srt_tracer *t, int what, const float planes[32], const float cam_org[3], const uint32_t *in, uint32_t waves,
                             uint32_t *out_new, uint32_t *out_ref, uint32_t *fast, uint64_t *mismatches);

/* Device self-test of the NO_SPEC scene classes' diffuse-wave bounce (tests only; DESIGN.md 5 "Diffuse waves"). Each wave runs
 * what a SHADE phase runs between random_dir and SHADE_TAIL -- the vote on the materials, the vote on the operands, then the
 * short form (dir = random_dir, mask * colour, the generator three steps on) or the per-lane form on all 64 lanes -- and, beside
 * it, the per-lane form alone. Lane i reads in[20 * i ..] = {random_dir, dir, nrm, metallic threshold, transmittance threshold,
 * smoothness, mask, colour (float bits; the thresholds are the 32-bit draw thresholds), seed, unused} and writes eight words of
 * each result: {dir, mask, seed afterwards, 1 where the lane drew transparent (its dir is then the rough direction the glass
 * branch goes on from)}. fast[w] = 1 when wave w took the short form; *mismatches = the words of out_new that differ from
 * out_ref (must be 0). waves <= 65536. */
int srt_selftest_diffuse_bounce(srt_tracer *t, const uint32_t *in, uint32_t waves, uint32_t *out_new, uint32_t *out_ref, uint32_t *fast, uint64_t *mismatches);

/* ---- selection overlay and the ID pass (new; no counterpart in the reference) ----------------------------------------------
 * The ID pass: per pixel of a frame the closest hit of the ray through the pixel's centre, xy = (px + 0.5, py + 0.5), as three
 * planes of width * height words -- shape, triangle inside its model, material. Pixel (px, py) holds what srt_pick reports for
 * that point under the same options, bit for bit and under every acceleration mode; a miss is SRT_HIT_NONE, SRT_HIT_NONE, -1; a
 * shape without a material is reported. The pass is one kernel over the frame (csrc/selection.hip): no staging, 12 bytes written
 * per pixel. It touches neither canvas nor counters nor any denoiser, exposure, bloom or noise state. The material plane sees
 * srt_set_triangle_materials as of the pass.
 *
 * The overlay: with a selection set, every site that produces a picture's bytes -- srt_render, srt_render_async,
 * srt_render_pipelined, srt_resolve, srt_resolve_denoised, srt_resolve_gathered, srt_group_render, srt_group_resolve_denoised --
 * composites a tint over the selected shapes' visible pixels and an outline around them, as the last step on the bytes (behind
 * the denoiser, exposure and bloom). Unchanged: srt_resolve_external, srt_resolve_noise_view, srt_read_canvas, the denoiser's
 * history, and the interleaved rows of a partitioned handle (world > 1), which are no picture. Off (the default): not one launch
 * more, every byte and every srt_last_* answer as without the feature.
 *   m(p) = 1 when the ID pass's shape at p is in the set. R = ceil(width + 0.5) - 1 (1..8).
 *   d2(p) = the smallest dx^2 + dy^2 over the pixels q = p + (dx, dy), |dx|, |dy| <= R, q inside the frame, m(q) = 1 (integers).
 *   table[d2] = floor(clamp(width + 0.5 - sqrt((double)d2), 0, 1) * outline alpha + 0.5), d2 = 0 .. 2 R^2, made on the host in
 *   double from the float width (srt_selection_alpha_table_host); the device computes no square root.
 *   alpha(p) = fill alpha (colour: fill) where m(p) = 1; table[d2] (colour: outline) where m(p) = 0 and d2 exists; else 0.
 *   Per colour byte: out = (byte * (255 - a) + colour * a + 127) / 255 in integers; the picture's alpha byte stays; pixels with
 *   a == 0 are not written.
 * The overlay's camera is that of the handle's most recent dispatch (srt_trace, srt_render*); before any dispatch there is no
 * overlay. Its ID pass runs behind a resolve only when its key -- the scene's revision (every successful srt_update_scene), the
 * bytes of camera_to_world, aspect_ratio and fov_scale, width and height -- differs from the planes the handle holds: under an
 * unchanged camera and scene it costs nothing per frame. The key is compared on the host; nothing waits for the device.
 * Everything is enqueued on the handle's stream. A group keeps ONE state, on its first device, whose member holds the whole scene. */
int srt_selection_defaults(srt_selection_params *out); /* enabled 1, width 2, outline 255 / 255, 160, 0, fill 0 / 255, 160, 0 */
/* Host-only: the validation srt_set_selection applies. SRT_ERR_INVALID: a width outside [1, 8] or not finite, a non-zero
 * reserved field, enabled neither 0 nor 1. */
int srt_selection_check_host(const srt_selection_params *p);
/* Host-only: out = {sizeof(srt_selection_params)} as the library was built. */
int srt_selection_sizes(size_t out[1]);
/* Host-only: table[0 .. 2 R^2] as defined above into table (cap entries, >= 2 R^2 + 1; SRT_SELECTION_TABLE_MAX always fits),
 * *radius = R (may be NULL). SRT_ERR_INVALID as srt_selection_check_host, or cap too small. */
int srt_selection_alpha_table_host(const srt_selection_params *p, uint8_t *table, size_t cap, int *radius);
/* shapes: n indices into the array srt_update_scene was given; kept across scene updates, stored on the device as a bit table
 * sized to the current scene's shape count -- an index beyond the scene never matches. p NULL, p->enabled == 0 or n == 0: off.
 * Waits for the handle's stream. SRT_ERR_INVALID as srt_selection_check_host, or shapes NULL with n > 0. */
int srt_set_selection(srt_tracer *t, const srt_selection_params *p, const uint32_t *shapes, size_t n);
int srt_group_set_selection(srt_group *g, const srt_selection_params *p, const uint32_t *shapes, size_t n);
/* The ID pass alone, for the camera and frame size of `options` (any positive size), asynchronous on the handle's stream: the
 * AOV for callers who want no overlay. The planes it makes are the handle's: an overlay behind it reuses them when its key agrees. */
int srt_render_ids(srt_tracer *t, const srt_render_data *options);
/* Waits for the handle's stream. The planes of the last ID pass (srt_render_ids, or the overlay's), *w x *h words each, into the
 * pointers that are not NULL, of cap_pixels words each. All three NULL: the size alone. SRT_ERR_STATE: no ID pass yet;
 * SRT_ERR_INVALID: cap_pixels too small. */
int srt_read_id_pass(srt_tracer *t, uint32_t *shape, uint32_t *triangle, int32_t *material, size_t cap_pixels, int *w, int *h);
int srt_group_read_id_pass(srt_group *g, uint32_t *shape, uint32_t *triangle, int32_t *material, size_t cap_pixels, int *w, int *h);
/* Waits for the handle's stream. alpha(p) of the last overlaid frame, one byte per pixel of the frame. SRT_ERR_STATE: no overlaid
 * frame yet. */
int srt_read_selection_alpha(srt_tracer *t, uint8_t *alpha, size_t cap_pixels);
/* For tests: *applied = 1 when the last picture-producing resolve on the handle (the group: on its first device) ran the overlay,
 * *id_pass_ran = 1 when it had to make the ID planes first. Either may be NULL. */
int srt_last_resolve_selected(const srt_tracer *t, int *applied, int *id_pass_ran);
int srt_group_last_resolve_selected(const srt_group *g, int *applied, int *id_pass_ran);

/* ---- ambient-occlusion pass (new; no counterpart in the reference) ----------------------------------------------------------
 * Per pixel of a frame: how many of S cosine-weighted hemisphere rays from the visible surface meet anything within a radius.
 * A "clay" picture of the geometry with a bounded, fixed noise, for the viewport while the camera or a gizmo moves, and the one
 * AOV neither the denoiser's guides nor the ID pass cover. `options` supplies only the camera (camera_to_world, aspect_ratio,
 * fov_scale) and the frame size (width, height: any positive size, not necessarily the handle's); S = params->samples.
 *
 * THE DEFINITION, per pixel q = py * width + px. The library is built with fp-contract=off: every line below is a plain float
 * statement per component, nothing is fused.
 *   SURFACE. The ray is the ID pass's: xy = (px + 0.5, py + 0.5), unit direction `dir`, origin `org`, tmax = +inf, refused and
 *     walked exactly as srt_pick refuses and walks it. t = the pick's t, N = the pick's normal (the winner's, turned to face the
 *     ray). A shape without a material is a surface, as it is for the pick. A miss or an invalid ray: no surface.
 *   ORIGIN. P = org + dir * t;  O = P + N * bias.
 *   SAMPLE s of S:  uint32_t seed = params->seed + (q * S + s) * 0x9E3779B9u;  then the per-lane random unit vector of the
 *     trace's diffuse bounce, added to the normal:  rd = normalize3(random_normal3_lane(seed));  D = normalize3(N + rd).
 *     The ray is {O, tmax = radius, D}, its direction of unit length. That is the cosine law about N (a point of the unit
 *     sphere that touches the surface at P, seen from P): E[dot(D, N)] = 2/3. The trace's bounce first turns rd into N's
 *     hemisphere (rd * sign(dot(N, rd))); the pass does NOT: normalize3(N + a direction of the hemisphere) keeps every ray
 *     within 45 degrees of N (mean cosine 0.862) and is no cosine law. rd = -N, for which D would be 0, gives an invalid ray,
 *     which is not occluded.
 *   ANSWER. occluded[q] = the number of the pixel's S rays for which srt_occluded_rays(ray, SRT_RAYS_UNIT_DIRECTIONS) would set
 *     its bit -- the occlusion contract unchanged: tmax strict, glass and shapes without a material occlude, an invalid ray is
 *     not occluded. A pixel without a surface holds SRT_HIT_NONE.
 * The plane is width * height uint32_t; a caller who wants a float derives 1 - occluded / S. The integer is what can be pinned:
 * it does not depend on how the kernels map rays to lanes, nor on the acceleration mode.
 *
 * THE RAYS. srt_ao_rays returns the n_pixels * S rays defined above for pixels first_pixel .. of the frame, ray (q, s) at
 * (q - first_pixel) * S + s, made by the same device function the pass makes a ray with (blocking; through the queries' staging
 * allocation). A pixel without a surface gets S records with tmax = NaN (origin and direction 0): invalid rays by the cast's
 * rule. So the per-pixel sum of srt_occluded_rays(srt_ao_rays(...), SRT_RAYS_UNIT_DIRECTIONS) equals srt_read_ao's plane,
 * integer for integer.
 * THE VIEW. srt_resolve_ao_view writes the grey picture into the handle's ARGB bytes (srt_read_argb reads it), asynchronous:
 * A = 255, R = G = B = table[occluded], table[c] = floor(255 * (1 - c / S) + 0.5) made on the host in double
 * (srt_ao_table_host); a pixel without a surface gets the bytes A, R, G, B of params->background = 0xAARRGGBB. Like
 * srt_resolve_noise_view it is no picture site: selection overlay, exposure and bloom do not apply. The pass's frame must be
 * the handle's size, else SRT_ERR_STATE.
 * STATE. As a cast: the scene as the last srt_update_scene left it, ordered on the handle's stream behind that update's
 * pre-pass, refit and build. The pass writes planes of its own on the handle (36 B per pixel, freed in srt_destroy),
 * srt_ao_rays the queries' staging allocation (32 B per ray + 32 B per pixel), the view the ARGB bytes, and nothing else:
 * canvas, counters, ID planes, denoiser, exposure, bloom, noise and selection state stay as they were, and so does every
 * srt_last_* answer but srt_last_ray_query_ms, which covers the launches of the last of these calls when the kernel timers
 * are on. A handle that never calls these launches exactly what it launched before. Before any scene is set every pixel is
 * SRT_HIT_NONE.
 * ERRORS. SRT_ERR_INVALID: a NULL argument; what srt_ao_check_host refuses; first_pixel + n_pixels beyond the frame; a
 * capacity too small. SRT_ERR_STATE: srt_read_ao or srt_resolve_ao_view before any pass. n_pixels == 0: SRT_OK, no launch. */
int srt_ao_defaults(srt_ao_params *out); /* samples 16, radius +inf, bias 0.001f (the reference's acne offset), seed 0, background 0xff000000 */
/* Host-only: the validation srt_render_ao applies. SRT_ERR_INVALID unless samples is one of 1, 2, 4, 8, 16, 32, 64; radius > 0
 * and not NaN (+inf allowed); bias >= 0 and finite; reserved zero; width, height > 0 and width * height * samples < 2^31. */
int srt_ao_check_host(const srt_ao_params *p, int width, int height);
/* Host-only: out = {sizeof(srt_ao_params)} as the library was built. */
int srt_ao_sizes(size_t out[1]);
/* Host-only: table[c] for c = 0 .. samples as defined above (the entries past samples: 0). SRT_ERR_INVALID: samples refused. */
int srt_ao_table_host(const srt_ao_params *p, uint8_t table[65]);
/* The pass, asynchronous on the handle's stream. */
int srt_render_ao(srt_tracer *t, const srt_render_data *options, const srt_ao_params *params);
/* Waits for the handle's stream. The last pass's plane, *w x *h words, into `occluded` of cap_pixels words; *samples = its S.
 * `occluded` NULL: the sizes alone. Any of w, h, samples may be NULL. */
int srt_read_ao(srt_tracer *t, uint32_t *occluded, size_t cap_pixels, int *w, int *h, int *samples);
int srt_ao_rays(srt_tracer *t, const srt_render_data *options, const srt_ao_params *params, size_t first_pixel, size_t n_pixels, srt_ray *rays_out);
int srt_resolve_ao_view(srt_tracer *t);
/* On the group's first member, which holds the whole scene, as the group casts. srt_group_read_ao_view: blocking, the group's
 * width * height * 4 bytes of the view (a group has no srt_read_argb). */
int srt_group_render_ao(srt_group *g, const srt_render_data *options, const srt_ao_params *params);
int srt_group_read_ao(srt_group *g, uint32_t *occluded, size_t cap_pixels, int *w, int *h, int *samples);
int srt_group_ao_rays(srt_group *g, const srt_render_data *options, const srt_ao_params *params, size_t first_pixel, size_t n_pixels, srt_ray *rays_out);
int srt_group_resolve_ao_view(srt_group *g);
int srt_group_read_ao_view(srt_group *g, uint8_t *argb_out);

/* ---- area selection (new; no counterpart in the reference) ------------------------------------------------------------------
 * The rubber band of an editor: which shapes, or which faces of one mesh, are VISIBLE inside a rectangle or a lasso, and how
 * many pixels of each -- counted on the device from the ID pass's planes (above), which are already there. A few hundred
 * integers come back instead of 12 bytes per pixel. Records: srt_area, srt_area_summary (srt_types.h). Everything is an integer.
 *
 * THE AREA is the half-open pixel rectangle [x0, x1) x [y0, y1), optionally intersected with a lasso.
 *   - The rectangle is clipped to the ID planes' frame; it may lie partly or wholly outside; an empty one gives all zeros.
 *   - The lasso is a polygon of n_vertices in {0, 3..SRT_AREA_MAX_VERTICES}, 0 meaning the rectangle alone, closed implicitly,
 *     even-odd rule. Self-intersecting, clockwise, counter-clockwise and zero-area polygons are legal.
 *   - Vertices are int32 pairs {vx, vy} in pixel-CORNER coordinates: (vx, vy) is the corner shared by pixels (vx - 1 .. vx,
 *     vy - 1 .. vy). Each coordinate lies in [-2^20, 2^20].
 * Pixel (px, py) is inside the lasso by exact integer arithmetic on doubled coordinates. With C = (2 px + 1, 2 py + 1) and, for
 * edge i, A = 2 v[i], B = 2 v[(i + 1) % n]:
 *   - the edge SPANS THE ROW when (A.y < C.y) != (B.y < C.y). C.y is odd and A.y, B.y are even: equality cannot occur, so there
 *     is no vertex-on-row case;
 *   - cross = (B.x - A.x) * (C.y - A.y) - (B.y - A.y) * (C.x - A.x) in int64;
 *   - a spanning edge COUNTS when cross > 0 for B.y > A.y, or cross < 0 for B.y < A.y. A pixel centre exactly on an edge
 *     (cross == 0) does not count for that edge;
 *   - the pixel is inside when the number of counting edges is odd.
 * The mask M(p) is "rectangle and frame and (no lasso or inside)". One implementation, csrc/area_host.h, is compiled into the
 * counting kernel and into srt_area_mask_host.
 * SHAPE COVERAGE over the shape plane S, n_shapes = the scene's shape count:
 *   counts[s] = #{p : M(p), S(p) == s} for s < n_shapes;  area_pixels = #M;  miss_pixels = #{M, S == SRT_HIT_NONE};
 *   hit_pixels = area_pixels - miss_pixels (= sum(counts));  distinct = #{s : counts[s] > 0};  target_pixels = 0.
 * TRIANGLE COVERAGE of one model shape s0 over the triangle plane T, n_tri = the triangles of the shape's model:
 *   counts[k] = #{p : M(p), S(p) == s0, T(p) == k} for k < n_tri;  target_pixels = sum(counts);  distinct = #{k : counts[k] > 0};
 *   area_pixels, miss_pixels and hit_pixels as above. s0 not a model shape: SRT_ERR_INVALID.
 * THE KERNEL (csrc/area.hip) covers the clipped rectangle only, a wave per 64 pixels of one row; a wave adds the lanes that
 * share a key with one atomic, SRT_AREA_AGG_ROUNDS times, and what is left lane by lane. Every key is compared with the count
 * array's length before its atomic: whatever the planes hold, nothing is written outside `counts`.
 * THE PLANES. options != NULL: the handle's ID planes are brought up to date for that camera and frame first, under the overlay's
 * key -- an unchanged camera and scene run no ID pass, and an overlay behind the call reuses the planes. options == NULL: the
 * planes the handle holds; SRT_ERR_STATE when there are none, or when the scene's revision has moved on since they were made
 * (counts of a stale plane would index another scene).
 * STATE. A coverage call writes its own result buffers on the handle and nothing else: canvas, counters, denoiser, exposure,
 * bloom, noise and AO state stay as they were and, unless it is srt_select_area, so does the selection. A handle that never
 * calls any of this launches exactly what it launched before.
 * ERRORS. SRT_ERR_INVALID: a NULL handle, area, counts (with a capacity needed) or summary; what srt_area_check_host refuses; a
 * capacity below n_shapes / n_tri (nothing is launched); options with a frame that is not positive or has 2^31 pixels or more. */
/* Host-only: out = {sizeof(srt_area), sizeof(srt_area_summary)} as the library was built. */
int srt_area_sizes(size_t out[2]);
/* Host-only: the validation every call below applies. SRT_ERR_INVALID: n_vertices 1, 2 or above SRT_AREA_MAX_VERTICES; a
 * coordinate outside [-2^20, 2^20]; vertices NULL with n_vertices > 0; flags or a reserved field not 0; x1 < x0 or y1 < y0. */
int srt_area_check_host(const srt_area *area, const int32_t *vertices);
/* Host-only: M(p) of a w x h frame as defined above, one byte (0 or 1) per pixel into mask of cap bytes. SRT_ERR_INVALID as
 * srt_area_check_host; w or h not positive; w * h >= 2^31; mask NULL or cap < w * h. */
int srt_area_mask_host(const srt_area *area, const int32_t *vertices, int w, int h, uint8_t *mask, size_t cap);
/* Blocking. counts: cap_shapes >= n_shapes words, of which n_shapes are written (NULL allowed when n_shapes == 0). The counts and
 * the summary come back as one copy through pinned memory behind an event. */
int srt_area_coverage(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                      srt_area_summary *out);
int srt_area_triangle_coverage(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape, uint32_t *counts,
                               size_t cap_triangles, srt_area_summary *out);
/* Shape coverage left in device memory of the handle's device, asynchronous on the handle's stream: d_counts of n >= n_shapes
 * words (all n are zeroed, n_shapes counted), d_summary of 8 words laid out as srt_area_summary; both 4-byte aligned. */
int srt_area_coverage_device(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *d_counts, size_t n,
                             uint32_t *d_summary);
/* Blocking. Shape coverage, then the shapes with counts[s] >= max(min_pixels, 1) combined with the handle's current selection
 * (srt_read_selection) by mode -- SRT_SELECT_REPLACE: they alone; ADD: the union; SUBTRACT: the current ones that are not
 * among them; TOGGLE: those in exactly one of the two -- and set as srt_set_selection sets a list, with the parameters last given
 * to it (never given: srt_selection_defaults) and the overlay enabled. An empty result switches the overlay off, as
 * srt_set_selection does for n == 0. *n_selected (may be NULL) = the length of the new list. SRT_ERR_INVALID: an unknown mode. */
int srt_select_area(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                    size_t *n_selected);
/* The current selection: the list the overlay shows (srt_set_selection's, or srt_select_area's), ascending and unique, *n of
 * them; empty while the overlay is off. shapes NULL: the length alone. SRT_ERR_INVALID: cap < *n. Host state only. */
int srt_read_selection(srt_tracer *t, uint32_t *shapes, size_t cap, size_t *n);
/* On the group's first device, which holds the group's one ID / selection state and the whole scene. */
int srt_group_area_coverage(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                            srt_area_summary *out);
int srt_group_area_triangle_coverage(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                     uint32_t *counts, size_t cap_triangles, srt_area_summary *out);
int srt_group_select_area(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                          size_t *n_selected);
int srt_group_read_selection(srt_group *g, uint32_t *shapes, size_t cap, size_t *n);
/* With srt_set_kernel_timers on: the device time of the last coverage call's clear and counting launches (its ID pass excluded),
 * in milliseconds; 0 when the timers were off or nothing was launched. Blocking, as srt_last_ray_query_ms. */
int srt_last_area_ms(srt_tracer *t, float *ms);
/* For tests: *id_pass_ran = 1 when the last coverage call on the handle had to make the ID planes first. */
int srt_last_area_id_pass(const srt_tracer *t, int *id_pass_ran);

/* ---- multi-hit ray queries (new): the first K hits along caller rays -------------------------------------------------------- */

/* For each of n rays, the first k surfaces along it in order, not only the closest: click-through selection (the object under
 * the one already selected, the shape seen through the glass sphere, the list for an "objects under the cursor" pop-up),
 * dropping a dragged object along a ray while ignoring itself (the first record whose shape is not the dragged one), entry and
 * exit distances of a body, and the number of surface crossings, whose parity says whether the origin is inside a closed mesh.
 * Repeated casts cannot give this: a cast has no lower limit and no exclusion, and restarting the ray "a bit past" the last hit
 * changes the ray's bits and loses coincident surfaces. Records: srt_ray, srt_ray_hit (srt_types.h), k of the latter per ray,
 * k in 1 .. SRT_MULTI_HIT_MAX (8).
 *
 * THE ANSWER IS A SET OVER PRIMITIVES, ORDERED, so it does not depend on how the scene is traversed: the array scan, the host's
 * SAH hierarchy, the device-built hierarchies and a refitted hierarchy give the same bytes.
 * THE RAY is the cast's ("ray queries" above): the same validity rule, decided on the device; the same normalisation unless
 * SRT_RAYS_UNIT_DIRECTIONS is given; tmax strict, and tmax <= 0 (-0 and -inf included) gives no hits.
 * THE CANDIDATES of a ray are the primitives whose own intersector accepts the ray and for whose t the comparison t < tmax is
 * true (so a NaN t is no candidate):
 *   - every sphere, by intersect_sphere (render.cl:180-204): ONE hit per sphere, the nearer root when it is not negative, else
 *     the farther one -- the exit when the origin is inside;
 *   - every plane, by intersect_plane (render.cl:206-221);
 *   - every triangle, by intersect_triangle (render.cl:243-275) on the world triangle, of every model whose bounding box passes
 *     intersection_aabb(bounds, origin, 1 / direction, tmax) (render.cl:279-290) with the CALLER'S tmax as the limit.
 *     The cast tests a model's box against its SHRINKING closest distance instead; that is a different statement. The two can
 *     differ only when a box's entry distance rounds past a hit that lies on the box's surface: the cast then skips the model,
 *     this query, whose limit for the box does not depend on what was found before, keeps the hit. With k = 1 record 0 is
 *     otherwise the cast's record.
 * THE ORDER. Candidates are ordered by t compared as floats; equal t (-0 == +0) goes to the lower shape index; inside a model
 * equal t goes to the lower triangle index inside the model. Two triangles that share an edge the ray passes through are two
 * candidates and two records.
 * THE RECORDS. hits[q * k + j] is candidate j of ray q in that order, for j < min(k, #candidates), with the cast's fields: t as
 * the intersector computed it, the winner_normal of the primitive at origin + direction * t turned to face the ray,
 * SRT_HIT_HIT, SRT_HIT_FRONT by the cast's rule, the triangle index inside its model, the per-triangle material rule, and a
 * shape WITHOUT a material reported with material = -1. The remaining slots hold the cast's miss record. An invalid ray has
 * the miss record with SRT_HIT_INVALID_RAY in all k slots and count 0.
 * COUNTS. counts[q] (counts may be NULL: not written) is the number of records written, min(k, #candidates). With
 * SRT_RAYS_COUNT_ALL it is #candidates, which may exceed k; the records are the same bytes either way. (The flag keeps the
 * walk's limit at tmax: every candidate has to be met to be counted.)
 * STATE, HOSTILE RAYS. As a cast: the scene as the last srt_update_scene left it, ordered on the handle's stream; nothing is
 * written but the outputs and the queries' shared staging allocation; before any scene is set every valid ray has no hits.
 * srt_last_ray_query_ms covers the launches.
 * COUNTS AND ERRORS. n == 0: SRT_OK, no launch. k outside 1 .. SRT_MULTI_HIT_MAX, flag bits other than
 * SRT_RAYS_UNIT_DIRECTIONS | SRT_RAYS_COUNT_ALL, a null rays or hits pointer with n > 0, n >= 2^31, device rays or hits not
 * aligned to 16 bytes, device counts not aligned to 4: SRT_ERR_INVALID. The host forms use the handle's one staging allocation
 * (per ray 32 B of rays, 32 k B of records, 4 B of counts -- that region rounded up to 8 bytes -- and the 8 B of a picked point,
 * reserved by both forms though only srt_pick_through writes them: 44 B + 32 k B), grown as needed; what the other calls get of
 * it does not change.
 *
 * srt_cast_rays_multi: host arrays, blocking. srt_cast_rays_multi_device: n srt_ray, n * k srt_ray_hit and n words in device
 * memory of the handle's device, asynchronous on the handle's stream. srt_pick_through: srt_pick's rays (the same small kernel,
 * the same `options` and xy), then this query with unit directions and tmax = +inf; blocking. */
int srt_cast_rays_multi(srt_tracer *t, const srt_ray *rays, size_t n, uint32_t k, uint32_t flags, srt_ray_hit *hits /* n * k */,
                        uint32_t *counts /* n, may be NULL */);
int srt_cast_rays_multi_device(srt_tracer *t, const void *rays_dev, size_t n, uint32_t k, uint32_t flags, void *hits_dev, void *counts_dev /* may be NULL */);
int srt_pick_through(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, uint32_t k, srt_ray_hit *hits, uint32_t *counts /* may be NULL */);
/* On the group's first member, as srt_group_cast_rays. */
int srt_group_cast_rays_multi(srt_group *g, const srt_ray *rays, size_t n, uint32_t k, uint32_t flags, srt_ray_hit *hits, uint32_t *counts);
int srt_group_pick_through(srt_group *g, const srt_render_data *options, const float *xy, size_t n, uint32_t k, srt_ray_hit *hits, uint32_t *counts);
/* Host-only: the argument check every call above applies to k and flags. */
int srt_multi_hit_check_host(uint32_t k, uint32_t flags);
/* Host-only: out = {sizeof(srt_ray), sizeof(srt_ray_hit), SRT_MULTI_HIT_MAX} as the library was built. */
int srt_multi_hit_sizes(size_t out[3]);

/* ---- area selection, through (new): coverage of shapes hidden behind others -------------------------------------------------
 * The selection mode modellers call X-ray or "select through": every shape, or every face of one mesh, that lies inside the
 * marquee or lasso, the ones BEHIND other shapes included -- back faces, objects inside a glass sphere, a mesh behind a wall.
 * "area selection" above counts what is visible, from the ID planes; this counts over each pixel ray's whole candidate set, so
 * there are no ID planes and no key. Records as above. Everything is an integer.
 *
 * THE AREA M(p) is the one "area selection" defines: the same srt_area (flags still 0), the same srt_area_check_host, the same
 * integer lasso (csrc/area_host.h, compiled into these kernels too).
 * THE FRAME comes from `options`, which is REQUIRED (NULL: SRT_ERR_INVALID): the rectangle is clipped against options->width x
 * options->height, which must be positive and below 2^31 pixels.
 * THE RAY OF p is the ID pass's: the image point (px + 0.5, py + 0.5) through srt_pick's ray set-up (device_math.h camera_ray),
 * refused by the cast's validity rule on the device, unit direction, tmax = +inf. srt_pick_rays returns exactly these rays.
 * CANDIDATES. cand(p) is the candidate set of that ray exactly as "multi-hit ray queries" defines it: each primitive's own
 * intersector with t < tmax true, a model's triangles only when intersection_aabb passes with the caller's tmax (+inf here). A
 * refused ray has no candidates.
 * SHAPE COVERAGE, THROUGH, n_shapes = the scene's shape count:
 *   counts[s] = #{p : M(p), some candidate of p belongs to shape s} -- a pixel counts a shape ONCE however many of its triangles
 *   the ray crosses;  area_pixels = #M;  miss_pixels = #{M, cand(p) empty};  hit_pixels = area_pixels - miss_pixels (NOT
 *   sum(counts): a pixel may count several shapes);  distinct = #{s : counts[s] > 0};  target_pixels = 0.
 * TRIANGLE COVERAGE, THROUGH, of one model shape s0, n_tri = the triangles of the shape's model:
 *   counts[k] = #{p : M(p), triangle k of s0 is a candidate of p} -- back-facing and hidden faces included; only s0 is walked;
 *   miss_pixels = #{M, s0 has no candidate on p};  hit_pixels = target_pixels = area_pixels - miss_pixels, which counts PIXELS,
 *   not sum(counts), which may be larger;  distinct = #{k : counts[k] > 0}. s0 not a model shape: SRT_ERR_INVALID.
 * ACCELERATION MODES. Both coverages are sets over primitives: the array scan, the host's SAH hierarchy, the device-built
 * Morton and median hierarchies and refitted hierarchies give the same integers.
 * INFINITE PLANES. A plane the frame faces is a candidate of most pixels, visible or not -- the floor under everything, the wall
 * behind everything. Front-ends that select through filter such planes with min_pixels or by the shape's type.
 * THE KERNELS (csrc/area_through.hip) use the area kernel's mapping (the clipped rectangle only, a wave per 64 pixels of one
 * row). Per shape and wave ONE atomic adds the popcount of a ballot; a model is asked for existence only (the any-hit walk). In
 * triangle mode every accepted triangle is one atomic on its index. Every index is compared with the count array's length
 * before its atomic.
 * STATE. As a cast: the scene as the last srt_update_scene left it, ordered on the handle's stream. The calls write their own
 * result buffers (shared with "area selection") and nothing else: ID planes, selection (except srt_select_area_through), canvas,
 * counters, denoiser, exposure, bloom, noise and AO state stay untouched. A handle that never calls these launches what it
 * launched before. Before any scene is set every pixel is a miss. srt_last_area_ms covers these launches;
 * srt_last_area_id_pass answers 0 after them.
 * ERRORS. As "area selection", and options == NULL. flags = 1 in the srt_area stays refused. */
int srt_area_coverage_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts, size_t cap_shapes,
                              srt_area_summary *out);
int srt_area_triangle_coverage_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                       uint32_t *counts, size_t cap_triangles, srt_area_summary *out);
/* As srt_area_coverage_device: all n >= n_shapes words of d_counts are zeroed, n_shapes counted; asynchronous. */
int srt_area_coverage_through_device(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *d_counts, size_t n,
                                     uint32_t *d_summary);
/* Blocking. srt_select_area's four modes and rules applied to the through counts. Mind the infinite planes (above). */
int srt_select_area_through(srt_tracer *t, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                            size_t *n_selected);
/* On the group's first member, as srt_group_area_coverage. */
int srt_group_area_coverage_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t *counts,
                                    size_t cap_shapes, srt_area_summary *out);
int srt_group_area_triangle_coverage_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, uint32_t shape,
                                             uint32_t *counts, size_t cap_triangles, srt_area_summary *out);
int srt_group_select_area_through(srt_group *g, const srt_render_data *options, const srt_area *area, const int32_t *vertices, int mode, uint32_t min_pixels,
                                  size_t *n_selected);
/* The rays srt_pick would cast for n image points xy (its small kernel, the same `options`): n srt_ray with unit directions and
 * tmax = +inf into rays_out; cast them with SRT_RAYS_UNIT_DIRECTIONS. Blocking; counts, errors and staging as srt_pick. */
int srt_pick_rays(srt_tracer *t, const srt_render_data *options, const float *xy, size_t n, srt_ray *rays_out);
int srt_group_pick_rays(srt_group *g, const srt_render_data *options, const float *xy, size_t n, srt_ray *rays_out);

/* Library / build identification, e.g. "srt-hip gfx950 parity fp-contract=off". */
const char *srt_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SRT_ABI_H */
