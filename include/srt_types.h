/* srt_types.h — plain-C scene/record layouts crossing the C ABI.
 *
 * These are byte-for-byte the device structs of the reference kernel
 * (/root/reference/src/render.cl:5-105) and of their host mirrors
 * (/root/reference/include/material.hpp:10-38, include/shape.hpp:15-111,
 * include/tracer.hpp:48-80). OpenCL float3 occupies 16 bytes, so every
 * 3-vector below carries one pad float. No glm, boost or OpenCL headers needed.
 */
#ifndef SRT_TYPES_H
#define SRT_TYPES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srt_float3 {
	float x, y, z, _pad;
} srt_float3; /* cl_float3 */

typedef struct srt_float4 {
	float x, y, z, w;
} srt_float4; /* cl_float4 */

/* render.cl:17-27 / material.hpp:10-21 */
typedef struct srt_material {
	float smoothness;
	float metallic;
	float specular;
	float emission_strength;
	float transmittance;
	float refraction_index;
	float _pad[2];
	srt_float3 color;
	srt_float3 emission;
} srt_material;

/* render.cl:29-32 / shape.hpp:15-20 */
typedef struct srt_sphere {
	srt_float3 position;
	float radius;
	float _pad[3];
} srt_sphere;

/* render.cl:34-37 / shape.hpp:22-27 */
typedef struct srt_plane {
	srt_float3 position;
	srt_float3 normal;
} srt_plane;

/* render.cl:39-42 / shape.hpp:30-33 — note: normal FIRST, then position */
typedef struct srt_vertex {
	srt_float3 normal;
	srt_float3 pos;
} srt_vertex;

/* render.cl:44-53 / shape.hpp:29-44 */
typedef struct srt_triangle {
	srt_vertex vertices[3];
} srt_triangle;

/* render.cl:55-61 / shape.hpp:47-68; transform = 4 COLUMNS (glm::mat4) */
typedef struct srt_model {
	uint32_t triangle_index;
	uint32_t num_triangles;
	uint32_t _pad[2];
	srt_float3 bounding_min;
	srt_float3 bounding_max;
	srt_float4 transform[4];
} srt_model;

/* render.cl:63-67 / shape.hpp:78-82 */
enum { SRT_SHAPE_SPHERE = 0, SRT_SHAPE_PLANE = 1, SRT_SHAPE_MODEL = 2 };

/* render.cl:69-77 / shape.hpp:84-111 */
typedef struct srt_shape {
	int32_t type;
	int32_t material;
	int32_t _pad[2];
	union {
		srt_sphere sphere;
		srt_plane plane;
		srt_model model;
	} shape;
} srt_shape;

/* One node of the binary hierarchy the host builds over a model's triangles (srt_set_acceleration
 * in srt_abi.h; new, no counterpart in the reference) and srt_bvh_build_host hands out. Nodes of a
 * model are stored in depth-first order: an inner node's first child is node + 1, its second child
 * that child's `skip`. The device walks a four-wide folding of it (srt_bvh_wide_host). */
typedef struct srt_bvh_node {
	float lo[3];
	uint32_t skip; /* first node after this node's subtree, or SRT_BVH_END */
	float hi[3];
	uint32_t leaf; /* 0: inner node; else (count << 28) | first triangle record */
} srt_bvh_node;
#define SRT_BVH_END 0xffffffffu

/* render.cl:79-92 / tracer.hpp:48-67 */
typedef struct srt_render_data {
	int32_t width, height;
	int32_t num_samples;
	int32_t num_bounces;
	float aspect_ratio;
	float fov_scale;
	uint8_t show_normals;
	uint8_t _pad0[7];
	srt_float4 camera_to_world[4]; /* columns; column 3 = camera position */
	uint32_t time;
	uint32_t tick; /* never read by the kernel */
	uint32_t _pad1[2];
} srt_render_data;

/* render.cl:94-105 / tracer.hpp:69-80 */
typedef struct srt_scene_data {
	int32_t num_shapes;
	float sun_focus;
	float sun_intensity;
	float _pad0;
	srt_float3 horizon_color; /* unused by the kernel (render.cl:381-389) */
	srt_float3 zenith_color;  /* unused */
	srt_float3 ground_color;  /* unused */
	srt_float3 sun_color;
	srt_float3 sun_direction;
} srt_scene_data;

/* Edge-aware denoiser settings (srt_set_denoise in srt_abi.h; new, no counterpart in the reference).
 * A spatial, variance-guided a-trous filter (SVGF without its temporal part) over the canvas,
 * guided by primary-hit normals, distances and albedos. */
typedef struct srt_denoise_params {
	int32_t enable;          /* 0: off (the library launches what it launches without a denoiser) */
	int32_t iterations;      /* a-trous passes K, 0..8 (steps 1, 2, 4, ...); 0 = the plain resolve */
	int32_t feature_samples; /* camera rays per pixel and dispatch that feed the guide buffers, 1..64 */
	float sigma_luminance;   /* > 0 */
	float sigma_normal;      /* > 0: exponent of the normal weight */
	float sigma_depth;       /* > 0 */
	float sigma_albedo;      /* > 0 */
	int32_t reserved;        /* must be 0 */
} srt_denoise_params;

/* Temporal reprojection of the denoiser (srt_set_denoise_temporal in srt_abi.h; new, no counterpart in the
 * reference). The integrated colour and moments of the frame before the last srt_clear_canvas are reprojected
 * through the two cameras and blended into the current frame's, weighted by sample counts. */
typedef struct srt_temporal_params {
	int32_t enable;         /* 0: off */
	int32_t history_limit;  /* 1..2^20: the most samples a pixel's history counts for */
	float normal_threshold; /* -1..1: a history tap needs N . N_history >= this */
	float depth_threshold;  /* finite, > 0: and |Z_history - D| <= this * D, D = distance from the history camera */
	int32_t reserved[4];    /* must be 0 */
} srt_temporal_params;

/* Exposure for the resolve (srt_set_exposure in srt_abi.h; new, no counterpart in the reference): the divided colour is
 * multiplied by an exposure before the tone map, a fixed one (MANUAL) or one metered from the frame's luminance histogram
 * on the device (AUTO). */
enum { SRT_EXPOSURE_MANUAL = 0, SRT_EXPOSURE_AUTO = 1 };
typedef struct srt_exposure_params {
	int32_t enable;        /* 0: off (the library launches what it launches without the feature) */
	int32_t mode;          /* SRT_EXPOSURE_MANUAL / SRT_EXPOSURE_AUTO */
	float ev;              /* finite, |ev| <= 32. MANUAL: exposure = 2^ev. AUTO: a bias added to the metered log2 exposure */
	float key;             /* finite, > 0: the luminance the metered average is mapped to (default 0.18) */
	int32_t low_permille;  /* 0..999: histogram mass ignored at the dark end (default 100) */
	int32_t high_permille; /* low_permille + 1..1000: ... and kept up to here (default 950) */
	float adapt;           /* 0 < adapt <= 1: share of the way from the previous exposure to the target per metered frame, in log2 (default 1: immediate) */
	float min_ev, max_ev;  /* finite, min_ev <= max_ev, |.| <= 32: clamp of the metered log2 exposure before the bias (defaults -16, 16) */
	int32_t reserved[3];   /* must be 0 */
} srt_exposure_params;

/* Bloom for the resolve (srt_set_bloom in srt_abi.h, where the arithmetic is written down; new, no counterpart in the
 * reference): the part of the exposed colour above a threshold is blurred over an image pyramid and added before the tone map. */
#define SRT_BLOOM_MAX_LEVELS 8
typedef struct srt_bloom_params {
	int32_t enable;   /* 0: off (the library launches what it launches without the feature) */
	float threshold;  /* finite, >= 0: luminance of the exposed colour above which a pixel glows (default 1) */
	float knee;       /* finite, 0 <= knee <= threshold: half width of the soft onset around the threshold; 0: a hard one (default 0.5) */
	float intensity;  /* finite, 0 <= intensity <= 16: weight of the glow in the composite (default 0.1) */
	float scatter;    /* finite, 0 <= scatter <= 1: weight of a coarser level when it is added to the next finer one (default 0.7) */
	float clamp;      /* finite; 0: none; > 0: the largest luminance a pixel may contribute, the firefly limit (default 64) */
	int32_t levels;   /* 1..SRT_BLOOM_MAX_LEVELS pyramid levels; cut off after the first that is 1 x 1 (default 6) */
	int32_t reserved; /* must be 0 */
} srt_bloom_params;

/* Noise metering (srt_set_noise_meter in srt_abi.h, where the arithmetic is written down; new, no counterpart in the
 * reference): a per-pixel relative standard error of the mean from the denoiser's moments, its histogram, and a stopping rule. */
typedef struct srt_noise_params {
	int32_t enable;         /* 0: off (the library launches what it launches without the feature) */
	float threshold;        /* finite, 2^-24 <= threshold <= 2^8: a pixel with r <= threshold counts as converged (default 0.05) */
	float luminance_floor;  /* finite, 2^-20 <= floor <= 2^20: the error is relative to max(L, floor) (default 0.01) */
	int32_t permille;       /* 1..1000: the share of the metered pixels that has to be below the threshold, and the percentile the level is taken at (default 950) */
	uint32_t min_samples;   /* >= 1: no frame with fewer samples per pixel is converged (default 16) */
	int32_t check_every;    /* 1..65536: the resolving calls and srt_render_until meter when the dispatch count is a multiple of this (default 4) */
	int32_t reserved[2];    /* must be 0 */
} srt_noise_params;

/* One metering as srt_poll_noise / srt_read_noise / srt_render_until report it */
typedef struct srt_noise_result {
	uint32_t metered;    /* pixels in the histogram */
	uint32_t left_out;   /* pixels with a non-finite L, m2 or r */
	uint32_t below;      /* metered pixels with r <= threshold */
	int32_t converged;   /* the stopping rule (srt_abi.h) */
	uint32_t dispatches; /* T at the metering */
	uint32_t samples;    /* P at the metering */
	int32_t level_bin;   /* the bin the permille percentile falls in; -1: nothing metered */
	float level;         /* that bin's upper edge; 0: nothing metered */
} srt_noise_result;

/* Albedo textures (srt_set_textures, srt_set_material_textures; include/srt_abi.h). */
#define SRT_MAX_TEXTURES 64
enum { SRT_FILTER_LINEAR = 0, SRT_FILTER_NEAREST = 1 };
typedef struct srt_texture_desc {
	const float *rgba; /* width * height * 4 floats, row 0 = bottom (as the skybox) */
	int32_t width, height;
} srt_texture_desc;
typedef struct srt_material_texture {
	int32_t texture; /* index into the images of srt_set_textures; -1: the material keeps its colour */
	int32_t filter;  /* SRT_FILTER_* */
	float scale_u, scale_v; /* finite; u *= scale_u, v *= scale_v before the sampler */
} srt_material_texture;

/* Ray queries (srt_cast_rays, srt_pick; include/srt_abi.h "ray queries"). Both records are 32 bytes, read and written by the
 * device as two 128-bit words each. */
typedef struct srt_ray {
	float origin[3];
	float tmax; /* hits must be closer than this, strictly; +inf allowed */
	float direction[3];
	uint32_t reserved; /* not read */
} srt_ray;
typedef struct srt_ray_hit {
	float t;           /* world distance along the unit direction; +inf: a miss */
	uint32_t shape;    /* index into srt_update_scene's shapes; SRT_HIT_NONE: a miss */
	uint32_t triangle; /* index inside its model; SRT_HIT_NONE: a sphere, a plane, a miss */
	int32_t material;  /* the material the trace would shade with; -1: a miss, or a shape without one */
	float normal[3];   /* unit, facing the ray; 0 for a miss */
	uint32_t flags;    /* SRT_HIT_* */
} srt_ray_hit;
#define SRT_HIT_NONE 0xffffffffu
#define SRT_RAYS_UNIT_DIRECTIONS 1u /* per call: directions are used as given (already unit length) */
#define SRT_HIT_HIT 1u
#define SRT_HIT_FRONT 2u
#define SRT_HIT_INVALID_RAY 4u
/* Multi-hit ray queries (srt_cast_rays_multi, srt_pick_through; include/srt_abi.h "multi-hit ray queries"): the same two
 * records, k srt_ray_hit per ray. */
#define SRT_MULTI_HIT_MAX 8u  /* the largest k */
#define SRT_RAYS_COUNT_ALL 2u /* per call, multi-hit only: counts[q] is the size of the whole candidate set, not min(k, that) */

/* Occlusion queries (srt_occluded_segments, srt_segment_rays; include/srt_abi.h "occlusion queries"): is anything between
 * `from` and the point end_gap short of `to`. 32 bytes, read by the device as two 128-bit words. */
typedef struct srt_segment {
	float from[3];
	float end_gap; /* >= 0, finite: the stretch in front of `to` that does not count (0: up to `to` itself, exclusive) */
	float to[3];
	float reserved; /* must be 0 */
} srt_segment;

/* Selection overlay (srt_set_selection in srt_abi.h, where the arithmetic is written down; new, no counterpart in the
 * reference): the selected shapes' visible pixels are tinted and outlined over the resolved bytes. Colours are 8-bit A, R, G, B,
 * the order of the picture's bytes. */
#define SRT_SELECTION_MAX_WIDTH 8
#define SRT_SELECTION_TABLE_MAX 129 /* entries of the alpha table at the largest radius: d2 = 0 .. 2 * 8 * 8 */
typedef struct srt_selection_params {
	int32_t enabled;         /* 0: off (the library launches what it launches without the feature); 1: on; anything else is refused */
	float outline_width;     /* finite, 1 <= width <= SRT_SELECTION_MAX_WIDTH: pixels (default 2) */
	uint8_t outline_argb[4]; /* A: the outline's opacity; R, G, B: its colour (default 255, 255, 160, 0) */
	uint8_t fill_argb[4];    /* A: the tint's strength over the selected pixels, 0: no fill; R, G, B: its colour (default 0, 255, 160, 0) */
	int32_t reserved[4];     /* must be 0 */
} srt_selection_params;

/* Ambient-occlusion pass (srt_render_ao in srt_abi.h, where the rays are written down; new, no counterpart in the reference):
 * per pixel, how many of `samples` cosine-weighted hemisphere rays from the visible surface meet anything within `radius`. */
#define SRT_AO_MAX_SAMPLES 64
typedef struct srt_ao_params {
	uint32_t samples;     /* rays per pixel: 1, 2, 4, 8, 16, 32 or 64 (default 16) */
	float radius;         /* > 0, +inf allowed: a ray's tmax, strict (default +inf) */
	float bias;           /* >= 0, finite: the origin's offset along the facing normal (default 0.001f) */
	uint32_t seed;        /* the rays' generator starts from seed + (pixel * samples + sample) * 0x9E3779B9 (default 0) */
	uint32_t background;  /* srt_resolve_ao_view: 0xAARRGGBB of the pixels without a surface (default 0xff000000) */
	uint32_t reserved[3]; /* must be 0 */
} srt_ao_params;

/* Nearest-surface queries (srt_nearest_points; include/srt_abi.h "nearest-surface queries"). The query is 16 bytes, one 128-bit
 * load on the device; the answer 32 bytes, two 128-bit stores. */
typedef struct srt_point_query {
	float point[3];
	float max_distance; /* the surface must be closer than this, strictly; +inf allowed */
} srt_point_query;
typedef struct srt_nearest {
	float distance;    /* +inf: nothing within max_distance */
	uint32_t shape;    /* index into srt_update_scene's shapes; SRT_HIT_NONE: nothing */
	uint32_t triangle; /* index inside its model; SRT_HIT_NONE: a sphere, a plane, nothing */
	int32_t material;  /* the cast's rule; -1: nothing, or a shape without one */
	float point[3];    /* the closest point on the surface; 0 for nothing */
	uint32_t flags;    /* SRT_NEAREST_* | feature << SRT_NEAREST_FEATURE_SHIFT */
} srt_nearest;
#define SRT_NEAREST_FOUND 1u
#define SRT_NEAREST_BACK 2u    /* the query point is behind the surface: inside a sphere, under a plane, behind a triangle's cross(e1, e2) */
#define SRT_NEAREST_INVALID 4u /* a non-finite point component or a NaN max_distance: not traversed */
#define SRT_NEAREST_FEATURE_SHIFT 8 /* bits 8..10: 0 the face, 1/2/3 vertex v0/v1/v2, 4/5/6 edge v0v1 / v0v2 / v1v2; spheres and planes 0 */
#define SRT_NEAREST_FEATURE_MASK 0x700u

/* Area selection (srt_area_coverage, srt_select_area; include/srt_abi.h "area selection"). */
typedef struct srt_area {
	int32_t x0, y0, x1, y1; /* the half-open pixel rectangle [x0, x1) x [y0, y1); x0 <= x1, y0 <= y1; clipped to the frame */
	uint32_t n_vertices;    /* 0: the rectangle alone; else 3..SRT_AREA_MAX_VERTICES lasso vertices */
	uint32_t flags;         /* must be 0 */
	uint32_t reserved[2];   /* must be 0 */
} srt_area;
typedef struct srt_area_summary {
	uint32_t area_pixels;   /* #M */
	uint32_t hit_pixels;    /* area_pixels - miss_pixels */
	uint32_t miss_pixels;   /* #{M, shape == SRT_HIT_NONE} */
	uint32_t distinct;      /* #{k : counts[k] > 0} */
	uint32_t target_pixels; /* triangle coverage: sum(counts); shape coverage: 0 */
	uint32_t reserved[3];   /* written as 0 */
} srt_area_summary;
#define SRT_AREA_MAX_VERTICES 256u
#define SRT_AREA_AGG_ROUNDS 4u /* the counting kernel's wave-aggregated rounds before its per-lane atomics */
#define SRT_SELECT_REPLACE 0
#define SRT_SELECT_ADD 1
#define SRT_SELECT_SUBTRACT 2
#define SRT_SELECT_TOGGLE 3

#ifdef __cplusplus
}
#endif

#if defined(__cplusplus)
#define SRT_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define SRT_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif

SRT_STATIC_ASSERT(sizeof(srt_float3) == 16, "float3 is 16 B");
SRT_STATIC_ASSERT(sizeof(srt_material) == 64, "Material 64 B");
SRT_STATIC_ASSERT(offsetof(srt_material, transmittance) == 16, "Material.transmittance@16");
SRT_STATIC_ASSERT(offsetof(srt_material, refraction_index) == 20, "Material.refraction_index@20");
SRT_STATIC_ASSERT(offsetof(srt_material, color) == 32, "Material.color@32");
SRT_STATIC_ASSERT(offsetof(srt_material, emission) == 48, "Material.emission@48");
SRT_STATIC_ASSERT(sizeof(srt_sphere) == 32, "Sphere 32 B");
SRT_STATIC_ASSERT(offsetof(srt_sphere, radius) == 16, "Sphere.radius@16");
SRT_STATIC_ASSERT(sizeof(srt_plane) == 32, "Plane 32 B");
SRT_STATIC_ASSERT(offsetof(srt_plane, normal) == 16, "Plane.normal@16");
SRT_STATIC_ASSERT(sizeof(srt_vertex) == 32, "Vertex 32 B");
SRT_STATIC_ASSERT(offsetof(srt_vertex, pos) == 16, "Vertex.pos@16");
SRT_STATIC_ASSERT(sizeof(srt_triangle) == 96, "Triangle 96 B");
SRT_STATIC_ASSERT(sizeof(srt_model) == 112, "Model 112 B");
SRT_STATIC_ASSERT(offsetof(srt_model, num_triangles) == 4, "Model.num_triangles@4");
SRT_STATIC_ASSERT(offsetof(srt_model, bounding_min) == 16, "Model.bounding_min@16");
SRT_STATIC_ASSERT(offsetof(srt_model, bounding_max) == 32, "Model.bounding_max@32");
SRT_STATIC_ASSERT(offsetof(srt_model, transform) == 48, "Model.transform@48");
SRT_STATIC_ASSERT(sizeof(srt_shape) == 128, "Shape 128 B");
SRT_STATIC_ASSERT(offsetof(srt_shape, material) == 4, "Shape.material@4");
SRT_STATIC_ASSERT(offsetof(srt_shape, shape) == 16, "Shape.union@16");
SRT_STATIC_ASSERT(sizeof(srt_bvh_node) == 32, "BVH node 32 B");
SRT_STATIC_ASSERT(sizeof(srt_render_data) == 112, "RenderData 112 B");
SRT_STATIC_ASSERT(offsetof(srt_render_data, aspect_ratio) == 16, "RenderData.aspect_ratio@16");
SRT_STATIC_ASSERT(offsetof(srt_render_data, show_normals) == 24, "RenderData.show_normals@24");
SRT_STATIC_ASSERT(offsetof(srt_render_data, camera_to_world) == 32, "RenderData.camera_to_world@32");
SRT_STATIC_ASSERT(offsetof(srt_render_data, time) == 96, "RenderData.time@96");
SRT_STATIC_ASSERT(offsetof(srt_render_data, tick) == 100, "RenderData.tick@100");
SRT_STATIC_ASSERT(sizeof(srt_scene_data) == 96, "SceneData 96 B");
SRT_STATIC_ASSERT(offsetof(srt_scene_data, sun_focus) == 4, "SceneData.sun_focus@4");
SRT_STATIC_ASSERT(offsetof(srt_scene_data, horizon_color) == 16, "SceneData.horizon@16");
SRT_STATIC_ASSERT(offsetof(srt_scene_data, sun_color) == 64, "SceneData.sun_color@64");
SRT_STATIC_ASSERT(offsetof(srt_scene_data, sun_direction) == 80, "SceneData.sun_direction@80");
SRT_STATIC_ASSERT(sizeof(srt_denoise_params) == 32, "DenoiseParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_denoise_params, feature_samples) == 8, "DenoiseParams.feature_samples@8");
SRT_STATIC_ASSERT(offsetof(srt_denoise_params, sigma_luminance) == 12, "DenoiseParams.sigma_luminance@12");
SRT_STATIC_ASSERT(offsetof(srt_denoise_params, sigma_albedo) == 24, "DenoiseParams.sigma_albedo@24");
SRT_STATIC_ASSERT(offsetof(srt_denoise_params, reserved) == 28, "DenoiseParams.reserved@28");
SRT_STATIC_ASSERT(sizeof(srt_temporal_params) == 32, "TemporalParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_temporal_params, history_limit) == 4, "TemporalParams.history_limit@4");
SRT_STATIC_ASSERT(offsetof(srt_temporal_params, normal_threshold) == 8, "TemporalParams.normal_threshold@8");
SRT_STATIC_ASSERT(offsetof(srt_temporal_params, depth_threshold) == 12, "TemporalParams.depth_threshold@12");
SRT_STATIC_ASSERT(offsetof(srt_temporal_params, reserved) == 16, "TemporalParams.reserved@16");
SRT_STATIC_ASSERT(sizeof(srt_exposure_params) == 48, "ExposureParams 48 B");
SRT_STATIC_ASSERT(offsetof(srt_exposure_params, ev) == 8, "ExposureParams.ev@8");
SRT_STATIC_ASSERT(offsetof(srt_exposure_params, low_permille) == 16, "ExposureParams.low_permille@16");
SRT_STATIC_ASSERT(offsetof(srt_exposure_params, adapt) == 24, "ExposureParams.adapt@24");
SRT_STATIC_ASSERT(offsetof(srt_exposure_params, min_ev) == 28, "ExposureParams.min_ev@28");
SRT_STATIC_ASSERT(offsetof(srt_exposure_params, reserved) == 36, "ExposureParams.reserved@36");
SRT_STATIC_ASSERT(sizeof(srt_bloom_params) == 32, "BloomParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_bloom_params, clamp) == 20, "BloomParams.clamp@20");
SRT_STATIC_ASSERT(offsetof(srt_bloom_params, levels) == 24, "BloomParams.levels@24");
SRT_STATIC_ASSERT(sizeof(srt_noise_params) == 32, "NoiseParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_noise_params, permille) == 12, "NoiseParams.permille@12");
SRT_STATIC_ASSERT(offsetof(srt_noise_params, check_every) == 20, "NoiseParams.check_every@20");
SRT_STATIC_ASSERT(offsetof(srt_noise_params, reserved) == 24, "NoiseParams.reserved@24");
SRT_STATIC_ASSERT(sizeof(srt_noise_result) == 32, "NoiseResult 32 B");
SRT_STATIC_ASSERT(offsetof(srt_noise_result, level) == 28, "NoiseResult.level@28");
SRT_STATIC_ASSERT(sizeof(srt_material_texture) == 16, "MaterialTexture 16 B");
SRT_STATIC_ASSERT(offsetof(srt_material_texture, scale_u) == 8, "MaterialTexture.scale_u@8");
SRT_STATIC_ASSERT(sizeof(srt_ray) == 32, "Ray 32 B");
SRT_STATIC_ASSERT(offsetof(srt_ray, direction) == 16, "Ray.direction@16");
SRT_STATIC_ASSERT(sizeof(srt_ray_hit) == 32, "RayHit 32 B");
SRT_STATIC_ASSERT(offsetof(srt_ray_hit, normal) == 16, "RayHit.normal@16");
SRT_STATIC_ASSERT(sizeof(srt_segment) == 32, "Segment 32 B");
SRT_STATIC_ASSERT(offsetof(srt_segment, end_gap) == 12, "Segment.end_gap@12");
SRT_STATIC_ASSERT(offsetof(srt_segment, to) == 16, "Segment.to@16");
SRT_STATIC_ASSERT(sizeof(srt_selection_params) == 32, "SelectionParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_selection_params, outline_argb) == 8, "SelectionParams.outline_argb@8");
SRT_STATIC_ASSERT(offsetof(srt_selection_params, reserved) == 16, "SelectionParams.reserved@16");
SRT_STATIC_ASSERT(sizeof(srt_ao_params) == 32, "AoParams 32 B");
SRT_STATIC_ASSERT(offsetof(srt_ao_params, background) == 16, "AoParams.background@16");
SRT_STATIC_ASSERT(sizeof(srt_point_query) == 16, "PointQuery 16 B");
SRT_STATIC_ASSERT(offsetof(srt_point_query, max_distance) == 12, "PointQuery.max_distance@12");
SRT_STATIC_ASSERT(sizeof(srt_nearest) == 32, "Nearest 32 B");
SRT_STATIC_ASSERT(offsetof(srt_nearest, material) == 12, "Nearest.material@12");
SRT_STATIC_ASSERT(offsetof(srt_nearest, point) == 16, "Nearest.point@16");
SRT_STATIC_ASSERT(offsetof(srt_nearest, flags) == 28, "Nearest.flags@28");
SRT_STATIC_ASSERT(sizeof(srt_area) == 32, "Area 32 B");
SRT_STATIC_ASSERT(offsetof(srt_area, n_vertices) == 16, "Area.n_vertices@16");
SRT_STATIC_ASSERT(sizeof(srt_area_summary) == 32, "AreaSummary 32 B");
SRT_STATIC_ASSERT(offsetof(srt_area_summary, target_pixels) == 16, "AreaSummary.target_pixels@16");

#endif /* SRT_TYPES_H */
