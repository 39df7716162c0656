/* srt_oracle.c — CPU restatement of the reference path-tracing hot path.
 *
 * TEST INFRASTRUCTURE ONLY. Nothing in the product path (simple-raytracer_amd/,
 * include/) may include, link, import or execute this file or anything else under
 * oracle/. Allowed users: tests/, __graft_entry__.smoke() and the `cpu_baseline`
 * leg of bench.py — as the checker, never as the thing measured or shipped.
 *
 * What it restates: the OpenCL kernels `render` and `average` of
 * /root/reference/src/render.cl (lines cited at every function), scalar C, one
 * pixel at a time, same operation order, same RNG stream. The OpenCL built-ins
 * (implementation-defined within ULP bounds) are taken from
 * simple-raytracer_amd/csrc/detmath.h — the same definitions the HIP kernels and
 * the reference-kernel shim (oracle/cl_builtins_shim.cpp) use.
 *
 * PARITY UNPINNED at the built-in boundary: the reference has no tests, fixtures or golden
 * vectors, and its program cannot be built in this image. What this file IS checked against:
 * `make -C oracle ref` compiles the reference's own render.cl for x86-64
 * (oracle/_ref/libsrt_ref.so) with the OpenCL built-ins supplied by cl_builtins_shim.cpp from
 * detmath.h; tests/test_oracle_vs_ref.py requires this file to be BIT-IDENTICAL to that build
 * (control flow, RNG stream, draw and operation order are then the reference's own), and
 * tests/golden/ holds vectors generated from it (tests/golden/make_golden.py) so the same check
 * runs where /root/reference is absent. The built-ins themselves are held to the OpenCL ULP
 * bounds against glibc (tests/test_detmath.py) and to statistical agreement with a glibc-backed
 * build of the same object (tests/test_oracle_statistics.py). See DESIGN.md "Oracle and parity".
 *
 * The TEXTURED entry points (orc_render_textured, orc_trace_paths_textured, orc_features_textured, orc_sample_texture)
 * restate this repository's own contract, include/srt_abi.h "albedo textures": they have no counterpart in the reference and
 * no `_ref` build to check against. What earns them trust is tests/test_oracle_textures.py: with nothing bound they are the
 * untextured functions bit for bit, at the first hit they equal the independent numpy restatement tests/texture_ref.py,
 * and hand-computed paths pin how the texel meets the mask. The untextured entry points pass a NULL table and compile
 * `trace` without a trace of it (trace_body's `textured` is a literal).
 *
 * Build: gcc -O2 -ffp-contract=off [-mfma] -fopenmp -fPIC -shared (oracle/Makefile).
 */
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "../include/srt_types.h"
#include "../simple-raytracer_amd/csrc/detmath.h"

#ifdef _OPENMP
#include <omp.h>
#endif

typedef struct {
	float x, y, z;
} v3;

/* deterministic work counters: schedule independent */
enum {
	ORC_C_PATHS = 0,
	ORC_C_RAYS,        /* closest_intersection calls = path segments */
	ORC_C_SPHERE,      /* intersect_sphere calls */
	ORC_C_PLANE,       /* intersect_plane calls */
	ORC_C_AABB,        /* intersection_aabb calls */
	ORC_C_TRI,         /* intersect_triangle calls */
	ORC_C_TRI_PASS_U,  /* triangle tests that got past the u check */
	ORC_C_BOUNCE,      /* shaded hits that drew a new direction */
	ORC_C_SKY,         /* sky_box evaluations */
	ORC_C_NAN_PIXELS,  /* pixels whose per-dispatch colour is NaN in any channel */
	ORC_C_COUNT
};

/* ---- vector helpers with the pinned operation order ------------------------ */
static inline v3 V(float x, float y, float z) {
	v3 r = {x, y, z};
	return r;
}
static inline v3 f3(const srt_float3 *p) { return V(p->x, p->y, p->z); }
static inline v3 vadd(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 vsub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 vmul(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline v3 vscale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static inline v3 vdivs(v3 a, float s) { return V(a.x / s, a.y / s, a.z / s); }
static inline v3 vneg(v3 a) { return V(-a.x, -a.y, -a.z); }
/* the built-ins dot, cross, normalize, mix as detmath.h pins them (FMA forms) */
static inline float vdot(v3 a, v3 b) { return dm_dot3(a.x, a.y, a.z, b.x, b.y, b.z); }
static inline v3 vcross(v3 a, v3 b) {
	return V(dm_cross1(a.y, b.z, a.z, b.y), dm_cross1(a.z, b.x, a.x, b.z), dm_cross1(a.x, b.y, a.y, b.x));
}
static inline v3 vnormalize(v3 a) {
	float v[3] = {a.x, a.y, a.z};
	dm_normalize3(v, v);
	return V(v[0], v[1], v[2]);
}
static inline v3 vmix(v3 x, v3 y, float a) {
	return V(dm_mix(x.x, y.x, a), dm_mix(x.y, y.y, a), dm_mix(x.z, y.z, a));
}

/* render.cl:114-120 — column-major 4x4 times (v, w); xyz of the result.
 * Each row is ((m0*v.x + m1*v.y) + m2*v.z) + m3*w, left associated. */
static inline v3 mat_by_vec(const srt_float4 *m, v3 v, float w) {
	return V(((m[0].x * v.x + m[1].x * v.y) + m[2].x * v.z) + m[3].x * w,
	         ((m[0].y * v.x + m[1].y * v.y) + m[2].y * v.z) + m[3].y * w,
	         ((m[0].z * v.x + m[1].z * v.y) + m[2].z * v.z) + m[3].z * w);
}

/* render.cl:139-141 */
static inline v3 reflect3(v3 v, v3 n) { return vsub(v, vscale(n, 2.0f * vdot(v, n))); }

/* render.cl:143-148 — PCG-RXS-M-XS-32; (float)UINT_MAX == 2^32 */
float orc_random_float(uint32_t *seed) {
	*seed = *seed * 747796405u + 2891336453u;
	uint32_t result = ((*seed >> ((*seed >> 28) + 4)) ^ *seed) * 277803737u;
	result = (result >> 22) ^ result;
	return (float)result / 4294967296.0f;
}

/* render.cl:150-154 */
static inline float random_float_normal(uint32_t *seed) {
	float theta = 6.28318548f * orc_random_float(seed); /* 2 * M_PI_F */
	float rho = dm_sqrtf(-2.0f * dm_logf(orc_random_float(seed)));
	return rho * dm_cosf(theta);
}

/* render.cl:156-158 — components drawn x, then y, then z */
static inline v3 random_direction(uint32_t *seed) {
	float x = random_float_normal(seed);
	float y = random_float_normal(seed);
	float z = random_float_normal(seed);
	return vnormalize(V(x, y, z));
}

/* render.cl:160-163 */
static inline v3 random_direction_hemisphere(v3 normal, uint32_t *seed) {
	v3 dir = random_direction(seed);
	return vscale(dir, dm_sign(vdot(normal, dir)));
}

/* render.cl:173-178 — the literals are double, so this runs in fp64 */
float orc_shlick_reflectance(float mu, float cos_theta) {
	float r0 = (float)((1.0 - (double)mu) / (1.0 + (double)mu));
	r0 = r0 * r0;
	return (float)((double)r0 + (1.0 - (double)r0) * dm_pown_d(1.0 - (double)cos_theta, 5));
}

/* render.cl:180-204 */
int orc_intersect_sphere(const srt_sphere *sphere, const float *o, const float *d, float *t) {
	v3 org = V(o[0], o[1], o[2]), dir = V(d[0], d[1], d[2]);
	v3 rayToCenter = vsub(f3(&sphere->position), org);
	float b = vdot(rayToCenter, dir);
	float c = vdot(rayToCenter, rayToCenter) - sphere->radius * sphere->radius;
	float disc = b * b - c;
	if (disc < 0.0f) return 0;
	*t = b - dm_sqrtf(disc);
	if (*t < 0.0f) {
		*t = b + dm_sqrtf(disc);
		if (*t < 0.0f) return 0;
	}
	return 1;
}

/* render.cl:206-221 */
int orc_intersect_plane(const srt_plane *plane, const float *o, const float *d, float *t) {
	v3 org = V(o[0], o[1], o[2]), dir = V(d[0], d[1], d[2]);
	float denom = vdot(f3(&plane->normal), dir);
	if (dm_fabs(denom) == 0.0f) return 0;
	float tmp = vdot(f3(&plane->normal), vsub(f3(&plane->position), org)) / denom;
	if (tmp < 0.0f) return 0;
	*t = tmp;
	return 1;
}

/* render.cl:223-241 — returns the "shifted" weights (w2, w0, w1) */
static inline v3 barycentric_weights(v3 p0, v3 p1, v3 p2, v3 p) {
	v3 v0 = vsub(p1, p0);
	v3 v1 = vsub(p2, p0);
	v3 v2 = vsub(p, p0);
	float d00 = vdot(v0, v0);
	float d01 = vdot(v0, v1);
	float d11 = vdot(v1, v1);
	float d20 = vdot(v2, v0);
	float d21 = vdot(v2, v1);
	float denom = d00 * d11 - d01 * d01;
	float w0 = (d11 * d20 - d01 * d21) / denom;
	float w1 = (d00 * d21 - d01 * d20) / denom;
	float w2 = 1.0f - w0 - w1;
	return V(w2, w0, w1);
}

/* render.cl:243-275 — Moller-Trumbore, no epsilon, two-sided.
 * pass_u (optional) reports whether the u-range check was passed. */
static inline int intersect_triangle(v3 p0, v3 p1, v3 p2, v3 org, v3 dir, float *t, int *pass_u) {
	v3 edge1 = vsub(p1, p0);
	v3 edge2 = vsub(p2, p0);
	v3 h = vcross(dir, edge2);
	float a = vdot(edge1, h);
	if (a == 0.0f) return 0;
	float f = 1.0f / a;
	v3 s = vsub(org, p0);
	float u = f * vdot(s, h);
	if (u < 0.0f || u > 1.0f) return 0;
	if (pass_u) *pass_u = 1;
	v3 q = vcross(s, edge1);
	float v = f * vdot(dir, q);
	if (v < 0.0f || u + v > 1.0f) return 0;
	*t = f * vdot(edge2, q);
	if (*t > 0.0f) return 1;
	return 0;
}

int orc_intersect_triangle(const float *p0, const float *p1, const float *p2, const float *o, const float *d, float *t) {
	return intersect_triangle(V(p0[0], p0[1], p0[2]), V(p1[0], p1[1], p1[2]), V(p2[0], p2[1], p2[2]),
	                          V(o[0], o[1], o[2]), V(d[0], d[1], d[2]), t, NULL);
}

/* render.cl:279-290 */
int orc_intersection_aabb(const float *bmin, const float *bmax, const float *o, const float *inv_dir, float tmax) {
	float tmin = 0.0f;
	for (int d = 0; d < 3; d++) {
		float t1 = (bmin[d] - o[d]) * inv_dir[d];
		float t2 = (bmax[d] - o[d]) * inv_dir[d];
		tmin = dm_max(tmin, dm_min(t1, t2));
		tmax = dm_min(tmax, dm_max(t1, t2));
	}
	return tmin < tmax;
}

/* ---- albedo textures (include/srt_abi.h "albedo textures"): this repository's own contract, no counterpart in the
 * reference. The table a caller hands to the orc_*_textured entry points; NULL means no textures at all. ---- */
typedef struct {
	int32_t has_frame; /* 0: the plane's normal is zero or not finite -- it keeps the material colour */
	float T[3], B[3];  /* tests/texture_ref.py plane_frame (float64, rounded to float32); never made here */
} orc_plane_frame;

typedef struct {
	const srt_texture_desc *images; /* rgba, width, height; row 0 = bottom */
	int32_t num_images;
	int32_t first_hit_only; /* coverage probe of the tests: hits after a path's first keep the material colour */
	const srt_material_texture *bindings; /* one per material */
	const float *tri_uvs;                 /* num triangles x 3 x 2, or NULL */
	const orc_plane_frame *frames;        /* one per shape (read for planes only) */
} orc_textures;

typedef struct {
	const srt_scene_data *data;
	const srt_shape *shapes;
	const srt_triangle *triangles;
	const srt_material *materials;
	const float *sky; /* RGBA32F, row 0 first */
	int sky_w, sky_h;
	const orc_textures *tex; /* NULL: none (every reference-parity entry point) */
} scene_t;

typedef struct {
	v3 position, normal;
	int front;
	float t; /* tmin: the distance along the (unit) ray to the closest hit, INFINITY when nothing was hit */
	int shape;    /* index of the closest shape; written with tmin */
	uint32_t tri; /* a model's winning triangle, counted from its triangle_index; written with tmin */
} hit_t;

/* render.cl:293-378 */
static int closest_intersection(const scene_t *scene, v3 org, v3 dir, hit_t *rayhit, uint64_t *ctr) {
	int closest = -1;
	float tmin = DM_INF_F;
	float o[3] = {org.x, org.y, org.z}, d[3] = {dir.x, dir.y, dir.z};
	float inv_dir[3] = {1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z};
	ctr[ORC_C_RAYS]++;

	for (int i = 0; i < scene->data->num_shapes; i++) {
		const srt_shape *shape = &scene->shapes[i];
		if (shape->type == SRT_SHAPE_SPHERE) {
			const srt_sphere *sphere = &shape->shape.sphere;
			float t_i;
			ctr[ORC_C_SPHERE]++;
			if (orc_intersect_sphere(sphere, o, d, &t_i)) {
				if (t_i < tmin) {
					tmin = t_i;
					closest = shape->material;
					rayhit->shape = i;
					rayhit->position = vadd(org, vscale(dir, tmin));
					rayhit->normal = vdivs(vsub(rayhit->position, f3(&sphere->position)), sphere->radius);
				}
			}
		} else if (shape->type == SRT_SHAPE_MODEL) {
			const srt_model *model = &shape->shape.model;
			float bmin[3] = {model->bounding_min.x, model->bounding_min.y, model->bounding_min.z};
			float bmax[3] = {model->bounding_max.x, model->bounding_max.y, model->bounding_max.z};
			ctr[ORC_C_AABB]++;
			if (!orc_intersection_aabb(bmin, bmax, o, inv_dir, tmin)) continue;
			for (size_t j = 0; j < model->num_triangles; j++) {
				const srt_triangle *tri = &scene->triangles[model->triangle_index + j];
				/* render.cl:325-328: positions to world space, per ray */
				v3 p0 = mat_by_vec(model->transform, f3(&tri->vertices[0].pos), 1.0f);
				v3 p1 = mat_by_vec(model->transform, f3(&tri->vertices[1].pos), 1.0f);
				v3 p2 = mat_by_vec(model->transform, f3(&tri->vertices[2].pos), 1.0f);
				float t_i;
				int pass_u = 0;
				ctr[ORC_C_TRI]++;
				int hit = intersect_triangle(p0, p1, p2, org, dir, &t_i, &pass_u);
				ctr[ORC_C_TRI_PASS_U] += (uint64_t)pass_u;
				if (hit) {
					if (t_i < tmin) {
						tmin = t_i;
						closest = shape->material;
						rayhit->shape = i;
						rayhit->tri = (uint32_t)j;
						rayhit->position = vadd(org, vscale(dir, tmin));
						/* render.cl:340-343 smooth shading; forward matrix, w = 0 */
						v3 w = barycentric_weights(p0, p1, p2, rayhit->position);
						v3 n = vadd(vadd(vscale(f3(&tri->vertices[0].normal), w.x),
						                 vscale(f3(&tri->vertices[1].normal), w.y)),
						            vscale(f3(&tri->vertices[2].normal), w.z));
						n = mat_by_vec(model->transform, n, 0.0f);
						rayhit->normal = vnormalize(n);
					}
				}
			}
		} else if (shape->type == SRT_SHAPE_PLANE) {
			const srt_plane *plane = &shape->shape.plane;
			float t_i;
			ctr[ORC_C_PLANE]++;
			if (orc_intersect_plane(plane, o, d, &t_i)) {
				if (t_i < tmin) {
					tmin = t_i;
					closest = shape->material;
					rayhit->shape = i;
					rayhit->normal = f3(&plane->normal);
					rayhit->position = vadd(org, vscale(dir, tmin));
				}
			}
		}
	}
	/* render.cl:369 `tmin == FLT_MAX` never fires (tmin starts at INFINITY) */
	rayhit->t = tmin;
	rayhit->front = vdot(rayhit->normal, dir) < 0.0f;
	rayhit->normal = vscale(rayhit->normal, rayhit->front ? 1.0f : -1.0f);
	return closest;
}

/* OpenCL 3.0 §8.2 linear filter, normalized coords, CLAMP_TO_EDGE
 * (sampler: /root/reference/src/tracer.cpp:47-48). Manual float bilinear. */
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static v3 sample_sky(const scene_t *scene, float s, float t) {
	int W = scene->sky_w, H = scene->sky_h;
	float fu = s * (float)W - 0.5f;
	float fv = t * (float)H - 0.5f;
	/* pin float->int for NaN / out-of-range so x86 and gfx950 agree */
	float cu = dm_clamp(fu, -1.0f, (float)W);
	float cv = dm_clamp(fv, -1.0f, (float)H);
	if (!(cu == cu)) cu = 0.0f;
	if (!(cv == cv)) cv = 0.0f;
	float x0f = __builtin_floorf(cu), y0f = __builtin_floorf(cv);
	float a = fu - x0f, b = fv - y0f;
	int x0 = (int)x0f, y0 = (int)y0f;
	int i0 = clampi(x0, 0, W - 1), i1 = clampi(x0 + 1, 0, W - 1);
	int j0 = clampi(y0, 0, H - 1), j1 = clampi(y0 + 1, 0, H - 1);
	const float *T00 = scene->sky + 4 * ((size_t)j0 * W + i0);
	const float *T10 = scene->sky + 4 * ((size_t)j0 * W + i1);
	const float *T01 = scene->sky + 4 * ((size_t)j1 * W + i0);
	const float *T11 = scene->sky + 4 * ((size_t)j1 * W + i1);
	float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	v3 r;
	r.x = dm_bilinear(w00, T00[0], w10, T10[0], w01, T01[0], w11, T11[0]);
	r.y = dm_bilinear(w00, T00[1], w10, T10[1], w01, T01[1], w11, T11[1]);
	r.z = dm_bilinear(w00, T00[2], w10, T10[2], w01, T01[2], w11, T11[2]);
	return r;
}

/* render.cl:380-394 */
static v3 sky_box(const scene_t *scene, v3 dir) {
	const srt_scene_data *sd = scene->data;
	float lobe = dm_powf(dm_max(vdot(dir, vneg(f3(&sd->sun_direction))), 0.0f), sd->sun_focus);
	v3 sun = vscale(vscale(f3(&sd->sun_color), lobe), sd->sun_intensity);
	float u = dm_atan2pif(dir.z, dir.x) * 0.5f + 0.5f;
	float v = dir.y * 0.5f + 0.5f;
	return vadd(sample_sky(scene, u, v), sun);
}

/* ---- albedo textures: include/srt_abi.h "albedo textures", restated from the header's words ---------------------- */
static inline int wrapi(int x, int n) { /* x mod n, never negative */
	int m = x % n;
	return m < 0 ? m + n : m;
}

/* The sampler, addressing REPEAT, over a W x H image (row 0 = bottom); u, v already scaled. */
static v3 sample_texture(const float *rgba, int W, int H, int filter, float u, float v) {
	float fu = u * (float)W, fv = v * (float)H;
	if (filter == SRT_FILTER_LINEAR) {
		fu = fu - 0.5f;
		fv = fv - 0.5f;
	}
	/* NaN, infinite or not below 2^30 in magnitude: the texel (0, 0) as stored */
	if (!(dm_fabs(fu) < 1073741824.0f) || !(dm_fabs(fv) < 1073741824.0f)) return V(rgba[0], rgba[1], rgba[2]);
	float x0f = __builtin_floorf(fu), y0f = __builtin_floorf(fv);
	int i0 = wrapi((int)x0f, W), j0 = wrapi((int)y0f, H);
	const float *T00 = rgba + 4 * ((size_t)j0 * W + i0);
	if (filter != SRT_FILTER_LINEAR) return V(T00[0], T00[1], T00[2]);
	float a = fu - x0f, b = fv - y0f;
	int i1 = wrapi(i0 + 1, W), j1 = wrapi(j0 + 1, H);
	const float *T10 = rgba + 4 * ((size_t)j0 * W + i1);
	const float *T01 = rgba + 4 * ((size_t)j1 * W + i0);
	const float *T11 = rgba + 4 * ((size_t)j1 * W + i1);
	float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
	return V(dm_bilinear(w00, T00[0], w10, T10[0], w01, T01[0], w11, T11[0]),
	         dm_bilinear(w00, T00[1], w10, T10[1], w01, T01[1], w11, T11[1]),
	         dm_bilinear(w00, T00[2], w10, T10[2], w01, T01[2], w11, T11[2]));
}

/* dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, unfused (the plane's UV) */
static inline float dot_unfused(v3 a, const float *b) { return (a.x * b[0] + a.y * b[1]) + a.z * b[2]; }

/* The colour a hit multiplies into the mask: the texel at the hit's UV where its material has a texture bound (a plane
 * needs a frame besides), else the material colour. *looked = 1 when a texel was read. X = hit->position. */
static v3 albedo(const scene_t *scene, const hit_t *hit, int material_index, int *looked) {
	const orc_textures *tex = scene->tex;
	const srt_material_texture *bind = &tex->bindings[material_index];
	const v3 mcolor = f3(&scene->materials[material_index].color);
	*looked = 0;
	if (bind->texture < 0) return mcolor;
	const srt_shape *shape = &scene->shapes[hit->shape];
	const v3 X = hit->position;
	float u, v;
	if (shape->type == SRT_SHAPE_SPHERE) {
		/* the normal as made from X, whichever side was hit */
		v3 n = vdivs(vsub(X, f3(&shape->shape.sphere.position)), shape->shape.sphere.radius);
		u = dm_atan2pif(n.z, n.x) * 0.5f + 0.5f;
		v = n.y * 0.5f + 0.5f;
	} else if (shape->type == SRT_SHAPE_PLANE) {
		const orc_plane_frame *fr = &tex->frames[hit->shape];
		if (!fr->has_frame) return mcolor;
		v3 d = vsub(X, f3(&shape->shape.plane.position));
		u = dot_unfused(d, fr->T);
		v = dot_unfused(d, fr->B);
	} else {
		const srt_model *model = &shape->shape.model;
		const size_t ti = (size_t)model->triangle_index + hit->tri;
		const srt_triangle *tri = &scene->triangles[ti];
		v3 p0 = mat_by_vec(model->transform, f3(&tri->vertices[0].pos), 1.0f);
		v3 p1 = mat_by_vec(model->transform, f3(&tri->vertices[1].pos), 1.0f);
		v3 p2 = mat_by_vec(model->transform, f3(&tri->vertices[2].pos), 1.0f);
		v3 w = barycentric_weights(p0, p1, p2, X); /* (w2, w0, w1): the shading's weights */
		const float w2 = w.x, w0 = w.y, w1 = w.z;
		u = w0, v = w1;
		if (tex->tri_uvs) {
			const float *t = tex->tri_uvs + 6 * ti;
			u = (t[0] * w2 + t[2] * w0) + t[4] * w1;
			v = (t[1] * w2 + t[3] * w0) + t[5] * w1;
		}
	}
	const srt_texture_desc *img = &tex->images[bind->texture];
	*looked = 1;
	return sample_texture(img->rgba, img->width, img->height, bind->filter, u * bind->scale_u, v * bind->scale_v);
}

/* render.cl:396-471. One body, compiled twice: `textured` is a literal at both call sites, so the untextured form is the
 * reference's text and nothing else. lookups (textured only, may be NULL): [0] += texels read at the path's first hit,
 * [1] += texels read at later hits, [2] += specular bounces whose mix(texel, 1, 1) is not 1.0f in every channel (the
 * texel's bits reach the mask where a colour "is ignored"). */
static inline __attribute__((always_inline)) v3 trace_body(const srt_render_data *render, const scene_t *scene, v3 org, v3 dir, uint32_t seed,
                                                           uint64_t *ctr, const int textured, int32_t *lookups) {
	v3 color = V(0.f, 0.f, 0.f);
	v3 mask = V(1.f, 1.f, 1.f);
	hit_t rayhit;
	memset(&rayhit, 0, sizeof rayhit);

	for (int i = 0; i < render->num_bounces; i++) {
		int material_index = closest_intersection(scene, org, dir, &rayhit, ctr);
		if (material_index >= 0) {
			if (render->show_normals) {
				color = V(rayhit.normal.x * 0.5f + 0.5f, rayhit.normal.y * 0.5f + 0.5f, rayhit.normal.z * 0.5f + 0.5f);
				break;
			}
			const srt_material *material = &scene->materials[material_index];
			color = vadd(color, vscale(vmul(mask, f3(&material->emission)), material->emission_strength));
			if (i == render->num_bounces - 1) break;
			ctr[ORC_C_BOUNCE]++;

			org = rayhit.position;
			/* cosine weighted: 6 draws */
			v3 random_dir = vnormalize(vadd(rayhit.normal, random_direction_hemisphere(rayhit.normal, &seed)));
			v3 reflected_dir = reflect3(dir, rayhit.normal);
			int is_metallic = material->metallic > orc_random_float(&seed);
			int is_specular = material->specular > orc_random_float(&seed);
			v3 rough_dir = vmix(random_dir, reflected_dir, material->smoothness);
			int is_transparent = material->transmittance > orc_random_float(&seed);
			v3 mcolor = f3(&material->color);
			int looked = 0;
			if (textured && !(scene->tex->first_hit_only && i > 0)) {
				mcolor = albedo(scene, &rayhit, material_index, &looked);
				if (lookups) lookups[i > 0] += looked;
			}

			if (!is_transparent) {
				dir = vmix(random_dir, rough_dir, (is_metallic || is_specular) ? 1.0f : 0.0f);
				v3 f = vmix(mcolor, V(1.0f, 1.0f, 1.0f), is_specular ? 1.0f : 0.0f);
				mask = vmul(mask, f);
				if (textured && lookups && looked && is_specular && (f.x != 1.0f || f.y != 1.0f || f.z != 1.0f)) lookups[2]++;
			} else {
				v3 in_dir = reflect3(rough_dir, rayhit.normal);
				float mu = rayhit.front ? 1.0f / material->refraction_index : material->refraction_index;
				float cos_theta = dm_min(1.0f, vdot(in_dir, vneg(rayhit.normal)));
				float sin_theta = dm_sqrtf(1.0f - cos_theta * cos_theta);
				int reflected = mu * sin_theta > 1.0f;
				if (!reflected) reflected = orc_shlick_reflectance(mu, cos_theta) > orc_random_float(&seed);
				if (reflected) {
					dir = rough_dir;
				} else {
					v3 out_perp = vscale(vadd(in_dir, vscale(rayhit.normal, cos_theta)), mu);
					float lsq = out_perp.x * out_perp.x + out_perp.y * out_perp.y + out_perp.z * out_perp.z;
					v3 out_parallel = vscale(rayhit.normal, -dm_sqrtf(dm_fabs(1.0f - lsq)));
					dir = vadd(out_perp, out_parallel);
					mask = vmul(mask, mcolor);
				}
			}
			dir = vnormalize(dir);
			org = vadd(org, vscale(vscale(rayhit.normal, dm_sign(vdot(rayhit.normal, dir))), 0.001f));
		} else {
			ctr[ORC_C_SKY]++;
			mask = vmul(mask, sky_box(scene, dir));
			color = vadd(color, mask);
			break;
		}
	}
	return color;
}

static v3 trace(const srt_render_data *render, const scene_t *scene, v3 org, v3 dir, uint32_t seed, uint64_t *ctr) {
	return trace_body(render, scene, org, dir, seed, ctr, 0, NULL);
}
static v3 trace_textured(const srt_render_data *render, const scene_t *scene, v3 org, v3 dir, uint32_t seed, uint64_t *ctr,
                         int32_t *lookups) {
	return trace_body(render, scene, org, dir, seed, ctr, 1, lookups);
}

/* render.cl:489-516: the camera ray of (pixel id, sample) -> org, unit dir; returns the seed after the two jitter draws */
static inline uint32_t camera_ray(const srt_render_data *data, uint32_t id, uint32_t sample, v3 *org, v3 *dir) {
	int px = (int)(id % (uint32_t)data->width), py = (int)(id / (uint32_t)data->width);
	uint32_t seed = (sample + id * (uint32_t)data->num_samples) * data->time * 5304u;
	float ndc_x = ((float)px + orc_random_float(&seed)) / (float)data->width;
	float ndc_y = ((float)py + orc_random_float(&seed)) / (float)data->height;
	float sx = ((2.f * ndc_x - 1.f) * data->aspect_ratio) * data->fov_scale;
	float sy = (1.f - 2.f * ndc_y) * data->fov_scale;
	*org = V(data->camera_to_world[3].x, data->camera_to_world[3].y, data->camera_to_world[3].z);
	*dir = vnormalize(mat_by_vec(data->camera_to_world, V(sx, sy, -1.0f), 0.0f));
	return seed;
}

/* render.cl:483-523 for one pixel; returns the per-dispatch colour (already /num_samples) */
static inline __attribute__((always_inline)) v3 render_pixel_body(const srt_render_data *data, const scene_t *scene, int px, int py,
                                                                  uint64_t *ctr, const int textured) {
	uint32_t id = (uint32_t)px + (uint32_t)py * (uint32_t)data->width;
	v3 color = V(0.f, 0.f, 0.f);
	for (int sample = 0; sample < data->num_samples; sample++) {
		v3 org, dir;
		uint32_t seed = camera_ray(data, id, (uint32_t)sample, &org, &dir);
		ctr[ORC_C_PATHS]++;
		color = vadd(color, textured ? trace_textured(data, scene, org, dir, seed, ctr, NULL) : trace(data, scene, org, dir, seed, ctr));
	}
	return vdivs(color, (float)data->num_samples);
}
static v3 render_pixel(const srt_render_data *data, const scene_t *scene, int px, int py, uint64_t *ctr) {
	return render_pixel_body(data, scene, px, py, ctr, 0);
}
static v3 render_pixel_textured(const srt_render_data *data, const scene_t *scene, int px, int py, uint64_t *ctr) {
	return render_pixel_body(data, scene, px, py, ctr, 1);
}

/* The `render` kernel over rows [y0, y1): canvas[id] += colour. canvas is the full
 * width*height image of 16-byte float3 (x,y,z,pad). counters may be NULL. */
void orc_render_strided(const srt_render_data *data, const srt_scene_data *scene_data, float *canvas,
                        const srt_shape *shapes, const srt_triangle *triangles, const srt_material *materials,
                        const float *sky_rgba, int sky_w, int sky_h, int y0, int y1, int ystride, int nthreads,
                        uint64_t *counters);

static void render_rows(const srt_render_data *data, const scene_t *scene, float *canvas, int y0, int y1, int ystride, int nthreads,
                        uint64_t *counters);

void orc_render(const srt_render_data *data, const srt_scene_data *scene_data, float *canvas,
                const srt_shape *shapes, const srt_triangle *triangles, const srt_material *materials,
                const float *sky_rgba, int sky_w, int sky_h, int y0, int y1, int nthreads, uint64_t *counters) {
	orc_render_strided(data, scene_data, canvas, shapes, triangles, materials, sky_rgba, sky_w, sky_h, y0, y1, 1, nthreads,
	                   counters);
}

/* rows y0, y0+ystride, ... < y1 (a strided sample of the frame for the CPU baseline) */
void orc_render_strided(const srt_render_data *data, const srt_scene_data *scene_data, float *canvas,
                        const srt_shape *shapes, const srt_triangle *triangles, const srt_material *materials,
                        const float *sky_rgba, int sky_w, int sky_h, int y0, int y1, int ystride, int nthreads,
                        uint64_t *counters) {
	scene_t scene = {scene_data, shapes, triangles, materials, sky_rgba, sky_w, sky_h, NULL};
	render_rows(data, &scene, canvas, y0, y1, ystride, nthreads, counters);
}

/* The same with albedo textures (tex == NULL: none, and then this is orc_render_strided). */
void orc_render_textured(const srt_render_data *data, const srt_scene_data *scene_data, float *canvas, const srt_shape *shapes,
                         const srt_triangle *triangles, const srt_material *materials, const float *sky_rgba, int sky_w, int sky_h,
                         const orc_textures *tex, int y0, int y1, int ystride, int nthreads, uint64_t *counters) {
	scene_t scene = {scene_data, shapes, triangles, materials, sky_rgba, sky_w, sky_h, tex};
	render_rows(data, &scene, canvas, y0, y1, ystride, nthreads, counters);
}

static void render_rows(const srt_render_data *data, const scene_t *scene, float *canvas, int y0, int y1, int ystride, int nthreads,
                        uint64_t *counters) {
	const int textured = scene->tex != NULL && !data->show_normals; /* chosen once per call */
	uint64_t total[ORC_C_COUNT];
	memset(total, 0, sizeof total);
#ifdef _OPENMP
	if (nthreads > 0) omp_set_num_threads(nthreads);
#else
	(void)nthreads;
#endif
#pragma omp parallel
	{
		uint64_t ctr[ORC_C_COUNT];
		memset(ctr, 0, sizeof ctr);
		if (ystride < 1) ystride = 1;
		const int nrows = y1 > y0 ? (y1 - y0 + ystride - 1) / ystride : 0;
		/* pixels, not rows, are the unit of work: a sample of a few rows still fills every core */
#pragma omp for collapse(2) schedule(dynamic, 16)
		for (int r = 0; r < nrows; r++) {
			for (int x = 0; x < data->width; x++) {
				const int y = y0 + r * ystride;
				v3 c = textured ? render_pixel_textured(data, scene, x, y, ctr) : render_pixel(data, scene, x, y, ctr);
				float *out = canvas + 4 * ((size_t)y * data->width + x);
				out[0] += c.x;
				out[1] += c.y;
				out[2] += c.z;
				if (c.x != c.x || c.y != c.y || c.z != c.z) ctr[ORC_C_NAN_PIXELS]++;
			}
		}
#pragma omp critical
		for (int k = 0; k < ORC_C_COUNT; k++) total[k] += ctr[k];
	}
	if (counters)
		for (int k = 0; k < ORC_C_COUNT; k++) counters[k] += total[k];
}

/* radiance of single (pixel, sample) paths — for trace-level golden vectors */
void orc_trace_paths(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                     const srt_triangle *triangles, const srt_material *materials, const float *sky_rgba, int sky_w,
                     int sky_h, const int32_t *pixel_ids, const int32_t *samples, int n, float *out_rgb) {
	scene_t scene = {scene_data, shapes, triangles, materials, sky_rgba, sky_w, sky_h, NULL};
	uint64_t ctr[ORC_C_COUNT];
	memset(ctr, 0, sizeof ctr);
	for (int k = 0; k < n; k++) {
		v3 org, dir;
		uint32_t seed = camera_ray(data, (uint32_t)pixel_ids[k], (uint32_t)samples[k], &org, &dir);
		v3 c = trace(data, &scene, org, dir, seed, ctr);
		out_rgb[3 * k + 0] = c.x;
		out_rgb[3 * k + 1] = c.y;
		out_rgb[3 * k + 2] = c.z;
	}
}

/* The same with albedo textures (tex may be NULL). out_lookups (may be NULL): three counts per path, the texels read at its
 * first hit and at its later hits -- only hits that bounce on read one (the last bounce adds emission alone) -- and the
 * specular bounces among them whose mix(texel, 1, 1) is not 1.0f. */
void orc_trace_paths_textured(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                              const srt_triangle *triangles, const srt_material *materials, const float *sky_rgba, int sky_w,
                              int sky_h, const orc_textures *tex, const int32_t *pixel_ids, const int32_t *samples, int n,
                              float *out_rgb, int32_t *out_lookups) {
	scene_t scene = {scene_data, shapes, triangles, materials, sky_rgba, sky_w, sky_h, tex};
	const int textured = tex != NULL && !data->show_normals;
#pragma omp parallel for schedule(dynamic, 64)
	for (int k = 0; k < n; k++) {
		uint64_t ctr[ORC_C_COUNT] = {0};
		int32_t looks[3] = {0, 0, 0};
		v3 org, dir;
		uint32_t seed = camera_ray(data, (uint32_t)pixel_ids[k], (uint32_t)samples[k], &org, &dir);
		v3 c = textured ? trace_textured(data, &scene, org, dir, seed, ctr, looks) : trace(data, &scene, org, dir, seed, ctr);
		out_rgb[3 * k + 0] = c.x;
		out_rgb[3 * k + 1] = c.y;
		out_rgb[3 * k + 2] = c.z;
		if (out_lookups) out_lookups[3 * k + 0] = looks[0], out_lookups[3 * k + 1] = looks[1], out_lookups[3 * k + 2] = looks[2];
	}
}

/* The primary hit of single (pixel, sample) camera rays, for the denoiser's guide buffers. out: 8 floats per ray:
 * the unit direction, tmin, the front-facing normal (0 without a hit) and the material index (-1: sky, or a shape
 * without a material -- render.cl:404 shades neither). */
void orc_primary_hits(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                      const srt_triangle *triangles, const srt_material *materials, const int32_t *pixel_ids,
                      const int32_t *samples, int n, float *out) {
	scene_t scene = {scene_data, shapes, triangles, materials, NULL, 0, 0, NULL};
	uint64_t ctr[ORC_C_COUNT];
	memset(ctr, 0, sizeof ctr);
	for (int k = 0; k < n; k++) {
		v3 org, dir;
		hit_t hit;
		memset(&hit, 0, sizeof hit);
		(void)camera_ray(data, (uint32_t)pixel_ids[k], (uint32_t)samples[k], &org, &dir);
		int material = closest_intersection(&scene, org, dir, &hit, ctr);
		v3 nrm = material >= 0 ? hit.normal : V(0.f, 0.f, 0.f);
		float *o = out + 8 * (size_t)k;
		o[0] = dir.x, o[1] = dir.y, o[2] = dir.z, o[3] = hit.t;
		o[4] = nrm.x, o[5] = nrm.y, o[6] = nrm.z, o[7] = (float)material;
	}
}

/* ---- what tests/ao_ref.py states the ambient-occlusion pass with (include/srt_abi.h "ambient-occlusion pass"): the statics
 * above under exported names, and the loops above over caller rays. No arithmetic of their own. ---- */
void orc_random_direction(uint32_t *seed, float out[3]) { /* random_direction: the unit vector, *seed advanced by its six draws */
	v3 d = random_direction(seed);
	out[0] = d.x, out[1] = d.y, out[2] = d.z;
}

void orc_normalize3(const float in[3], float out[3]) { /* vnormalize */
	v3 d = vnormalize(V(in[0], in[1], in[2]));
	out[0] = d.x, out[1] = d.y, out[2] = d.z;
}

/* closest_intersection over n caller rays (srt_ray: origin, tmax -- not read --, direction -- used as given --, reserved) ->
 * 8 words per ray: t (+inf: nothing hit), the winner's normal turned to face the ray (0 without a hit), the shape's index and
 * the triangle's inside its model as int32 (-1: none; a shape WITHOUT a material is a hit here, unlike orc_primary_hits'
 * material), 0, 0. */
void orc_closest_hits(const srt_scene_data *scene_data, const srt_shape *shapes, const srt_triangle *triangles,
                      const srt_material *materials, const float *rays, int n, float *out) {
	scene_t scene = {scene_data, shapes, triangles, materials, NULL, 0, 0, NULL};
	uint64_t ctr[ORC_C_COUNT];
	memset(ctr, 0, sizeof ctr);
	for (int k = 0; k < n; k++) {
		const float *r = rays + 8 * (size_t)k;
		hit_t hit;
		memset(&hit, 0, sizeof hit);
		(void)closest_intersection(&scene, V(r[0], r[1], r[2]), V(r[4], r[5], r[6]), &hit, ctr);
		const int found = hit.t < DM_INF_F;
		float *o = out + 8 * (size_t)k;
		int32_t ids[2] = {found ? hit.shape : -1, found && shapes[hit.shape].type == SRT_SHAPE_MODEL ? (int32_t)hit.tri : -1};
		o[0] = hit.t;
		o[1] = found ? hit.normal.x : 0.f, o[2] = found ? hit.normal.y : 0.f, o[3] = found ? hit.normal.z : 0.f;
		memcpy(o + 4, ids, sizeof ids);
		o[6] = o[7] = 0.f;
	}
}

/* The occlusion contract (include/srt_abi.h "occlusion queries") over n caller rays with unit directions: out[k] = 1 when, in
 * array order, a sphere's, a plane's or a triangle's intersector accepts the ray with t < tmax true -- the strict bound;
 * materials are not looked at, so glass and shapes without one occlude --, a model's triangles (world positions made as
 * closest_intersection makes them) only when its box passes orc_intersection_aabb against the ray's tmax. Which rays are
 * valid is the caller's business (tests/ao_ref.py). */
void orc_any_hit(const srt_scene_data *scene_data, const srt_shape *shapes, const srt_triangle *triangles, const float *rays,
                 int n, uint8_t *out) {
	for (int k = 0; k < n; k++) {
		const float *r = rays + 8 * (size_t)k;
		const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]}, tmax = r[3];
		const float inv_dir[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
		int occluded = 0;
		for (int i = 0; i < scene_data->num_shapes && !occluded; i++) {
			const srt_shape *shape = &shapes[i];
			float t_i;
			if (shape->type == SRT_SHAPE_SPHERE) {
				occluded = orc_intersect_sphere(&shape->shape.sphere, o, d, &t_i) && t_i < tmax;
			} else if (shape->type == SRT_SHAPE_PLANE) {
				occluded = orc_intersect_plane(&shape->shape.plane, o, d, &t_i) && t_i < tmax;
			} else if (shape->type == SRT_SHAPE_MODEL) {
				const srt_model *model = &shape->shape.model;
				float bmin[3] = {model->bounding_min.x, model->bounding_min.y, model->bounding_min.z};
				float bmax[3] = {model->bounding_max.x, model->bounding_max.y, model->bounding_max.z};
				if (!orc_intersection_aabb(bmin, bmax, o, inv_dir, tmax)) continue;
				for (size_t j = 0; j < model->num_triangles && !occluded; j++) {
					const srt_triangle *tri = &triangles[model->triangle_index + j];
					v3 p0 = mat_by_vec(model->transform, f3(&tri->vertices[0].pos), 1.0f);
					v3 p1 = mat_by_vec(model->transform, f3(&tri->vertices[1].pos), 1.0f);
					v3 p2 = mat_by_vec(model->transform, f3(&tri->vertices[2].pos), 1.0f);
					occluded = intersect_triangle(p0, p1, p2, V(o[0], o[1], o[2]), V(d[0], d[1], d[2]), &t_i, NULL) && t_i < tmax;
				}
			}
		}
		out[k] = (uint8_t)occluded;
	}
}

/* One dispatch's guide sums, as the denoiser's feature pass adds them (kernels.hip srt_features_kernel): for each pixel
 * its samples 0 .. min(feature_samples, max(num_samples, 0)) - 1 in order, float32 partial sums of {front-facing normal,
 * tmin} and {material colour, 1} over the hits and {1, 1, 1, 0} over the misses, then added into normal_depth and
 * albedo_hits ((h, w, 4) float32 each). */
void orc_features_textured(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                           const srt_triangle *triangles, const srt_material *materials, const orc_textures *tex,
                           int feature_samples, float *normal_depth, float *albedo_hits, int nthreads);

void orc_features(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                  const srt_triangle *triangles, const srt_material *materials, int feature_samples, float *normal_depth,
                  float *albedo_hits, int nthreads) {
	orc_features_textured(data, scene_data, shapes, triangles, materials, NULL, feature_samples, normal_depth, albedo_hits, nthreads);
}

/* The same with albedo textures (tex may be NULL): the albedo of a hit is the texel where its material has one bound.
 * show_normals ignores textures here as in the trace. */
void orc_features_textured(const srt_render_data *data, const srt_scene_data *scene_data, const srt_shape *shapes,
                           const srt_triangle *triangles, const srt_material *materials, const orc_textures *tex,
                           int feature_samples, float *normal_depth, float *albedo_hits, int nthreads) {
	scene_t scene = {scene_data, shapes, triangles, materials, NULL, 0, 0, tex};
	const int textured = tex != NULL && !data->show_normals;
	const int ns = data->num_samples > 0 ? data->num_samples : 0;
	const int fs = feature_samples < ns ? feature_samples : ns;
	const int npix = data->width * data->height;
#ifdef _OPENMP
	if (nthreads > 0) omp_set_num_threads(nthreads);
#else
	(void)nthreads;
#endif
#pragma omp parallel
	{
		uint64_t ctr[ORC_C_COUNT];
		memset(ctr, 0, sizeof ctr);
#pragma omp for schedule(dynamic, 64)
		for (int id = 0; id < npix; id++) {
			v3 nsum = V(0.f, 0.f, 0.f), asum = V(0.f, 0.f, 0.f);
			float tsum = 0.f, hits = 0.f;
			for (int sample = 0; sample < fs; sample++) {
				v3 org, dir;
				hit_t hit;
				memset(&hit, 0, sizeof hit);
				(void)camera_ray(data, (uint32_t)id, (uint32_t)sample, &org, &dir);
				int material = closest_intersection(&scene, org, dir, &hit, ctr);
				if (material >= 0) {
					nsum = vadd(nsum, hit.normal);
					tsum = tsum + hit.t;
					int looked;
					asum = vadd(asum, textured ? albedo(&scene, &hit, material, &looked) : f3(&scene.materials[material].color));
					hits = hits + 1.0f;
				} else {
					asum = vadd(asum, V(1.f, 1.f, 1.f));
				}
			}
			float *nd = normal_depth + 4 * (size_t)id, *ah = albedo_hits + 4 * (size_t)id;
			nd[0] += nsum.x, nd[1] += nsum.y, nd[2] += nsum.z, nd[3] += tsum;
			ah[0] += asum.x, ah[1] += asum.y, ah[2] += asum.z, ah[3] += hits;
		}
	}
}

/* render.cl:473-481 */
static inline float aces1(float x) {
	const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
	return dm_clamp((x * (x * a + b)) / (x * (x * c + d) + e), 0.0f, 1.0f);
}

/* float -> uchar as x86 cvttss2si + truncation does for in-range values; NaN -> 0 */
static inline uint8_t to_uchar(float v) {
	if (!(v == v)) return 0;
	return (uint8_t)(int)v;
}

/* render.cl:525-535 — memory byte order A,R,G,B */
void orc_average(uint32_t num_steps, const float *canvas, uint8_t *output, size_t num_pixels) {
	for (size_t id = 0; id < num_pixels; id++) {
		float n = (float)num_steps;
		float r = dm_sqrtf(aces1(canvas[4 * id + 0] / n));
		float g = dm_sqrtf(aces1(canvas[4 * id + 1] / n));
		float b = dm_sqrtf(aces1(canvas[4 * id + 2] / n));
		output[4 * id + 0] = 255;
		output[4 * id + 1] = to_uchar(r * 255.0f);
		output[4 * id + 2] = to_uchar(g * 255.0f);
		output[4 * id + 3] = to_uchar(b * 255.0f);
	}
}

/* ---- small KAT entry points ------------------------------------------------ */
void orc_matrix_by_vector(const float *m16, const float *v4, float *out4) {
	srt_float4 m[4];
	memcpy(m, m16, sizeof m);
	out4[0] = ((m[0].x * v4[0] + m[1].x * v4[1]) + m[2].x * v4[2]) + m[3].x * v4[3];
	out4[1] = ((m[0].y * v4[0] + m[1].y * v4[1]) + m[2].y * v4[2]) + m[3].y * v4[3];
	out4[2] = ((m[0].z * v4[0] + m[1].z * v4[1]) + m[2].z * v4[2]) + m[3].z * v4[3];
	out4[3] = ((m[0].w * v4[0] + m[1].w * v4[1]) + m[2].w * v4[2]) + m[3].w * v4[3];
}
void orc_barycentric_weights(const float *p0, const float *p1, const float *p2, const float *p, float *out3) {
	v3 w = barycentric_weights(V(p0[0], p0[1], p0[2]), V(p1[0], p1[1], p1[2]), V(p2[0], p2[1], p2[2]), V(p[0], p[1], p[2]));
	out3[0] = w.x;
	out3[1] = w.y;
	out3[2] = w.z;
}
void orc_sky_box(const srt_scene_data *sd, const float *sky, int w, int h, const float *dir, float *out3) {
	scene_t scene = {sd, NULL, NULL, NULL, sky, w, h, NULL};
	v3 c = sky_box(&scene, V(dir[0], dir[1], dir[2]));
	out3[0] = c.x;
	out3[1] = c.y;
	out3[2] = c.z;
}
/* The texture sampler alone: n coordinates (u, v) before the scale -> n x 3 texels. */
void orc_sample_texture(const float *rgba, int w, int h, int filter, float scale_u, float scale_v, const float *u, const float *v,
                        size_t n, float *out_rgb) {
	for (size_t k = 0; k < n; k++) {
		v3 c = sample_texture(rgba, w, h, filter, u[k] * scale_u, v[k] * scale_v);
		out_rgb[3 * k + 0] = c.x, out_rgb[3 * k + 1] = c.y, out_rgb[3 * k + 2] = c.z;
	}
}
void orc_aces(const float *in3, float *out3) {
	for (int k = 0; k < 3; k++) out3[k] = aces1(in3[k]);
}
float orc_cos(float x) { return dm_cosf(x); }
float orc_log(float x) { return dm_logf(x); }
float orc_pow(float x, float y) { return dm_powf(x, y); }
float orc_atan2pi(float y, float x) { return dm_atan2pif(y, x); }
int orc_num_counters(void) { return ORC_C_COUNT; }

/* Host-side twin of the device self-test (srt_selftest_math): sums of result bit
 * patterns of detmath over r = 0, stride, ... ; out[3..7] as in include/srt_abi.h. */
static inline uint64_t canon_bits(float a) { return (a != a) ? 0x7fc00000ull : (uint64_t)dm_f2u(a); }
void orc_math_checksums(uint32_t stride, uint64_t *out8) {
	uint64_t s_log = 0, s_cos = 0, s_sqrt = 0, s_atan = 0, s_pow = 0, s_norm = 0;
	const uint64_t total = (0x100000000ull + stride - 1) / stride;
#pragma omp parallel for reduction(+ : s_log, s_cos, s_sqrt, s_atan, s_pow, s_norm) schedule(static)
	for (uint64_t i = 0; i < total; i++) {
		const uint32_t r = (uint32_t)(i * stride);
		const float u = (float)r / 4294967296.0f;
		const float th = 6.28318548f * u;
		s_log += canon_bits(dm_logf(u));
		s_cos += canon_bits(dm_cosf(th));
		s_sqrt += canon_bits(dm_sqrtf(u));
		s_atan += canon_bits(dm_atan2pif(u - 0.5f, 0.37f - u));
		s_pow += canon_bits(dm_powf(u, 25.0f));
		const v3 nv = vnormalize(V(u - 0.5f, 0.37f - u, (float)(r & 0xffffu) * 1e-3f - 30.0f));
		s_norm += canon_bits(nv.x) + canon_bits(nv.y) + canon_bits(nv.z);
	}
	for (int k = 0; k < 8; k++) out8[k] = 0;
	out8[0] = s_norm; /* compared with out[9] of the device self-test */
	out8[3] = s_log;
	out8[4] = s_cos;
	out8[5] = s_sqrt;
	out8[6] = s_atan;
	out8[7] = s_pow;
}
