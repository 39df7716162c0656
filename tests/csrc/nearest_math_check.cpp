// nearest_math_check.cpp -- csrc/nearest_math.h by itself, built with plain g++ (no HIP, no library): the distance functions of
// the nearest-surface queries (include/srt_abi.h) on their edge cases. May be built with -fsanitize=address,undefined and run
// directly.
// usage: nearest_math_check self   the directed cases below, checked against what the header states; prints "ok"
//        nearest_math_check eval   stdin: one case per line, `t|s|p` and 12 / 7 / 9 words of float bits in hex (triangle: the
//                                  world record and q; sphere: centre, radius, q; plane: position, normal, q); stdout: the bits of
//                                  distance, point and flags per line (tests/test_nearest_reference.py compares them with
//                                  tests/nearest_ref.py and with the library's host exports)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "nearest_math.h"

#define CHECK(c, ...)                                             \
	do {                                                          \
		if (!(c)) {                                               \
			fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); \
			fprintf(stderr, __VA_ARGS__);                         \
			fprintf(stderr, "\n");                                \
			exit(1);                                              \
		}                                                         \
	} while (0)

static nm_result tri(const float *w, float x, float y, float z) { return nm_triangle(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], x, y, z); }
static unsigned feature(const nm_result &r) { return (r.flags >> NM_FEATURE_SHIFT) & 7u; }
static bool back(const nm_result &r) { return (r.flags & NM_BACK) != 0u; }

static int mode_self() {
	// a right triangle in z = 1: v0 = (1, 1, 1), v1 = (3, 1, 1), v2 = (1, 2, 1); cross(e1, e2) = (0, 0, 2): front is +z
	const float w[9] = {1, 1, 1, 2, 0, 0, 0, 1, 0};
	struct {
		float q[3];
		unsigned feature;
		float p[3];
	} const at[] = {
	    {{1, 1, 1}, 1, {1, 1, 1}},          {{3, 1, 1}, 2, {3, 1, 1}},        {{1, 2, 1}, 3, {1, 2, 1}},      // the vertices themselves
	    {{0, 0, 1}, 1, {1, 1, 1}},          {{5, 0.5f, 1}, 2, {3, 1, 1}},     {{0.5f, 4, 1}, 3, {1, 2, 1}},   // beyond them, in the plane
	    {{2, 1, 1}, 4, {2, 1, 1}},          {{1, 1.5f, 1}, 5, {1, 1.5f, 1}},  {{2, 1.5f, 1}, 6, {2, 1.5f, 1}}, // edge midpoints
	    {{2, 0, 3}, 4, {2, 1, 1}},          {{0, 1.5f, -2}, 5, {1, 1.5f, 1}},                                  // off the edges
	    {{1.5f, 1.25f, 1}, 0, {1.5f, 1.25f, 1}}, {{1.5f, 1.25f, 4}, 0, {1.5f, 1.25f, 1}}, {{1.5f, 1.25f, -4}, 0, {1.5f, 1.25f, 1}}, // the face
	};
	for (const auto &c : at) {
		const nm_result r = tri(w, c.q[0], c.q[1], c.q[2]);
		CHECK(feature(r) == c.feature, "q %g %g %g: feature %u, expected %u", c.q[0], c.q[1], c.q[2], feature(r), c.feature);
		CHECK(r.px == c.p[0] && r.py == c.p[1] && r.pz == c.p[2], "q %g %g %g: point %g %g %g", c.q[0], c.q[1], c.q[2], r.px, r.py, r.pz);
		const double dx = c.q[0] - c.p[0], dy = c.q[1] - c.p[1], dz = c.q[2] - c.p[2];
		CHECK(std::fabs(r.distance - std::sqrt(dx * dx + dy * dy + dz * dz)) <= 1e-6, "q %g %g %g: distance %g", c.q[0], c.q[1], c.q[2], r.distance);
		CHECK(back(r) == (c.q[2] < 1.0f), "q %g %g %g: back %d", c.q[0], c.q[1], c.q[2], (int)back(r));
	}
	// far away: 10^3 and 10^4 triangle sizes; the distance stays within a few ulps of the exact one
	for (const float far : {2.0e3f, 2.0e4f}) {
		const nm_result r = tri(w, far, far, far);
		const double ex = std::sqrt((far - 3.0) * (far - 3.0) + (far - 1.0) * (far - 1.0) + (far - 1.0) * (far - 1.0)); // nearest: v1 or the edge v1v2
		CHECK(std::isfinite(r.distance) && r.distance > 0.0f && std::fabs(r.distance - ex) <= 0.25 * far, "far %g: distance %g", far, r.distance);
	}
	// fully degenerate (e1 = e2 = 0): the vertex v0
	const float point_tri[9] = {4, 5, 6, 0, 0, 0, 0, 0, 0};
	nm_result r = tri(point_tri, 4, 5, 9);
	CHECK(feature(r) == 1u && r.distance == 3.0f && r.px == 4 && r.py == 5 && r.pz == 6, "degenerate: %g", r.distance);
	// the all-zero padding triangle is a point at the origin: callers must leave it out by count
	const float zero_tri[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	r = tri(zero_tri, 0, 0, 0);
	CHECK(r.distance == 0.0f, "padding triangle: %g", r.distance);
	// collinear: whatever region the arithmetic takes, the result is a point of the segment or a NaN, never garbage
	const float line_tri[9] = {0, 0, 0, 1, 0, 0, 2, 0, 0};
	for (const float x : {-1.0f, 0.5f, 1.5f, 3.0f}) {
		r = tri(line_tri, x, 1, 0);
		CHECK(std::isnan(r.distance) || (r.distance >= 1.0f && r.distance < 1.5f && r.py == 0.0f && r.px >= 0.0f && r.px <= 2.0f), "collinear x %g: %g at %g", x, r.distance, r.px);
	}
	// a NaN or an infinity in the record: runs through (the sanitizers watch), a NaN distance is the caller's "never taken"
	for (int k = 0; k < 9; k++) {
		float bad[9];
		memcpy(bad, w, sizeof bad);
		bad[k] = NAN;
		r = tri(bad, 1.5f, 1.25f, 2);
		CHECK(std::isnan(r.distance) || r.distance >= 0.0f, "NaN in %d", k);
		bad[k] = INFINITY;
		r = tri(bad, 1.5f, 1.25f, 2);
		CHECK(std::isnan(r.distance) || r.distance >= 0.0f, "inf in %d", k);
	}
	// spheres: outside, inside, on the surface (len == r), at the centre, a negative radius
	r = nm_sphere(1, 2, 3, 2, 1, 2, 8);
	CHECK(r.distance == 3.0f && !back(r) && r.px == 1 && r.py == 2 && r.pz == 5, "sphere outside: %g", r.distance);
	r = nm_sphere(1, 2, 3, 2, 1, 2, 4);
	CHECK(r.distance == 1.0f && back(r) && r.pz == 5, "sphere inside: %g", r.distance);
	r = nm_sphere(1, 2, 3, 2, 1, 4, 3);
	CHECK(r.distance == 0.0f && !back(r) && r.py == 4, "sphere surface: %g", r.distance);
	r = nm_sphere(1, 2, 3, 2, 1, 2, 3);
	CHECK(r.distance == 2.0f && back(r) && r.px == 3 && r.py == 2 && r.pz == 3, "sphere centre: %g at %g", r.distance, r.px);
	r = nm_sphere(1, 2, 3, -2, 1, 2, 8);
	CHECK(r.distance == 3.0f && r.pz == 5, "negative radius: %g", r.distance);
	// planes: a non-unit normal, below the plane, a zero normal
	r = nm_plane(0, 1, 0, 0, 4, 0, 3, 6, -2);
	CHECK(r.distance == 5.0f && !back(r) && r.px == 3 && r.py == 1 && r.pz == -2, "plane: %g at %g", r.distance, r.py);
	r = nm_plane(0, 1, 0, 0, 4, 0, 3, -1, -2);
	CHECK(r.distance == 2.0f && back(r) && r.py == 1, "plane below: %g", r.distance);
	r = nm_plane(0, 1, 0, 0, 0, 0, 3, 6, -2);
	CHECK(std::isnan(r.distance), "zero normal: %g", r.distance);
	r = nm_plane(0, 1, 0, 0, INFINITY, 0, 3, 6, -2);
	CHECK(std::isnan(r.distance), "infinite normal: %g", r.distance);
	printf("ok\n");
	return 0;
}

static int mode_eval() {
	char kind;
	while (scanf(" %c", &kind) == 1) {
		const int n = kind == 't' ? 12 : kind == 's' ? 7 : kind == 'p' ? 9 : 0;
		if (!n) return 2;
		float a[12];
		for (int k = 0; k < n; k++) {
			unsigned u;
			if (scanf("%x", &u) != 1) return 2;
			a[k] = dm_u2f(u);
		}
		const nm_result r = kind == 't'   ? nm_triangle(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11])
		                    : kind == 's' ? nm_sphere(a[0], a[1], a[2], a[3], a[4], a[5], a[6])
		                                  : nm_plane(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
		printf("%08x %08x %08x %08x %08x\n", dm_f2u(r.distance), dm_f2u(r.px), dm_f2u(r.py), dm_f2u(r.pz), r.flags);
	}
	return 0;
}

int main(int argc, char **argv) {
	if (argc == 2 && !strcmp(argv[1], "self")) return mode_self();
	if (argc == 2 && !strcmp(argv[1], "eval")) return mode_eval();
	fprintf(stderr, "usage: nearest_math_check self | eval\n");
	return 2;
}
