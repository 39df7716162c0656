// host_units_check.cpp -- the three host units of csrc/ that need no device, without the library: the BVH builder
// (bvh_host.cpp), the scene's host pass with its hierarchy cache (scene_prep.cpp), the launch plan (trace_plan.h) and the
// denoiser's settings, plans and staging key (denoise_plan.h), the layout of the queries' staging allocation (query_stage.h).
// usage: host_units_check bvh | scene | plan | batches | denoise | stage   (tests/test_host_units.py; scripts/host_asan.sh runs bvh, scene, batches and stage under sanitizers)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "denoise_plan.h"
#include "query_stage.h"
#include "scene_prep.h"
#include "trace_plan.h"

#define CHECK(c, ...)                                             \
	do {                                                          \
		if (!(c)) {                                               \
			fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c); \
			fprintf(stderr, __VA_ARGS__);                         \
			fprintf(stderr, "\n");                                \
			exit(1);                                              \
		}                                                         \
	} while (0)

template <class T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
	return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static srt_triangle triangle(const float p[3][3]) {
	srt_triangle t;
	memset(&t, 0, sizeof t);
	for (int k = 0; k < 3; k++) {
		t.vertices[k].pos.x = p[k][0], t.vertices[k].pos.y = p[k][1], t.vertices[k].pos.z = p[k][2];
		t.vertices[k].normal.z = 1.0f;
	}
	return t;
}

// n triangles of a grid of 1 x 0.75 quads in x and y, heights from a hash of the corner (no symmetry, so no two splits of
// equal cost for rounding to choose between); every coordinate is a multiple of 1/64 and none is zero
static std::vector<srt_triangle> grid_mesh(uint32_t n, uint32_t seed) {
	uint32_t side = 1;
	while (2ull * side * side < n) side++;
	auto height = [seed](uint32_t i, uint32_t j) {
		uint32_t h = (i * 73856093u) ^ (j * 19349663u) ^ (seed * 83492791u);
		h ^= h >> 13, h *= 0x5bd1e995u, h ^= h >> 15;
		return 0.25f + (float)(h & 63u) / 64.0f;
	};
	std::vector<srt_triangle> out;
	for (uint32_t i = 0; i < side && out.size() < n; i++)
		for (uint32_t j = 0; j < side && out.size() < n; j++) {
			const float x0 = 0.5f + (float)i, y0 = 0.5f + 0.75f * (float)j, x1 = x0 + 1.0f, y1 = y0 + 0.75f;
			const float a[3][3] = {{x0, y0, height(i, j)}, {x1, y0, height(i + 1, j)}, {x0, y1, height(i, j + 1)}};
			const float b[3][3] = {{x1, y0, height(i + 1, j)}, {x1, y1, height(i + 1, j + 1)}, {x0, y1, height(i, j + 1)}};
			out.push_back(triangle(a));
			if (out.size() < n) out.push_back(triangle(b));
		}
	return out;
}

static srt_shape model_shape(int material, uint32_t first, uint32_t count, float tx, float ty, float tz, float zero = 0.0f) {
	srt_shape s;
	memset(&s, 0, sizeof s);
	s.type = SRT_SHAPE_MODEL;
	s.material = material;
	srt_model &m = s.shape.model;
	m.triangle_index = first, m.num_triangles = count;
	m.bounding_min = {-1e6f, -1e6f, -1e6f, 0.0f}, m.bounding_max = {1e6f, 1e6f, 1e6f, 0.0f};
	m.transform[0] = {1.0f, zero, zero, zero}, m.transform[1] = {zero, 1.0f, zero, zero}, m.transform[2] = {zero, zero, 1.0f, zero};
	m.transform[3] = {tx, ty, tz, 1.0f};
	return s;
}

// ---- bvh ----------------------------------------------------------------------------------------------------------------------
static void check_bvh(const char *name, const std::vector<srt_triangle> &tris) {
	const uint32_t n = (uint32_t)tris.size();
	const srt_shape shape = model_shape(0, 0, n, 0.0f, 0.0f, 0.0f);
	const srt_model &m = shape.shape.model;
	// the subtrees built by threads of their own (par = 3) against the one-thread build: nodes, order and the whole wide form
	std::vector<BvhNode> nodes[2];
	std::vector<uint32_t> order[2];
	BvhBuilder::Wide wide[2];
	for (int k = 0; k < 2; k++) {
		BvhBuilder bb(nodes[k], order[k]);
		if (k == 0) CHECK(bb.par == 3, "%s: the default is the threaded build", name);
		else bb.par = 0;
		bb.run(m, tris.data(), 0u);
		BvhBuilder::fold_wide(nodes[k], n, false, wide[k]);
	}
	CHECK(same_bytes(nodes[0], nodes[1]), "%s: nodes differ between par = 3 and par = 0", name);
	CHECK(same_bytes(order[0], order[1]), "%s: order differs", name);
	CHECK(same_bytes(wide[0].blocks, wide[1].blocks) && same_bytes(wide[0].dest, wide[1].dest), "%s: wide blocks / dest differ", name);
	CHECK(wide[0].root == wide[1].root && wide[0].need == wide[1].need, "%s: root / need differ", name);
	CHECK(order[0].size() == n && wide[0].dest.size() == n, "%s: %zu records for %u triangles", name, order[0].size(), n);
	// what srt_update_scene keeps per model: within the walk's stack (falling back to the balanced form where the SAH's is not)
	BvhCacheEntry ent;
	ent.build(m, tris.data());
	CHECK(ent.wide.need <= SRT_BVH_STACK_CAP, "%s: need %u", name, ent.wide.need);
	if (!ent.balanced) CHECK(same_bytes(ent.nodes, nodes[0]) && same_bytes(ent.wide.blocks, wide[0].blocks), "%s: the cache entry's build differs", name);
	// a refit under a transform of equal values (-0 for 0: other bytes, what srt_update_scene takes for a move) gives the build's boxes back
	BvhCacheEntry moved = ent;
	const srt_shape shape2 = model_shape(0, 0, n, -0.0f, -0.0f, -0.0f, -0.0f);
	moved.refit(shape2.shape.model, tris.data());
	CHECK(same_bytes(moved.nodes, ent.nodes), "%s: refitted boxes differ from the build's", name);
	CHECK(same_bytes(moved.wide.blocks, ent.wide.blocks) && same_bytes(moved.wide.dest, ent.wide.dest) && moved.wide.need == ent.wide.need, "%s: refitted wide form differs", name);
	printf("bvh %-12s %6u triangles  %6zu nodes  %6zu blocks  need %2u%s\n", name, n, ent.nodes.size(), ent.wide.blocks.size() / 32, ent.wide.need, ent.balanced ? "  balanced" : "");
}

static int mode_bvh() {
	for (uint32_t n : {1u, 3u, 4u, 9u, 8192u, 100000u}) { // the last two: subtrees on threads of their own, the quantiser's too
		char name[32];
		snprintf(name, sizeof name, "grid%u", n);
		check_bvh(name, grid_mesh(n, n));
	}
	std::vector<srt_triangle> same(64, grid_mesh(1, 7)[0]); // coincident centroids: the index split
	check_bvh("coincident", same);
	std::vector<srt_triangle> bad = grid_mesh(9, 5); // non-finite vertices: all-embracing boxes
	bad[2].vertices[1].pos.x = std::numeric_limits<float>::quiet_NaN();
	bad[5].vertices[0].pos.z = std::numeric_limits<float>::infinity();
	bad[7].vertices[2].pos.y = -std::numeric_limits<float>::infinity();
	check_bvh("nonfinite", bad);
	printf("ok\n");
	return 0;
}

// ---- scene --------------------------------------------------------------------------------------------------------------------
struct Scene {
	std::vector<srt_shape> shapes;
	std::vector<srt_triangle> tris;
	std::vector<srt_material> mats;
};

static int prepare(int accel, BvhCache *&cache, const Scene &s, ScenePrep &sp, std::string &err) {
	srt_scene_data sd;
	memset(&sd, 0, sizeof sd);
	AccelPolicy ap;
	ap.accel = accel;
	return prepare_scene(ap, cache, 4096, err, sp, s.shapes.data(), s.shapes.size(), s.tris.data(), s.tris.size(), s.mats.data(), s.mats.size(), &sd);
}

// prepares `s` with the persistent cache, expects (built, reused, refitted), and the arrays of a preparation that starts from nothing
static void step(const char *what, BvhCache *&cache, const Scene &s, uint64_t built, uint64_t reused, uint64_t refitted) {
	ScenePrep sp, ref;
	std::string err;
	CHECK(prepare(SRT_ACCEL_BVH, cache, s, sp, err) == SRT_OK, "%s: %s", what, err.c_str());
	CHECK(sp.bvh_info[4] == built && sp.bvh_info[5] == reused && sp.bvh_info[6] == refitted, "%s: built %llu reused %llu refitted %llu", what,
	      (unsigned long long)sp.bvh_info[4], (unsigned long long)sp.bvh_info[5], (unsigned long long)sp.bvh_info[6]);
	BvhCache *none = nullptr;
	CHECK(prepare(SRT_ACCEL_BVH, none, s, ref, err) == SRT_OK, "%s (fresh cache): %s", what, err.c_str());
	delete none;
	CHECK(ref.bvh_info[4] == built + reused + refitted, "%s: a fresh cache builds every model", what);
	CHECK(same_bytes(sp.data, ref.data) && same_bytes(sp.winners, ref.winners) && same_bytes(sp.offs, ref.offs), "%s: data / winners / offs differ from a fresh preparation", what);
	CHECK(same_bytes(sp.bvh_blocks, ref.bvh_blocks), "%s: bvh_blocks differ from a fresh preparation", what);
	CHECK(same_bytes(sp.bvh_order, ref.bvh_order) && same_bytes(sp.bvh_dest, ref.bvh_dest), "%s: bvh_order / bvh_dest differ from a fresh preparation", what);
	CHECK(same_bytes(sp.dev_mats, ref.dev_mats), "%s: dev_mats differ from a fresh preparation", what);
	printf("scene %-44s built %llu reused %llu refitted %llu\n", what, (unsigned long long)built, (unsigned long long)reused, (unsigned long long)refitted);
}

static int mode_scene() {
	Scene s;
	const std::vector<srt_triangle> small = grid_mesh(12, 3), mesh = grid_mesh(242, 4);
	s.tris = small;
	s.tris.insert(s.tris.end(), mesh.begin(), mesh.end());
	s.mats.resize(2);
	memset(s.mats.data(), 0, 2 * sizeof(srt_material));
	s.mats[0].color = {0.7f, 0.7f, 0.9f, 0.0f}, s.mats[0].refraction_index = 1.0f;
	s.mats[1].color = {0.9f, 0.5f, 0.3f, 0.0f}, s.mats[1].refraction_index = 1.5f, s.mats[1].smoothness = 0.4f, s.mats[1].specular = 0.2f;
	srt_shape plane;
	memset(&plane, 0, sizeof plane);
	plane.type = SRT_SHAPE_PLANE;
	plane.shape.plane.position = {0.0f, -1.2f, 0.0f, 0.0f}, plane.shape.plane.normal = {0.0f, 1.0f, 0.0f, 0.0f};
	s.shapes = {plane, model_shape(1, 12, 242, 64.0f, 64.0f, 64.0f), model_shape(0, 0, 12, 80.0f, 66.0f, 64.5f)};

	BvhCache *cache = nullptr;
	step("1 two models", cache, s, 2, 0, 0);
	step("2 the same scene again", cache, s, 0, 2, 0);
	// Both models moved. A refit keeps the topology the build chose under the FIRST transform, so its arrays are those of a build
	// from nothing only where that build decides every split alike: here both are translations by multiples of 1/4 that leave
	// every coordinate in [64, 128), where float has one spacing -- each box, padded and rounded, moves by exactly the
	// translation, and every comparison the builder makes comes out as before. (A rotated or scaled model, or one that crosses a
	// power of two, is refitted just the same, into boxes around a topology a new build need not choose: no bytes to compare with.)
	Scene moved = s;
	moved.shapes[1] = model_shape(1, 12, 242, 66.0f, 64.5f, 64.25f);
	moved.shapes[2] = model_shape(0, 0, 12, 80.25f, 66.0f, 65.0f);
	step("3 both models moved", cache, moved, 0, 0, 2);
	{ // an array-scan update empties the cache ...
		ScenePrep sp;
		std::string err;
		CHECK(prepare(SRT_ACCEL_NONE, cache, moved, sp, err) == SRT_OK, "array scan: %s", err.c_str());
		CHECK(!sp.use_bvh && sp.bvh_blocks.empty() && sp.bvh_info[4] == 0 && cache && cache->entries.empty(), "array scan: the cache is emptied");
	}
	step("4 after an array-scan update: built again", cache, moved, 2, 0, 0);
	// two instances of one triangle range with equal transforms, told apart by their materials only
	Scene twins = s;
	twins.shapes = {model_shape(0, 12, 242, 70.0f, 64.0f, 64.0f), plane, model_shape(1, 12, 242, 70.0f, 64.0f, 64.0f)};
	{
		ScenePrep sp;
		std::string err;
		CHECK(prepare(SRT_ACCEL_BVH, cache, twins, sp, err) == SRT_OK, "twins: %s", err.c_str());
		CHECK(sp.bvh_info[4] + sp.bvh_info[5] + sp.bvh_info[6] == 2 && cache->entries.size() == 2, "twins: two models");
	}
	Scene swapped = twins;
	std::swap(swapped.shapes[0], swapped.shapes[2]);
	step("5 two instances of one range, swapped", cache, swapped, 0, 2, 0);
	{ // an error behind the models (they have been looked up and claimed by then) keeps every hierarchy
		Scene broken = swapped;
		broken.shapes.push_back(plane);
		broken.shapes.back().material = 99;
		ScenePrep sp;
		std::string err;
		CHECK(prepare(SRT_ACCEL_BVH, cache, broken, sp, err) == SRT_ERR_INVALID, "a bad material index must fail");
		CHECK(err == "srt_update_scene: shape 3 uses material 99 but only 2 exist", "the error text: %s", err.c_str());
		CHECK(cache->entries.size() == 2, "the failed call keeps the cache");
	}
	step("6 after a call that failed: both reused", cache, swapped, 0, 2, 0);
	delete cache;
	printf("ok\n");
	return 0;
}

// ---- plan ---------------------------------------------------------------------------------------------------------------------
// stdin: rows of pixels ns budget scan_tris scan_pairs force_batch num_cus slots has_models bvh_active sub_items items_per_wave cap_subs
// (the four development overrides: 0 = not set); stdout per row: batch halved n_batches radiance_stride scan_waves, then
// nbs job_items num_waves nbs_magic16 of the first and of the last launch (zeros when there is none)
static int mode_plan() {
	long long v[13];
	for (;;) {
		for (int k = 0; k < 13; k++)
			if (scanf("%lld", &v[k]) != 1) return k == 0 ? 0 : 1;
		const size_t pixels = (size_t)v[0];
		const int ns = (int)v[1];
		const uint32_t batch = plan_batch(pixels, ns, (size_t)v[2], (uint64_t)v[3], (double)v[4], (int)v[5]);
		const uint32_t n_batches = plan_num_batches(ns, batch);
		printf("%u %u %u %zu %zu", batch, plan_batch_halved(batch), n_batches, plan_radiance_stride(pixels, batch), plan_scan_waves((int)v[7], pixels, batch));
		for (int last = 0; last < 2; last++) {
			if (n_batches == 0) {
				printf(" 0 0 0 0");
				continue;
			}
			const uint32_t s0 = last ? (n_batches - 1) * batch : 0u;
			const uint32_t nbs = (uint32_t)ns - s0 < batch ? (uint32_t)ns - s0 : batch;
			const LaunchPlan lp = plan_launch((unsigned long long)pixels * nbs, nbs, (unsigned long long)v[10], (int)v[6], (int)v[7], v[8] != 0, v[9] != 0, (int)v[11], (int)v[12]);
			printf(" %u %u %d %u", nbs, lp.job_items, lp.num_waves, lp.nbs_magic16);
		}
		printf("\n");
	}
}

// ---- batches ------------------------------------------------------------------------------------------------------------------
// plan_batch_slice over every batch of a dispatch: the slices tile [0, ns) once and in order, parities alternate only when there
// is more than one batch, total_items = pixels x samples. Returns the number of batches; *first and *last = those slices.
static uint32_t check_batches(size_t pixels, int ns, uint32_t batch, BatchSlice *first, BatchSlice *last) {
	const uint32_t n_batches = plan_num_batches(ns, batch);
	CHECK((n_batches == 0) == (ns <= 0 || batch == 0), "pixels %zu ns %d batch %u: %u batches", pixels, ns, batch, n_batches);
	uint32_t next = 0;
	int previous_parity = 1; // (the first batch takes set 0)
	for (uint32_t b = 0; b < n_batches; b++) {
		const BatchSlice bs = plan_batch_slice(b, n_batches, pixels, ns, batch);
		CHECK(bs.first_sample == next, "batch %u of %u starts at sample %u, the one before ended at %u", b, n_batches, bs.first_sample, next);
		CHECK(bs.samples >= 1 && bs.samples <= batch, "batch %u holds %u samples of at most %u", b, bs.samples, batch);
		CHECK(b == n_batches - 1 || bs.samples == batch, "batch %u of %u is ragged (%u of %u) but not the last", b, n_batches, bs.samples, batch);
		CHECK(bs.parity == 0 || bs.parity == 1, "batch %u of %u has parity %d", b, n_batches, bs.parity);
		CHECK(b == 0 ? bs.parity == 0 : bs.parity != previous_parity, "batch %u of %u has parity %d after %d", b, n_batches, bs.parity, previous_parity);
		previous_parity = bs.parity;
		CHECK(bs.total_items == (unsigned long long)pixels * bs.samples, "batch %u: %llu items for %zu pixels x %u samples", b, bs.total_items, pixels, bs.samples);
		next = bs.first_sample + bs.samples;
		if (b == 0) *first = bs;
		*last = bs;
	}
	CHECK(next == (ns > 0 ? (uint32_t)ns : 0u), "pixels %zu ns %d batch %u: the batches end at sample %u", pixels, ns, batch, next);
	return n_batches;
}

// the cases every run checks, then stdin: rows of pixels ns batch; stdout per such row: n_batches, then parity first_sample
// samples of the first and of the last batch (zeros when there is none); "ok" at the end
static int mode_batches() {
	BatchSlice first, last;
	CHECK(check_batches(1200, 5, 2, &first, &last) == 3 && last.first_sample == 4 && last.samples == 1 && last.parity == 0, "5 samples in batches of 2: 2, 2, 1");
	CHECK(check_batches(1200, 5, 5, &first, &last) == 1 && first.parity == 0 && first.samples == 5, "5 samples in one batch: set 0");
	CHECK(check_batches(1200, 5, 1, &first, &last) == 5 && last.parity == 0, "5 samples one by one");
	CHECK(check_batches(1200, 0, 0, &first, &last) == 0 && check_batches(1200, -3, 0, &first, &last) == 0, "no samples: no batch");
	CHECK(check_batches(0, 4, 4, &first, &last) == 1 && first.total_items == 0, "a handle without rows: one launch of no items");
	long long v[3];
	for (;;) {
		for (int k = 0; k < 3; k++)
			if (scanf("%lld", &v[k]) != 1) {
				if (k == 0) printf("ok\n");
				return k == 0 ? 0 : 1;
			}
		memset(&first, 0, sizeof first), memset(&last, 0, sizeof last);
		const uint32_t n_batches = check_batches((size_t)v[0], (int)v[1], (uint32_t)v[2], &first, &last);
		printf("%u %d %u %u %d %u %u\n", n_batches, first.parity, first.first_sample, first.samples, last.parity, last.first_sample, last.samples);
	}
}

// ---- denoise ------------------------------------------------------------------------------------------------------------------
// One row per point of the lattice K x demod x sv_min x temporal x illum x gamma x feedback x history_valid x any_moved x
// any_deformed x vertex_motion (object motion on throughout; the sigmas and thresholds fixed): the point, then plan_filter (K
// demod spatial_var feedback inv_sigma_a2), plan_setup (motion_level illum clamp) and the staging key's fields as one word.
// Then operator== over every ordered pair against equality of those words, the cascades, and "ok".
static std::string key_word(const StagingKey &k) {
	char b[256];
	snprintf(b, sizeof b, "%llu/%d%d%d%d%d/%d/%d/%u/%a/%a/%a/%a/%a/%a/%a", (unsigned long long)k.serial, k.history_valid, k.illum, k.feedback, k.demod, k.pass1_last,
	         k.history_limit, k.motion_level, k.sv_min, k.normal_threshold, k.depth_threshold, k.clamp_gamma, k.sigma_l, k.sigma_n, k.sigma_z, k.inv_sigma_a2);
	return b;
}

static DenoiseSettings all_on() {
	DenoiseSettings s;
	s.on = s.demod = s.temporal = s.illum = s.feedback = s.object_motion = s.vertex_motion = true;
	s.p.iterations = 3, s.p.feature_samples = 2, s.p.sigma_luminance = 4.0f, s.p.sigma_normal = 128.0f, s.p.sigma_depth = 1.0f, s.p.sigma_albedo = 0.1f;
	s.sv_min = 8;
	s.tp.history_limit = 32, s.tp.normal_threshold = 0.9f, s.tp.depth_threshold = 0.05f;
	s.clamp_gamma = 1.0f;
	return s;
}

static int mode_denoise() {
	std::vector<StagingKey> keys;
	std::vector<std::string> words;
	for (int K : {0, 1, 3})
		for (int bits = 0; bits < 512; bits++)
			for (float gamma : {0.0f, 1.0f, 2.0f}) {
				DenoiseSettings s = all_on();
				s.p.iterations = K;
				s.demod = bits & 1, s.sv_min = bits & 2 ? 8 : 0, s.temporal = bits & 4, s.illum = bits & 8, s.feedback = bits & 16;
				s.clamp_gamma = gamma;
				const bool valid = bits & 32, moved = bits & 64, deformed = bits & 128;
				s.vertex_motion = bits & 256;
				const FilterPlan f = plan_filter(s);
				const SetupPlan u = plan_setup(s, valid, moved, deformed);
				keys.push_back(staging_key(s, valid, moved, deformed, 7));
				words.push_back(key_word(keys.back()));
				printf("%d %d %u %d %d %g %d %d %d %d %d  %d %d %d %d %a  %d %d %d  %s\n", K, s.demod, s.sv_min, s.temporal, s.illum, gamma, s.feedback, valid, moved, deformed,
				       s.vertex_motion, f.K, f.demod, f.spatial_var, f.feedback, f.inv_sigma_a2, u.motion_level, u.illum, u.clamp, words.back().c_str());
			}
	for (size_t a = 0; a < keys.size(); a++)
		for (size_t b = 0; b < keys.size(); b++)
			CHECK((keys[a] == keys[b]) == (words[a] == words[b]), "operator== and the printed fields disagree for rows %zu and %zu", a, b);
	StagingKey other = keys[0];
	other.serial++;
	CHECK(!(other == keys[0]), "another serial is another key");
	// a tiny sigma_albedo: the square underflows in float; the inverse is clamped, not inf
	DenoiseSettings tiny = all_on();
	tiny.p.sigma_albedo = 1e-30f;
	CHECK(plan_filter(tiny).inv_sigma_a2 == FLT_MAX, "inv_sigma_a2 %a", plan_filter(tiny).inv_sigma_a2);
	// the cascades: what is a mode of a stage goes off with it; the parameters and what is not stay
	const DenoiseSettings fresh;
	DenoiseSettings s = all_on();
	s.temporal_off();
	CHECK(s.temporal == fresh.temporal && s.illum == fresh.illum && s.clamp_gamma == fresh.clamp_gamma && s.feedback == fresh.feedback &&
	      s.object_motion == fresh.object_motion && s.vertex_motion == fresh.vertex_motion, "temporal_off leaves a mode of the temporal stage on");
	CHECK(s.on && s.demod && s.sv_min == 8 && s.p.iterations == 3 && s.tp.history_limit == 32, "temporal_off touches the filter's settings or the parameters");
	s = all_on();
	s.off();
	CHECK(s.on == fresh.on && s.demod == fresh.demod && s.sv_min == fresh.sv_min && s.temporal == fresh.temporal && s.illum == fresh.illum &&
	      s.clamp_gamma == fresh.clamp_gamma && s.feedback == fresh.feedback && s.object_motion == fresh.object_motion && s.vertex_motion == fresh.vertex_motion,
	      "off leaves a switch on");
	printf("ok\n");
	return 0;
}

// ---- stage --------------------------------------------------------------------------------------------------------------------
// query_stage.h for the counts at which something changes (one item, around one and two mask words) and the largest a call
// accepts: per call of include/srt_abi.h the regions it uses together and the bytes it moves through each (srt_ray,
// srt_ray_hit and srt_segment are 32 bytes, a picked point 8, a mask ceil(n / 64) words of 8), alignment as the kernels' 128-bit
// and 64-bit accesses need it, and a total within what the two formulas before the shared layout reserved.
struct StageRegion {
	const char *name;
	size_t at, bytes, align;
};

static int mode_stage() {
	for (const size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)129, ((size_t)1 << 31) - 1}) {
		const QueryStage s = query_stage(n);
		const size_t words = (n + 63) / 64;
		CHECK(query_mask_words(n) == words, "n %zu: %zu mask words", n, query_mask_words(n));
		const StageRegion rays = {"rays", s.rays, 32 * n, 16}, hits = {"hits", s.hits, 32 * n, 16}, segs = {"segs", s.segs, 32 * n, 16};
		const StageRegion xy = {"xy", s.xy, 8 * n, 8}, occluded = {"occluded", s.occluded, 8 * words, 8}, invalid = {"invalid", s.invalid, 8 * words, 8};
		const std::vector<std::pair<const char *, std::vector<StageRegion>>> calls = {
		    {"srt_cast_rays", {rays, hits}},
		    {"srt_pick", {xy, rays, hits}},
		    {"srt_occluded_rays", {rays, occluded, invalid}},
		    {"srt_occluded_segments", {segs, rays, occluded, invalid}},
		    {"srt_segment_rays", {segs, rays}},
		};
		for (const auto &call : calls) {
			const std::vector<StageRegion> &rs = call.second;
			for (size_t a = 0; a < rs.size(); a++) {
				CHECK(rs[a].at % rs[a].align == 0, "n %zu, %s: %s at %zu is not aligned to %zu", n, call.first, rs[a].name, rs[a].at, rs[a].align);
				CHECK(rs[a].at + rs[a].bytes <= s.total, "n %zu, %s: %s ends at %zu of %zu", n, call.first, rs[a].name, rs[a].at + rs[a].bytes, s.total);
				for (size_t b = a + 1; b < rs.size(); b++)
					CHECK(rs[a].at + rs[a].bytes <= rs[b].at || rs[b].at + rs[b].bytes <= rs[a].at, "n %zu, %s: %s and %s overlap", n, call.first, rs[a].name, rs[b].name);
			}
		}
		const size_t cast = n * 72, occlusion = n * 64 + 16 * words;
		CHECK(s.total <= (cast > occlusion ? cast : occlusion), "n %zu: %zu bytes, more than the %zu / %zu of the separate layouts", n, s.total, cast, occlusion);
		printf("stage n %10zu  total %12zu\n", n, s.total);
	}
	printf("ok\n");
	return 0;
}

int main(int argc, char **argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "bvh") return mode_bvh();
	if (mode == "scene") return mode_scene();
	if (mode == "plan") return mode_plan();
	if (mode == "batches") return mode_batches();
	if (mode == "denoise") return mode_denoise();
	if (mode == "stage") return mode_stage();
	fprintf(stderr, "usage: %s bvh | scene | plan | batches | denoise | stage\n", argv[0]);
	return 2;
}
