// scene_prep.cpp -- the host pass of srt_update_scene (scene_prep.h) and the material thresholds. Standard library only.
#include "scene_prep.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <utility>

// bernoulli() thresholds (device_math.h): T(p) = how many of the generator's 2^32 outputs r give p > (float)r * 2^-32 -- a prefix,
// the conversion is monotone. 0 for p <= 0 and NaN, 2^32 for p > 1; p = 1 gives 2^32 - 128 (the 128 largest r convert to 1.0).
// THE one copy: srt_update_scene and srt_bernoulli_threshold_host both call it.
uint64_t bernoulli_threshold(float pr) {
	uint64_t lo = 0, hi = (uint64_t)1 << 32; // first r in [lo, hi] for which !(pr > u(r)); hi = 2^32: none
	while (lo < hi) {
		const uint64_t mid = (lo + hi) >> 1;
		const float u = (float)(uint32_t)mid * 2.3283064365386963e-10f;
		if (pr > u) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// Axis planes (device_types.h "Axis planes"): 1, 2, 3 for a plane whose normal is +-e_x, +-e_y, +-e_z -- exactly one component
// equal to +1 or -1, the other two zeros of either sign -- and whose position is at most 2^100 in every component; 0 for every
// other plane (any other length, a denormal or a NaN anywhere). The position's clause is the twin's, not the identity's: its
// guard sees, of a plane's position, only the component on the axis; a position that is not finite in another component puts
// 0 * NaN into the reference's numerator, and one near FLT_MAX can overflow the difference to the origin. With |p| <= 2^100 and
// the origin within 2^50 of every axis's plane (the guard; the planes of a buildable pattern use all three axes) no difference
// does. THE one copy: srt_update_scene and srt_plane_axis_code_host both call it.
int srt_plane_axis_code(const float n[3], const float p[3]) {
	int axis = 0;
	for (int k = 0; k < 3; k++) {
		if (!(fabsf(p[k]) <= 0x1p100f)) return 0; // (a NaN fails)
		if (n[k] == 0.0f) continue;               // +0 or -0
		if (fabsf(n[k]) != 1.0f || axis != 0) return 0;
		axis = k + 1;
	}
	return axis;
}

// host pass; `cache` is made when a BVH scene first needs it and emptied by an array-scan scene; an error return leaves its text
// in `err` and every cached hierarchy in place
int prepare_scene(const AccelPolicy &policy, BvhCache *&cache, int scan_suspend_min, std::string &err, ScenePrep &sp, const srt_shape *shapes, size_t n_shapes,
                  const srt_triangle *triangles, size_t n_triangles, const srt_material *materials, size_t n_materials, const srt_scene_data *scene) {
	auto fail = [&err](int code, const char *msg) {
		err = msg;
		return code;
	};
	if (!scene) return fail(SRT_ERR_INVALID, "srt_update_scene: scene is NULL");
	if ((n_shapes && !shapes) || (n_triangles && !triangles) || (n_materials && !materials))
		return fail(SRT_ERR_INVALID, "srt_update_scene: NULL array with non-zero count");
	if (n_shapes > 0x7fffffffu || n_triangles > 0xffffffffu) return fail(SRT_ERR_INVALID, "srt_update_scene: too many records");

	// Host pass: runs of same-type shapes in array order, their packed scalar-load records,
	// per-shape winner records and world-triangle offsets. The reference would read out of
	// bounds for a bad triangle range or material index; we refuse instead.
	std::vector<ShapeRun> runs;
	std::vector<float> &data = sp.data; // packed, every run starts on a 16-dword boundary
	std::vector<WinnerRec> &winners = sp.winners;
	winners.assign(n_shapes ? n_shapes : 1, WinnerRec());
	std::vector<uint32_t> &offs = sp.offs;
	offs.assign(n_shapes ? n_shapes : 1, 0u);
	uint64_t &total_wtris = sp.total_wtris, &max_tris = sp.max_tris;
	int &num_models = sp.num_models;
	const bool use_bvh = sp.use_bvh = policy.accel == SRT_ACCEL_BVH;
	std::vector<uint32_t> &bvh_blocks = sp.bvh_blocks; // 32 dwords each (device_types.h)
	std::vector<uint32_t> &bvh_order = sp.bvh_order, &bvh_dest = sp.bvh_dest;
	uint64_t bvh_leaves = 0, bvh_depth = 0, bvh_reused = 0, bvh_refitted = 0, bvh_canonical_nodes = 0;
	std::deque<BvhCacheEntry> fresh;                 // hierarchies built by this call (deque: growth keeps references valid)
	std::vector<std::pair<bool, size_t>> plan;       // per model with triangles: {from the cache?, index there / in fresh}
	std::vector<std::pair<uint64_t, uint64_t>> range_hashes; // {triangle_index << 32 | count, hash}
	std::vector<std::pair<const BvhCacheEntry *, uint32_t>> stale_plan; // the models the device refits: {hierarchy, its first block}
	if (use_bvh && !cache) cache = new BvhCache();
	if (cache)
		for (BvhCacheEntry &e : cache->entries) e.claimed = false;
	if (!use_bvh && cache) cache->entries.clear();
	const auto build_t0 = std::chrono::steady_clock::now();
	// hash of a model's triangle range, once per distinct range per call (instances share ranges)
	auto range_hash = [&](const srt_model &m) {
		for (const auto &rh : range_hashes)
			if (rh.first == (((uint64_t)m.triangle_index << 32) | m.num_triangles)) return rh.second;
		const uint64_t th = hash_triangles(triangles + m.triangle_index, m.num_triangles);
		range_hashes.emplace_back(((uint64_t)m.triangle_index << 32) | m.num_triangles, th);
		return th;
	};
	// An unclaimed entry of the previous call with the same triangles: one with the model's transform if there is one. Hash and
	// transform are compared before any memcmp.
	auto find_same_triangles = [&](const srt_model &m, uint64_t th) {
		BvhCacheEntry *kept = nullptr;
		for (BvhCacheEntry &e : cache->entries) {
			if (e.claimed || e.count != m.num_triangles || e.tri_hash != th) continue;
			const bool exact = e.same_transform(m);
			if (!exact && kept) continue; // already holding a refit candidate: only an exact match improves on it
			if (!e.same_triangles(m, triangles, th)) continue;
			kept = &e;
			if (exact) break;
		}
		return kept;
	};
	// SRT_DEFORM_REFIT: every model's entry is chosen before the shape loop. First the models that find their own triangle bytes,
	// in array order, exactly as the loop would choose; then, among the entries nobody claimed, the models whose bytes changed
	// take one of the same triangle range (index and count) -- so a deformed model never takes what a later one matches byte
	// for byte. (Models the loop is going to refuse are left out here.)
	const bool deform_on = use_bvh && policy.deform.mode == SRT_DEFORM_REFIT;
	struct Match {
		BvhCacheEntry *ent = nullptr;
		bool deformed = false;
	};
	std::vector<Match> matched;
	uint64_t deform_kept = 0, deform_rebuilt = 0;
	if (deform_on) {
		matched.assign(n_shapes, Match());
		auto wants_entry = [&](size_t i) {
			const srt_model &m = shapes[i].shape.model;
			return shapes[i].type == SRT_SHAPE_MODEL && m.num_triangles > 0 && (uint64_t)m.triangle_index + m.num_triangles <= n_triangles;
		};
		for (size_t i = 0; i < n_shapes; i++) {
			if (!wants_entry(i)) continue;
			const srt_model &m = shapes[i].shape.model;
			if ((matched[i].ent = find_same_triangles(m, range_hash(m)))) matched[i].ent->claimed = true;
		}
		for (size_t i = 0; i < n_shapes; i++) {
			if (!wants_entry(i) || matched[i].ent) continue;
			const srt_model &m = shapes[i].shape.model;
			BvhCacheEntry *kept = nullptr;
			for (BvhCacheEntry &e : cache->entries) {
				if (e.claimed || e.count != m.num_triangles || e.triangle_index != m.triangle_index) continue;
				if (!kept || e.same_transform(m)) kept = &e;
				if (e.same_transform(m)) break;
			}
			if (kept) kept->claimed = true, matched[i].ent = kept, matched[i].deformed = true;
		}
	}
	auto u2f = [](uint32_t u) {
		float f;
		memcpy(&f, &u, 4);
		return f;
	};
	// The kernel walks 64-byte BLOCKS of same-type shapes in array order (device_types.h ShapeRun): four spheres,
	// two planes or two models each, block b at dword 16 * b. A block that is not full is
	// filled up with records that can never be hit (r*r = -inf makes the discriminant -inf or NaN; a zero plane
	// normal makes denom == 0, render.cl:209-211).
	auto pad_run = [&]() {
		if (!runs.empty() && runs.back().type == SRT_SHAPE_SPHERE)
			while (data.size() % 16) data.insert(data.end(), {0.0f, 0.0f, 0.0f, -INFINITY});
		while (data.size() % 16) data.push_back(0.0f);
	};
	for (size_t i = 0; i < n_shapes; i++) {
		const srt_shape &s = shapes[i];
		WinnerRec &wr = winners[i];
		memset(&wr, 0, sizeof wr);
		wr.type = s.type;
		wr.material = s.material;
		if (s.material >= 0 && (size_t)s.material >= n_materials) {
			char buf[128];
			snprintf(buf, sizeof buf, "srt_update_scene: shape %zu uses material %d but only %zu exist", i, s.material, n_materials);
			return fail(SRT_ERR_INVALID, buf);
		}
		if (s.type != SRT_SHAPE_SPHERE && s.type != SRT_SHAPE_PLANE && s.type != SRT_SHAPE_MODEL) continue; // ignored, as render.cl:301-366
		const uint32_t block_cap = s.type == SRT_SHAPE_SPHERE ? 4u : 2u;
		// array scan: a big model sits alone in its block (data_off's top bit marks the block until the headers are built)
		const bool big_model = !use_bvh && s.type == SRT_SHAPE_MODEL && s.shape.model.num_triangles >= (uint32_t)scan_suspend_min;
		const bool prev_big = !runs.empty() && (runs.back().data_off >> 31);
		if (runs.empty() || runs.back().type != s.type || runs.back().first_shape + runs.back().count != i || runs.back().count == block_cap || big_model || prev_big) {
			pad_run();
			ShapeRun r;
			r.type = s.type;
			r.first_shape = (uint32_t)i;
			r.count = 0;
			r.data_off = (uint32_t)data.size() | (big_model ? 0x80000000u : 0u); // = 16 * block number
			runs.push_back(r);
		}
		runs.back().count++;
		if (s.type == SRT_SHAPE_SPHERE) {
			const srt_sphere &sp = s.shape.sphere;
			data.insert(data.end(), {sp.position.x, sp.position.y, sp.position.z, sp.radius * sp.radius}); // r*r as render.cl:187
			wr.vx = sp.position.x, wr.vy = sp.position.y, wr.vz = sp.position.z, wr.w = sp.radius;
			{
				const float ar = fabsf(sp.radius);
				wr.inv_w = (ar >= 0x1p-40f && ar <= 0x1p40f) ? 1.0f / sp.radius : 0.0f; // (a NaN radius fails both compares)
			}
		} else if (s.type == SRT_SHAPE_PLANE) {
			const srt_plane &pl = s.shape.plane;
			data.insert(data.end(), {pl.position.x, pl.position.y, pl.position.z, 0.0f, pl.normal.x, pl.normal.y, pl.normal.z, 0.0f});
			wr.vx = pl.normal.x, wr.vy = pl.normal.y, wr.vz = pl.normal.z;
		} else {
			const srt_model &m = s.shape.model;
			if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles) {
				char buf[160];
				snprintf(buf, sizeof buf, "srt_update_scene: shape %zu references triangles [%u, %u+%u) but only %zu exist", i,
				         m.triangle_index, m.triangle_index, m.num_triangles, n_triangles);
				return fail(SRT_ERR_INVALID, buf);
			}
			if (total_wtris + m.num_triangles > (use_bvh ? 0x0fffffffull : 0xffffffffull))
				return fail(SRT_ERR_INVALID, "srt_update_scene: too many world triangles");
			uint32_t link = use_bvh ? SRT_BVH_NONE : (uint32_t)total_wtris; // first world triangle of the model; BVH: root reference (NONE = nothing to walk)
			if (use_bvh && m.num_triangles > 0) {
				const uint64_t th = range_hash(m);
				// An entry of the previous call with the same triangles: as it is when the transform did not change either,
				// otherwise refitted. Entries only LEAVE the cache once the whole shape loop has validated (an early error
				// return keeps every hierarchy).
				BvhCacheEntry *kept = deform_on ? matched[i].ent : find_same_triangles(m, th);
				bool deformed = deform_on && matched[i].deformed;
				if (deformed && policy.deform.rebuild_ratio > 0.0f && BvhBuilder::cost_ratio(kept->cost_now, kept->cost_built) > (double)policy.deform.rebuild_ratio) {
					kept = nullptr, deformed = false; // refitted too often: the tree has degraded past the caller's bound, build a new one
					deform_rebuilt++;
				}
				BvhCacheEntry *ent;
				bool device_built = false;
				if (kept) {
					ent = kept;
					ent->claimed = true;
					ent->triangle_index = m.triangle_index;
					const bool on_device = policy.refit == SRT_REFIT_DEVICE;
					if (deformed) { // other bytes in the same triangle range: the tree and its records' order stay, every box is recomputed
						ent->tris.assign(triangles + m.triangle_index, triangles + m.triangle_index + m.num_triangles);
						ent->tri_hash = th;
						memcpy(ent->transform, m.transform, sizeof ent->transform);
						if (on_device) ent->stale = true;
						else ent->refit(m, triangles), ent->cost_now = BvhBuilder::wide_cost(ent->nodes, ent->wide);
						bvh_refitted++, deform_kept++;
					} else if (ent->same_transform(m) && (!ent->stale || on_device)) {
						bvh_reused++; // (a stale one: refitted on the device again, below)
					} else if (on_device) { // the model moved: the topology is uploaded as it is, the device recomputes the boxes
						memcpy(ent->transform, m.transform, sizeof ent->transform);
						ent->stale = true;
						bvh_refitted++;
					} else { // the model moved (or its boxes are a device refit behind): keep the tree, recompute the boxes
						ent->refit(m, triangles);
						if (deform_on) ent->cost_now = BvhBuilder::wide_cost(ent->nodes, ent->wide);
						memcpy(ent->transform, m.transform, sizeof ent->transform);
						bvh_refitted++;
					}
					plan.emplace_back(true, (size_t)(kept - cache->entries.data()));
				} else {
					fresh.emplace_back();
					ent = &fresh.back();
					device_built = policy.build.mode == SRT_BUILD_DEVICE && m.num_triangles >= policy.build.min_triangles;
					// on the device: the topology of the count, stale with the identity order -- the device sorts the records
					// before the pre-pass reads them and refits every box behind it
					if (device_built) *ent = cache->balanced_topology(m.num_triangles);
					else ent->build(m, triangles);
					ent->count = m.num_triangles;
					ent->triangle_index = m.triangle_index;
					ent->tri_hash = th;
					memcpy(ent->transform, m.transform, sizeof ent->transform);
					ent->tris.assign(triangles + m.triangle_index, triangles + m.triangle_index + m.num_triangles);
					plan.emplace_back(false, fresh.size() - 1);
				}
				// Indices inside an entry are relative to the model's first block / first record: shift them to where the
				// model lands in the scene's arrays.
				const uint32_t b0 = (uint32_t)(bvh_blocks.size() / 32), r0 = (uint32_t)total_wtris;
				const BvhBuilder::Wide &wd = ent->wide;
				if ((uint64_t)b0 + wd.blocks.size() / 32 > SRT_BVH_INDEX_MAX) return fail(SRT_ERR_INVALID, "srt_update_scene: too many BVH blocks");
				if (wd.need > SRT_BVH_STACK_CAP) return fail(SRT_ERR_INVALID, "srt_update_scene: BVH deeper than the walk's stack"); // unreachable below 2^28 triangles
				bvh_blocks.insert(bvh_blocks.end(), wd.blocks.begin(), wd.blocks.end());
				for (uint32_t ib : wd.inner) bvh_blocks[32 * (size_t)(b0 + ib) + SRT_BVH_FIRST_DWORD] += b0; // where the block's children lie
				bvh_dest.resize(r0 + (size_t)m.num_triangles);
				for (uint32_t r = 0; r < m.num_triangles; r++) bvh_dest[r0 + r] = wd.dest[r] + (b0 << 2);
				bvh_canonical_nodes += ent->nodes.size();
				bvh_order.insert(bvh_order.end(), ent->order.begin(), ent->order.end());
				link = wd.root == SRT_BVH_NONE ? SRT_BVH_NONE : wd.root + b0; // the root reference (a leaf reference for a model of <= 3 triangles)
				if (ent->stale) { // its host boxes are not this transform's: never walked as they are
					ent->wide.ensure_schedule();
					sp.refit_models.push_back({(uint32_t)i, r0, m.num_triangles, 0u});
					stale_plan.emplace_back(ent, b0);
					if (m.num_triangles > sp.refit_max_records) sp.refit_max_records = m.num_triangles;
					if (device_built) {
						sp.build_models.push_back({(uint32_t)i, r0, m.num_triangles, sp.build_tiles});
						sp.build_tiles += SRT_BUILD_TILES(m.num_triangles);
						sp.build_entry.push_back(plan.size() - 1);
						if (m.num_triangles > sp.build_max_records) sp.build_max_records = m.num_triangles;
					}
					if (deform_on) { // the cost launch's view of the model
						const uint32_t nb = (uint32_t)(wd.blocks.size() / 32);
						sp.refit_cost_ranges.push_back({b0, nb});
						sp.refit_cost_entry.push_back(plan.size() - 1);
						sp.refit_cost_built.push_back(ent->cost_built);
						sp.refit_cost_fresh.push_back(device_built ? 1 : 0);
						sp.refit_weights.resize((size_t)b0 + nb, 0);
						for (const BvhBuilder::Wide::Job &j : wd.jobs) sp.refit_weights[b0 + j.self] = (uint8_t)j.nk;
						for (uint32_t d : wd.dest) sp.refit_weights[b0 + (d >> 2)]++;
					}
				} else if (deform_on) {
					sp.deform_worst_ratio = std::max(sp.deform_worst_ratio, BvhBuilder::cost_ratio(ent->cost_now, ent->cost_built));
				}
				bvh_leaves += ent->leaves;
				if (ent->depth > bvh_depth) bvh_depth = ent->depth;
			}
			data.insert(data.end(), {m.bounding_min.x, m.bounding_min.y, m.bounding_min.z, u2f(link), m.bounding_max.x, m.bounding_max.y,
			                         m.bounding_max.z, u2f(use_bvh ? 0u : m.num_triangles)});
			wr.first_wtri = (uint32_t)total_wtris;
			offs[i] = (uint32_t)total_wtris;
			// brute force: blocks of 4, the tail stays all-zero (never hit); BVH: records are addressed one by one
			total_wtris += use_bvh ? (uint64_t)m.num_triangles : (((uint64_t)m.num_triangles + 3u) & ~3ull);
			if (m.num_triangles > max_tris) max_tris = m.num_triangles;
			num_models++;
		}
	}
	pad_run();
	// group headers: three blocks each (device_types.h BlockGroup); the data of a last, partial group is zero-filled
	std::vector<BlockGroup> &groups = sp.groups;
	groups.assign((runs.size() + 2) / 3, BlockGroup());
	uint32_t n_big = 0; // big model number k waits in scan stack k & 1 (trace_body.inc)
	for (size_t b = 0; b < runs.size(); b++) {
		BlockGroup &g = groups[b / 3];
		if (b % 3 == 0) memset(&g, 0, sizeof g);
		const uint32_t big = runs[b].data_off >> 31;
		g.code |= (((uint32_t)runs[b].type + 1u) | (runs[b].count << 2) | (big << 5) | ((big ? (n_big++ & 1u) : 0u) << 6)) << (8 * (b % 3));
		g.first[b % 3] = runs[b].first_shape;
	}
	data.resize(groups.size() * 48 + 16, 0.0f);
	// a scene class (scene_class() below) is a scene of one group whose blocks hold shapes 0 .. n - 1 with none left out
	sp.one_group_code = 0;
	if (groups.size() == 1 && num_models == 0) {
		uint32_t next = 0;
		bool packed = true;
		for (size_t b = 0; b < runs.size(); b++) packed = packed && runs[b].first_shape == next, next += runs[b].count;
		if (packed && next == n_shapes) sp.one_group_code = groups[0].code;
	}
	// its plane form: 2 bits per plane slot, in block order (fillers and other shapes' slots stay 0)
	sp.plane_axes = 0;
	if (sp.one_group_code != 0)
		for (size_t b = 0; b < runs.size(); b++)
			for (uint32_t i = 0; runs[b].type == SRT_SHAPE_PLANE && i < runs[b].count; i++) {
				const srt_plane &pl = shapes[runs[b].first_shape + i].shape.plane;
				const float n[3] = {pl.normal.x, pl.normal.y, pl.normal.z}, q[3] = {pl.position.x, pl.position.y, pl.position.z};
				sp.plane_axes |= (uint32_t)srt_plane_axis_code(n, q) << (4 * b + 2 * i);
			}
	if (!stale_plan.empty()) { // the refit schedule of the scene: level h of every stale model, then level h + 1, ...
		size_t top = 0;
		for (const auto &st : stale_plan) top = std::max(top, st.first->wide.level_off.size());
		sp.refit_levels.assign(1, 0u);
		for (size_t h = 1; h < top; h++) {
			for (const auto &st : stale_plan) {
				const BvhBuilder::Wide &wd = st.first->wide;
				if (h >= wd.level_off.size()) continue;
				for (uint32_t k = wd.level_off[h - 1]; k < wd.level_off[h]; k++) sp.refit_sched.push_back(wd.sched[k] + st.second);
			}
			sp.refit_levels.push_back((uint32_t)sp.refit_sched.size());
		}
		for (size_t k = 0; k < sp.build_models.size(); k++)
			sp.build_extents.insert(sp.build_extents.end(), {SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT});
		for (size_t k = 0; k < stale_plan.size(); k++)
			sp.refit_extents.insert(sp.refit_extents.end(), {SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT});
	}
	const uint64_t build_us =
	    (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - build_t0).count();

	// Device-side material table = the caller's records with three per-material constants
	// parked in padding floats, so the glass branch does no division at all:
	//   _pad[0] (offset 24) = 1.0f / refraction_index                      (render.cl:442, front face)
	//   _pad[1] (offset 28) = Schlick r0 for mu = 1/refraction_index       (render.cl:174-175, fp64 then float)
	//   color._pad (offset 44) = Schlick r0 for mu = refraction_index      (back face)
	// Same IEEE operations the kernel would run per hit, hence the same bits.
	std::vector<srt_material> &dev_mats = sp.dev_mats;
	dev_mats.assign(materials, materials + n_materials);
	auto schlick_r0 = [](float mu) {
		float r0 = (float)((1.0 - (double)mu) / (1.0 + (double)mu));
		return r0 * r0;
	};
	// When every probability of the scene has a threshold (bernoulli_threshold() above) below 2^32 (p <= 1 does) the device table
	// carries the thresholds' bits in place of metallic / specular / transmittance.
	bool unit_materials = true;
	for (const auto &m : dev_mats)
		if (bernoulli_threshold(m.metallic) >> 32 || bernoulli_threshold(m.specular) >> 32 || bernoulli_threshold(m.transmittance) >> 32) unit_materials = false;
	sp.unit_materials = unit_materials;
	{
		// what holds for every material (SRT_MF_*): draws the scene decides are not made by the kernel
		bool no_specular = unit_materials, plain = true;
		for (const auto &m : dev_mats) {
			if (bernoulli_threshold(m.specular) != 0) no_specular = false;
			for (float c : {m.color.x, m.color.y, m.color.z})
				if (!std::isfinite(c) || (c == 0.0f && std::signbit(c))) plain = false;
		}
		sp.material_flags = (no_specular ? SRT_MF_NO_SPECULAR : 0) | (plain ? SRT_MF_PLAIN_COLORS : 0);
	}
	for (auto &m : dev_mats) {
		if (unit_materials) {
			const uint32_t tm = (uint32_t)bernoulli_threshold(m.metallic), ts = (uint32_t)bernoulli_threshold(m.specular), tt = (uint32_t)bernoulli_threshold(m.transmittance);
			memcpy(&m.metallic, &tm, 4), memcpy(&m.specular, &ts, 4), memcpy(&m.transmittance, &tt, 4);
		}
		const float inv_ior = 1.0f / m.refraction_index;
		m._pad[0] = inv_ior;
		m._pad[1] = schlick_r0(inv_ior);
		m.color._pad = schlick_r0(m.refraction_index);
	}
	sp.bvh_info[0] = bvh_canonical_nodes, sp.bvh_info[1] = bvh_leaves, sp.bvh_info[2] = bvh_depth, sp.bvh_info[3] = use_bvh ? build_us : 0;
	sp.bvh_info[4] = use_bvh ? plan.size() - bvh_reused - bvh_refitted : 0, sp.bvh_info[5] = bvh_reused, sp.bvh_info[6] = bvh_refitted;
	sp.deform_info[0] = deform_kept, sp.deform_info[1] = deform_rebuilt;
	if (deform_on) sp.refit_weights.resize(bvh_blocks.size() / 32, 0);
	if (use_bvh) {
		std::vector<BvhCacheEntry> next_cache;
		next_cache.reserve(plan.size());
		for (const auto &pl : plan) next_cache.push_back(std::move(pl.first ? cache->entries[pl.second] : fresh[pl.second]));
		cache->entries = std::move(next_cache);
	}
	sp.all_materials_ok = true;
	for (size_t i = 0; i < n_shapes; i++)
		if (shapes[i].material < 0) sp.all_materials_ok = false;
	return SRT_OK;
}

extern "C" int srt_plane_axis_code_host(const float normal[3], const float position[3], int *code_out) {
	if (!normal || !position || !code_out) return SRT_ERR_INVALID;
	*code_out = srt_plane_axis_code(normal, position);
	return SRT_OK;
}

extern "C" int srt_bernoulli_threshold_host(float p, uint64_t *threshold_out) {
	if (!threshold_out) return SRT_ERR_INVALID;
	*threshold_out = bernoulli_threshold(p);
	return SRT_OK;
}
