// accel_device.hip — upkeep of the BVH on the device, host side: what drives bvh_refit.hip and bvh_build.hip around an upload's
// pre-pass (srt_abi.hip upload_scene_begin calls the hooks declared in srt_internal.h), the results on their way back to the
// hierarchy cache, and the srt_*acceleration* entry points of include/srt_abi.h. The policy is scene_prep.h's AccelPolicy
// (srt_tracer::policy), the state srt_internal.h's AccelDevice (srt_tracer::upkeep); nothing else reads either.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstring>

#include "srt_internal.h"

// SRT_DEFORM_REFIT: waits for the last upload's cost sums (behind their event only, not for the stream) and turns them into
// ratios: on the handle for srt_acceleration_deform_info, and on the hierarchies `cache` keeps (the handle's own; a group's first
// member's) for the next srt_update_scene's rebuild rule. Once per upload.
int srt_accel_deform_consume(srt_tracer *t, BvhCache *cache) {
	AccelDevice &a = t->upkeep;
	if (!a.deform_sums_back.pending) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, a.deform_sums_back.wait());
	for (size_t k = 0; k < a.deform_entry.size(); k++) {
		const double cost_now = BvhBuilder::cost_of(a.deform_sums_back.host[2 * k], a.deform_sums_back.host[2 * k + 1]);
		const bool fresh = k < a.deform_fresh.size() && a.deform_fresh[k]; // built on the device by that upload: this IS its cost as built
		a.deform_ratio[k] = BvhBuilder::cost_ratio(cost_now, fresh ? cost_now : a.deform_built[k]);
		if (cache && a.deform_entry[k] < cache->entries.size()) {
			cache->entries[a.deform_entry[k]].cost_now = cost_now;
			if (fresh) cache->entries[a.deform_entry[k]].cost_built = cost_now;
		}
	}
	return SRT_OK;
}

// behind pass C: the cost of every refitted hierarchy, summed on the device and copied to pinned host memory
static int deform_cost_on_device(srt_tracer *t, const ScenePrep &sp) {
	AccelDevice &a = t->upkeep;
	const size_t n = sp.refit_cost_ranges.size();
	a.deform_entry = sp.refit_cost_entry, a.deform_built = sp.refit_cost_built, a.deform_fresh = sp.refit_cost_fresh;
	a.deform_ratio.assign(n, 0.0);
	if (n == 0) return SRT_OK;
	SRT_HIP(t, a.deform_ranges.reserve(n));
	SRT_HIP(t, a.deform_weights.reserve(sp.refit_weights.size()));
	SRT_HIP(t, a.deform_sums.reserve(2 * n));
	SRT_HIP(t, a.deform_sums_back.reserve(2 * n));
	SRT_HIP(t, hipMemcpyAsync(a.deform_ranges.ptr, sp.refit_cost_ranges.data(), n * sizeof(RefitCostRange), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipMemcpyAsync(a.deform_weights.ptr, sp.refit_weights.data(), sp.refit_weights.size(), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipMemsetAsync(a.deform_sums.ptr, 0, 2 * n * sizeof(double), t->stream));
	uint32_t max_blocks = 0;
	for (const RefitCostRange &r : sp.refit_cost_ranges) max_blocks = r.num_blocks > max_blocks ? r.num_blocks : max_blocks;
	a.deform_info[2] = (uint64_t)srt_launch_refit_cost(a.refit_boxes.ptr, a.deform_weights.ptr, a.deform_ranges.ptr, a.deform_sums.ptr, (uint32_t)n, max_blocks, t->stream);
	SRT_HIP(t, hipGetLastError());
	SRT_HIP(t, a.deform_sums_back.copy(a.deform_sums.ptr, 2 * n, t->stream));
	return SRT_OK;
}

// SRT_BUILD_DEVICE: waits for the last upload's sorted order (behind its event only, not for the stream) and hands every built
// model's records to its hierarchy in `cache` (the handle's own; a group's first member's), so that every host path that reads
// an entry's order finds it. An entry whose order never came back (an upload that failed half way) leaves the cache: its
// model is built again. Once per upload.
int srt_accel_build_consume(srt_tracer *t, BvhCache *cache) {
	AccelDevice &a = t->upkeep;
	if (a.build_order_back.pending) {
		SRT_HIP(t, hipSetDevice(t->device));
		SRT_HIP(t, a.build_order_back.wait());
		for (size_t k = 0; cache && k < a.build_entry.size(); k++) {
			if (a.build_entry[k] >= cache->entries.size()) continue;
			BvhCacheEntry &e = cache->entries[a.build_entry[k]];
			const RefitModel &rm = a.build_ranges[k];
			if (!e.order_pending || e.count != rm.num_records) continue;
			e.order.assign(a.build_order_back.host + rm.first_record, a.build_order_back.host + rm.first_record + rm.num_records);
			e.order_pending = false;
		}
	}
	if (cache)
		for (size_t k = cache->entries.size(); k-- > 0;)
			if (cache->entries[k].order_pending) cache->entries.erase(cache->entries.begin() + (ptrdiff_t)k);
	return SRT_OK;
}

// SRT_BUILD_DEVICE, before the pre-pass: the order of the models this call builds (bvh_build.hip) -- their extents over the
// identity order the upload carries, a Morton code per record, the sort, whose last pass writes the scene's order array. Under
// SRT_BUILD_ORDER_MEDIAN the median-split launches instead (they take their extents per range, of the centroids); a model too
// large for them keeps the Morton order: then the Morton launches run first, over every model, and the median ones overwrite
// the order of the models they take. (Nothing to do, and no launch, without SRT_BUILD_DEVICE.)
int srt_accel_before_prepass(srt_tracer *t, const ScenePrep &sp) {
	AccelDevice &a = t->upkeep;
	for (uint64_t &v : a.build_info) v = 0;
	a.build_span.timed = false;
	a.build_order_back.pending = false; // (upload_scene_begin has waited for the stream: an earlier copy has landed, nobody asked for it)
	a.build_entry.clear(), a.build_ranges.clear();
	if (sp.build_models.empty()) return SRT_OK;
	const uint32_t n_models = (uint32_t)sp.build_models.size();
	const size_t records = sp.bvh_order.size();
	SRT_HIP(t, a.build_models.reserve(n_models));
	SRT_HIP(t, a.build_extents.reserve(sp.build_extents.size()));
	SRT_HIP(t, a.build_table.reserve(256 * (size_t)sp.build_tiles));
	for (int k = 0; k < 2; k++) {
		SRT_HIP(t, a.build_keys[k].reserve(records));
		SRT_HIP(t, a.build_vals[k].reserve(records));
	}
	SRT_HIP(t, hipMemcpyAsync(a.build_models.ptr, sp.build_models.data(), n_models * sizeof(RefitModel), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipMemcpyAsync(a.build_extents.ptr, sp.build_extents.data(), sp.build_extents.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
	const bool median = t->policy.build.order == SRT_BUILD_ORDER_MEDIAN;
	bool morton = !median;
	uint32_t median_max_records = 0;
	if (median) { // per model its first range slot, then the slots: (2^levels - 1) empty boxes per model
		std::vector<uint32_t> &up = a.build_ranges_host;
		up.assign(n_models, 0u);
		uint32_t slots = 0;
		for (uint32_t k = 0; k < n_models; k++) {
			const uint32_t n = sp.build_models[k].num_records, levels = srt_build_median_levels(n);
			up[k] = slots;
			if (levels > SRT_BUILD_MEDIAN_MAX_LEVELS) {
				morton = true;
				continue;
			}
			slots += (1u << levels) - 1u;
			if (n > median_max_records) median_max_records = n;
		}
		for (uint32_t k = 0; k < slots; k++)
			up.insert(up.end(), {SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_LO_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT, SRT_REFIT_EXT_HI_INIT});
		SRT_HIP(t, a.build_ranges_dev.reserve(up.size()));
		SRT_HIP(t, hipMemcpyAsync(a.build_ranges_dev.ptr, up.data(), up.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
	}
	if (t->timers_in_render) SRT_HIP(t, a.build_span.begin(t->stream));
	RefitParams rp;
	memset(&rp, 0, sizeof rp);
	rp.shapes = t->shapes.ptr;
	rp.triangles = t->triangles.ptr;
	rp.order = t->bvh_order.ptr;
	rp.models = a.build_models.ptr;
	rp.extents = a.build_extents.ptr;
	BuildParams bp;
	bp.shapes = t->shapes.ptr;
	bp.triangles = t->triangles.ptr;
	bp.models = a.build_models.ptr;
	bp.extents = a.build_extents.ptr;
	for (int k = 0; k < 2; k++) bp.keys[k] = a.build_keys[k].ptr, bp.vals[k] = a.build_vals[k].ptr;
	bp.table = a.build_table.ptr;
	bp.order = t->bvh_order.ptr;
	bp.range_first = median ? a.build_ranges_dev.ptr : nullptr;
	bp.ranges = median ? a.build_ranges_dev.ptr + n_models : nullptr;
	int launches = 0;
	if (morton) {
		launches += srt_launch_refit_extents(rp, n_models, sp.build_max_records, t->stream);
		launches += srt_launch_build_keys(bp, n_models, sp.build_max_records, t->stream);
		launches += srt_launch_build_sort(bp, n_models, sp.build_max_records, t->stream);
	}
	if (median) launches += srt_launch_build_median(bp, n_models, median_max_records, t->stream);
	SRT_HIP(t, hipGetLastError());
	uint64_t sorted = 0;
	for (const RefitModel &rm : sp.build_models) sorted += rm.num_records;
	a.build_info[0] = n_models, a.build_info[1] = sorted, a.build_info[2] = (uint64_t)launches;
	return SRT_OK;
}

// SRT_REFIT_DEVICE: behind the pre-pass, new boxes for the models whose blocks were uploaded from a stale hierarchy
// (bvh_refit.hip): passes A and B over their records, then one launch per height level of their inner blocks
static int refit_on_device(srt_tracer *t, const ScenePrep &sp) {
	AccelDevice &a = t->upkeep;
	for (uint64_t &v : a.refit_info) v = 0;
	a.refit_span.timed = false;
	a.deform_sums_back.pending = false; // (upload_scene_begin has waited for the stream: an earlier copy has landed, nobody asked for it)
	a.deform_info[0] = sp.deform_info[0], a.deform_info[1] = sp.deform_info[1], a.deform_info[2] = 0, a.deform_info[3] = 0;
	a.deform_worst_host = sp.deform_worst_ratio;
	a.deform_entry.clear(), a.deform_built.clear(), a.deform_ratio.clear(), a.deform_fresh.clear();
	if (sp.refit_models.empty()) return SRT_OK;
	const uint32_t n_models = (uint32_t)sp.refit_models.size();
	SRT_HIP(t, a.refit_models.reserve(n_models));
	SRT_HIP(t, a.refit_extents.reserve(sp.refit_extents.size()));
	SRT_HIP(t, a.refit_sched.reserve(sp.refit_sched.size()));
	SRT_HIP(t, a.refit_boxes.reserve(sp.bvh_blocks.size() / 32 * 6));
	SRT_HIP(t, hipMemcpyAsync(a.refit_models.ptr, sp.refit_models.data(), n_models * sizeof(RefitModel), hipMemcpyHostToDevice, t->stream));
	SRT_HIP(t, hipMemcpyAsync(a.refit_extents.ptr, sp.refit_extents.data(), sp.refit_extents.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
	if (!sp.refit_sched.empty())
		SRT_HIP(t, hipMemcpyAsync(a.refit_sched.ptr, sp.refit_sched.data(), sp.refit_sched.size() * sizeof(uint32_t), hipMemcpyHostToDevice, t->stream));
	RefitParams rp;
	rp.shapes = t->shapes.ptr;
	rp.triangles = t->triangles.ptr;
	rp.order = t->bvh_order.ptr;
	rp.dest = t->bvh_dest.ptr;
	rp.models = a.refit_models.ptr;
	rp.extents = a.refit_extents.ptr;
	rp.boxes = a.refit_boxes.ptr;
	rp.blocks = t->bvh_blocks.ptr;
	rp.sched = a.refit_sched.ptr;
	if (t->timers_in_render) SRT_HIP(t, a.refit_span.begin(t->stream));
	int launches = srt_launch_refit_extents(rp, n_models, sp.refit_max_records, t->stream);
	launches += srt_launch_refit_leaves(rp, n_models, sp.refit_max_records, t->stream);
	for (size_t h = 1; h < sp.refit_levels.size(); h++)
		launches += srt_launch_refit_level(rp, sp.refit_levels[h - 1], sp.refit_levels[h] - sp.refit_levels[h - 1], t->stream);
	SRT_HIP(t, hipGetLastError());
	if (const int rc = deform_cost_on_device(t, sp)) return rc; // (nothing to do, and no launch, without SRT_DEFORM_REFIT)
	if (t->timers_in_render) SRT_HIP(t, a.refit_span.end(t->stream));
	a.refit_info[0] = n_models, a.refit_info[1] = sp.refit_sched.size(), a.refit_info[2] = (uint64_t)launches;
	return SRT_OK;
}

// Behind the pre-pass: the refit, and behind it what is left of SRT_BUILD_DEVICE for the same upload -- the end of its timed
// span, and the sorted order on its way to pinned host memory
int srt_accel_behind_prepass(srt_tracer *t, const ScenePrep &sp) {
	if (const int rc = refit_on_device(t, sp)) return rc;
	if (sp.build_models.empty()) return SRT_OK;
	AccelDevice &a = t->upkeep;
	if (t->timers_in_render) SRT_HIP(t, a.build_span.end(t->stream));
	SRT_HIP(t, a.build_order_back.reserve(sp.bvh_order.size()));
	a.build_entry = sp.build_entry, a.build_ranges = sp.build_models;
	SRT_HIP(t, a.build_order_back.copy(t->bvh_order.ptr, sp.bvh_order.size(), t->stream));
	return SRT_OK;
}

// srt_last_refit_kernel_ms / srt_last_build_kernel_ms: the span of the last upload; 0 when that upload recorded none
static int span_ms(srt_tracer *t, const TimedSpan &span, float *ms) {
	*ms = 0.f;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	SRT_HIP(t, span.elapsed(ms));
	return SRT_OK;
}

extern "C" {

int srt_set_acceleration(srt_tracer *t, int mode) {
	if (!t) return SRT_ERR_INVALID;
	if (mode != SRT_ACCEL_NONE && mode != SRT_ACCEL_BVH) return fail(t, SRT_ERR_INVALID, "srt_set_acceleration: unknown mode");
	t->policy.accel = mode;
	return SRT_OK;
}

int srt_set_acceleration_refit(srt_tracer *t, int mode) {
	if (!t) return SRT_ERR_INVALID;
	if (mode != SRT_REFIT_HOST && mode != SRT_REFIT_DEVICE) return fail(t, SRT_ERR_INVALID, "srt_set_acceleration_refit: unknown mode");
	t->policy.refit = mode;
	return SRT_OK;
}

int srt_set_acceleration_deform(srt_tracer *t, int mode, float rebuild_ratio) {
	if (!t) return SRT_ERR_INVALID;
	if (mode != SRT_DEFORM_REBUILD && mode != SRT_DEFORM_REFIT) return fail(t, SRT_ERR_INVALID, "srt_set_acceleration_deform: unknown mode");
	if (!(rebuild_ratio == 0.0f || (rebuild_ratio > 1.0f && rebuild_ratio <= FLT_MAX))) // (a NaN fails every comparison)
		return fail(t, SRT_ERR_INVALID, "srt_set_acceleration_deform: rebuild_ratio must be 0 or a finite value above 1");
	t->policy.deform.mode = mode;
	t->policy.deform.rebuild_ratio = rebuild_ratio;
	return SRT_OK;
}

int srt_set_acceleration_build(srt_tracer *t, int mode, uint32_t min_triangles) {
	if (!t) return SRT_ERR_INVALID;
	if (mode != SRT_BUILD_HOST && mode != SRT_BUILD_DEVICE) return fail(t, SRT_ERR_INVALID, "srt_set_acceleration_build: unknown mode");
	t->policy.build.mode = mode;
	t->policy.build.min_triangles = min_triangles;
	return SRT_OK;
}

int srt_set_acceleration_build_order(srt_tracer *t, int order) {
	if (!t) return SRT_ERR_INVALID;
	if (order != SRT_BUILD_ORDER_MORTON && order != SRT_BUILD_ORDER_MEDIAN) return fail(t, SRT_ERR_INVALID, "srt_set_acceleration_build_order: unknown order");
	t->policy.build.order = order;
	return SRT_OK;
}

int srt_acceleration_info(const srt_tracer *t, uint64_t out[7]) {
	if (!t || !out) return SRT_ERR_INVALID;
	for (int i = 0; i < 7; i++) out[i] = t->bvh_active ? t->bvh_info[i] : 0;
	return SRT_OK;
}

int srt_acceleration_refit_info(const srt_tracer *t, uint64_t out[4]) {
	if (!t || !out) return SRT_ERR_INVALID;
	for (int i = 0; i < 4; i++) out[i] = t->bvh_active ? t->upkeep.refit_info[i] : 0;
	return SRT_OK;
}

int srt_acceleration_deform_info(srt_tracer *t, uint64_t out[4], double *worst_ratio) {
	if (!t || !out || !worst_ratio) return SRT_ERR_INVALID;
	for (int i = 0; i < 4; i++) out[i] = 0;
	*worst_ratio = 0.0;
	if (const int rc = srt_accel_deform_consume(t, t->bvh_cache)) return rc;
	if (!t->bvh_active) return SRT_OK;
	for (int i = 0; i < 4; i++) out[i] = t->upkeep.deform_info[i];
	double worst = t->upkeep.deform_worst_host;
	for (double r : t->upkeep.deform_ratio) worst = r > worst ? r : worst;
	*worst_ratio = worst;
	return SRT_OK;
}

int srt_acceleration_build_info(srt_tracer *t, uint64_t out[4]) {
	if (!t || !out) return SRT_ERR_INVALID;
	for (int i = 0; i < 4; i++) out[i] = 0;
	if (const int rc = srt_accel_deform_consume(t, t->bvh_cache)) return rc; // (a built model's cost as built comes with the same upload)
	if (const int rc = srt_accel_build_consume(t, t->bvh_cache)) return rc;
	for (int i = 0; i < 4; i++) out[i] = t->bvh_active ? t->upkeep.build_info[i] : 0;
	return SRT_OK;
}

int srt_last_refit_kernel_ms(srt_tracer *t, float *ms) { return t && ms ? span_ms(t, t->upkeep.refit_span, ms) : SRT_ERR_INVALID; }
int srt_last_build_kernel_ms(srt_tracer *t, float *ms) { return t && ms ? span_ms(t, t->upkeep.build_span, ms) : SRT_ERR_INVALID; }

int srt_read_bvh_blocks(srt_tracer *t, uint32_t *blocks_out, size_t blocks_cap, size_t *n_blocks) {
	if (!t || !n_blocks) return SRT_ERR_INVALID;
	const size_t n = t->bvh_active ? t->bvh_num_blocks : 0;
	*n_blocks = n;
	const size_t take = n < blocks_cap ? n : blocks_cap;
	if (!blocks_out || take == 0) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	SRT_HIP(t, hipMemcpy(blocks_out, t->bvh_blocks.ptr, take * 32 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return SRT_OK;
}

} // extern "C"
