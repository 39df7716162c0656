// scene_prep.h — the host pass of srt_update_scene / srt_group_update_scene: everything a device needs of a scene, as host arrays.
// No HIP, and no handle: the caller (srt_abi.hip) passes what the pass reads of one -- its AccelPolicy and hierarchy cache -- and uploads the result.
#ifndef SRT_SCENE_PREP_H
#define SRT_SCENE_PREP_H

#include <string>
#include <vector>

#include "bvh_host.h"

// Everything a device needs of a scene, made on the host ONCE per srt_update_scene / srt_group_update_scene: shape blocks and group
// headers, winner records, world-triangle offsets, the hierarchy in its device form, the device material table (bernoulli()
// thresholds, Schlick constants). A group of N devices prepares one of these and uploads it N times (round 4; before, the whole
// host pass -- 18 ms of BVH build for 10^5 triangles -- ran once per device, in turn).
struct ScenePrep {
	std::vector<BlockGroup> groups;
	std::vector<float> data;
	std::vector<WinnerRec> winners;
	std::vector<uint32_t> offs, bvh_blocks, bvh_order, bvh_dest;
	std::vector<srt_material> dev_mats;
	uint64_t total_wtris = 0, max_tris = 0;
	int num_models = 0;
	bool use_bvh = false, unit_materials = false, all_materials_ok = true;
	int material_flags = 0;
	uint32_t one_group_code = 0; // srt_tracer::one_group_code
	uint32_t plane_axes = 0;     // srt_tracer::plane_axes: the one group's plane form (device_types.h "Axis planes")
	uint64_t bvh_info[7] = {0, 0, 0, 0, 0, 0, 0};
	// SRT_REFIT_DEVICE: the models whose blocks above come from a stale hierarchy (bvh_host.h) and are refitted on the device
	// behind the upload (bvh_refit.hip), their empty extents, their inner blocks as absolute indices level by level -- level h
	// of ALL of them in refit_sched[refit_levels[h - 1], refit_levels[h]): one launch per level, not per model and level
	std::vector<RefitModel> refit_models;
	std::vector<uint32_t> refit_extents, refit_sched, refit_levels;
	uint32_t refit_max_records = 0;
	// SRT_DEFORM_REFIT (empty / zero without it): {models kept across a change of triangle bytes, models rebuilt on their cost
	// ratio}; and what the cost launch behind the device's refit needs of every refitted model (bvh_refit.hip
	// srt_refit_cost_kernel): its blocks' range, per block of the scene the weight of its box in the cost (an inner block's
	// children, a leaf block's triangles; other models' stay 0), its entry in the cache as this call leaves it and that
	// entry's cost as built. deform_worst_ratio: the largest cost ratio the host knows among the models NOT refitted on the device.
	uint64_t deform_info[2] = {0, 0};
	std::vector<RefitCostRange> refit_cost_ranges;
	std::vector<uint8_t> refit_weights;
	std::vector<size_t> refit_cost_entry;
	std::vector<double> refit_cost_built;
	double deform_worst_ratio = 0.0;
	std::vector<uint8_t> refit_cost_fresh; // per cost range: the model was built by this call (below): the sum becomes its cost as built
	// SRT_BUILD_DEVICE (empty / zero without it): the models whose order the device sorts before the pre-pass (bvh_build.hip) --
	// bvh_order holds the identity for their records, their blocks come from the balanced topology and they are among
	// refit_models, too --, their first tiles in the sort's table (RefitModel::first_tile) adding up to build_tiles, their empty
	// extents, and per model its entry in the cache as this call leaves it: where the sorted order goes once it is back.
	std::vector<RefitModel> build_models;
	std::vector<uint32_t> build_extents;
	std::vector<size_t> build_entry;
	uint32_t build_max_records = 0, build_tiles = 0;
};

// srt_set_acceleration_build / _build_order: who builds a model that has no hierarchy to keep (nothing without SRT_ACCEL_BVH)
struct BuildPolicy {
	int mode = SRT_BUILD_HOST;
	uint32_t min_triangles = 0;         // SRT_BUILD_DEVICE: smaller models keep the host's build
	int order = SRT_BUILD_ORDER_MORTON; // SRT_BUILD_DEVICE: the order the device sorts into (accel_device.hip; the host pass does not read it)
};

// srt_set_acceleration_deform: what becomes of a model whose triangle bytes changed (nothing without SRT_ACCEL_BVH)
struct DeformPolicy {
	int mode = SRT_DEFORM_REBUILD;
	float rebuild_ratio = 0.0f; // SRT_DEFORM_REFIT: a kept model whose last known cost ratio is above this is rebuilt; 0 = never
};

// THE acceleration policy of a handle: what the five srt_set_acceleration* setters write and the next srt_update_scene reads. A
// group copies its first member's to every member whole; a new policy is a member here and nothing else.
struct AccelPolicy {
	int accel = SRT_ACCEL_NONE; // SRT_ACCEL_*
	int refit = SRT_REFIT_HOST; // SRT_REFIT_*: who refits a model that only moved (nothing without SRT_ACCEL_BVH)
	DeformPolicy deform;
	BuildPolicy build;
};

// cache: the caller's hierarchy cache (a group: its first member's); scan_suspend_min: srt_scan_suspend_min()
int prepare_scene(const AccelPolicy &policy, BvhCache *&cache, int scan_suspend_min, std::string &err, ScenePrep &sp, const srt_shape *shapes, size_t n_shapes,
                  const srt_triangle *triangles, size_t n_triangles, const srt_material *materials, size_t n_materials, const srt_scene_data *scene);

uint64_t bernoulli_threshold(float pr);
int srt_plane_axis_code(const float normal[3], const float position[3]);

#endif
