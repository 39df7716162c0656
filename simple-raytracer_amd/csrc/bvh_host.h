// bvh_host.h — the host BVH builder of libsrt_hip.so: what srt_update_scene (scene_prep.cpp) builds, caches and refits per model
// instance, and what srt_bvh_build_host / srt_bvh_wide_host hand out. No HIP: the standard library, the public record types and
// device_types.h only, so it compiles with any C++17 compiler and runs without a device (tests/csrc/host_units_check.cpp).
#ifndef SRT_BVH_HOST_H
#define SRT_BVH_HOST_H

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/srt_abi.h"
#include "device_types.h"

// ---- BVH builder (host; layout in device_types.h) --------------------
// Top-down, binned surface-area heuristic (16 bins, all three axes), leaves of at most
// SRT_BVH_LEAF_MAX triangles, nodes emitted in depth-first order with skip links. Runs once
// per srt_update_scene and model instance; ~35 ms for 10^5 triangles on one host core.
struct BvhBuilder {
	struct Tri {
		float lo[3], hi[3], c[3];
		uint32_t j;
	};
	std::vector<Tri> tris;
	// of the last load(): per triangle whether its unpadded box was finite, and the model's extents over the finite ones
	// (FLT_MAX / -FLT_MAX on an axis without any): what the Morton order below is defined over
	std::vector<uint8_t> is_finite;
	float ext_lo[3] = {0, 0, 0}, ext_hi[3] = {0, 0, 0};
	std::vector<BvhNode> &nodes;
	std::vector<uint32_t> &order;
	uint32_t rec_base = 0;
	uint32_t leaves = 0, max_depth = 0;
	uint32_t sah_depth = 48; // below this depth: median splits (0 = a balanced tree, see fold_wide's stack bound)
	int par = 3;             // levels at which build_into gives one half to a thread of its own: up to 8 subtrees at a time (0 = one thread)

	BvhBuilder(std::vector<BvhNode> &n, std::vector<uint32_t> &o) : nodes(n), order(o) {}

	static float half_area(const float lo[3], const float hi[3]) {
		const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
		return dx * dy + dy * dz + dz * dx;
	}
	// the same in double, the extents taken as (double)hi - (double)lo: the measure of the hierarchy's cost (wide_cost below, and
	// srt_refit_cost_kernel in bvh_refit.hip, which evaluates these operations in this order)
	static double half_area_d(const float lo[3], const float hi[3]) {
		const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
		return dx * dy + dy * dz + dz * dx;
	}

	void load(const srt_model &m, const srt_triangle *all);
	struct Stats {
		uint32_t leaves = 0, max_depth = 0;
	};
	Stats build_into(std::vector<BvhNode> &out, uint32_t b, uint32_t e, uint32_t depth, int par);
	uint32_t build(uint32_t b, uint32_t e, uint32_t depth);
	void refit(const srt_model &m, const srt_triangle *all);

	// The wide form of a hierarchy (device_types.h): `c` is the canonical binary form build() leaves (depth-first, the left
	// child directly behind its parent, the right one at the left one's skip link; indices and records relative to the
	// model). An inner block takes the two children of a node and then, while it has room, replaces the child with the
	// largest box by that child's own two (`balanced`: the node's grandchildren, level by level); leaves become leaf
	// blocks. Blocks are appended to `out` (32 dwords each, block indices relative to `out`'s start = the model's first
	// block), `inner` lists the inner ones (their references are shifted when the model is placed in the scene), dest[r]
	// = (leaf block << 2) | slot of record r. Returns the root reference and in `need` the most entries a walk can have
	// waiting at once: every block on the way down leaves at most (children - 1) behind.
	struct Wide {
		std::vector<uint32_t> blocks;
		std::vector<uint32_t> inner;
		std::vector<uint32_t> dest;
		uint32_t root = SRT_BVH_NONE, need = 0;
		struct Job { // an inner block and the nodes of `c` its boxes are quantised from (fold_wide does them on several threads)
			uint32_t self, kids[4], nk, tags, first;
		};
		// One per inner block, children before their parent (fold_node's post-order). Kept with the blocks: an in-place refit
		// (BvhCacheEntry::refit_in_place, and on the device bvh_refit.hip) requantises every inner block from the children it
		// already has. A block's children as BLOCKS are in the block itself: child k is block first + k, a leaf when its tag says so.
		std::vector<Job> jobs;
		// The refit schedule: the inner blocks by height (1 + the highest child's; leaf blocks have height 0), level h in
		// sched[level_off[h - 1], level_off[h]): every block of a level reads only boxes of lower levels. Made when first asked
		// for (ensure_schedule), dropped by fold_wide.
		std::vector<uint32_t> sched, level_off;
		void ensure_schedule();
	};
	static uint32_t fold_node(const std::vector<BvhNode> &c, uint32_t ci, uint32_t self, bool balanced, Wide &w, uint32_t &need);
	static void fold_wide(const std::vector<BvhNode> &c, uint32_t records, bool balanced, Wide &w);
	// The surface-area cost of the wide hierarchy `w` folded over `c`, with c's boxes as they are now:
	//   (sum over inner blocks H(box) * children + sum over leaf blocks H(box) * triangles) / H(root box)
	// A block's box is the union of its children's (an inner block) or its binary leaf node's (a leaf block). 0 = unknown: no
	// hierarchy, a root with H == 0, or a term that is not finite (cost_of).
	static double wide_cost(const std::vector<BvhNode> &c, const Wide &w);
	static double cost_of(double sum, double root_h) { // the quotient, or 0 where it says nothing
		const double q = sum / root_h;
		return root_h > 0.0 && q > 0.0 && q <= 1.7976931348623157e308 ? q : 0.0;
	}
	// cost_now / cost_built; 0 = unknown (either cost is)
	static double cost_ratio(double cost_now, double cost_built) { return cost_now > 0.0 && cost_built > 0.0 ? cost_of(cost_now, cost_built) : 0.0; }

	uint32_t run(const srt_model &m, const srt_triangle *all, uint32_t first_record);

	// ---- the Morton order and the balanced topology (include/srt_abi.h SRT_BUILD_DEVICE; bvh_build.hip sorts by the same codes) ----
	// 30 bits: per axis the centroid's cell of 1024 between the model's extents, x above y above z in every bit triple; an axis
	// whose extent is not a positive finite number gives cell 0. float32, unfused, in this order.
	static uint32_t morton_code(const float c[3], const float mlo[3], const float mhi[3]);
	static constexpr uint32_t MORTON_NONFINITE = 0x40000000u; // a triangle with a non-finite box: behind every finite one
	// after load(): the model's triangles by ascending (code, index)
	void morton_order(std::vector<uint32_t> &out) const;
	// The canonical binary form over `count` records that depends on nothing else: what build_into gives with sah_depth = 0 and
	// without its nth_element -- halves at b + n / 2 down to leaves of at most SRT_BVH_LEAF_MAX records, skip links as run()
	// leaves them. The boxes are zero: a refit fills them in.
	static Stats balanced_topology(uint32_t count, std::vector<BvhNode> &out);
	// ---- the median-split order (include/srt_abi.h SRT_BUILD_ORDER_MEDIAN; bvh_build.hip computes the same, bit for bit) ----
	// 17 bits: the centroid's cell of 65536 between a range's centroid extents `clo` and clo + ext on the range's widest axis; an
	// extent that is not a positive finite number gives cell 0. float32, unfused, in this order.
	static uint32_t median_key(float c, float clo, float ext);
	static constexpr uint32_t MEDIAN_NONFINITE = 0x10000u; // a triangle with a non-finite box: behind every finite one of its range
	// after load(): from the identity, every range of the balanced topology with more than SRT_BVH_LEAF_MAX records sorted stably
	// by key before its halves are visited. A model with too many triangles for the device's composite key
	// (device_types.h srt_build_median_levels) gets the Morton order.
	void median_order(std::vector<uint32_t> &out) const;
};

// One model instance's hierarchy with indices relative to its own first node / first record, kept
// between srt_update_scene calls together with what it was built from: an edit that leaves a model's
// triangles and transform alone (camera, materials, sun, OTHER shapes) re-uses it instead of paying
// the build again (10^5 triangles: 37 ms -> 1.5 ms for the comparison).
struct BvhCacheEntry {
	uint32_t count = 0;
	uint32_t triangle_index = 0; // of the model it was last used for (SRT_DEFORM_REFIT: the same range with other bytes keeps the entry)
	uint64_t tri_hash = 0; // of the triangle bytes: looked at before any memcmp
	bool claimed = false;  // taken by a model of the srt_update_scene in progress
	srt_float4 transform[4];
	std::vector<srt_triangle> tris;
	std::vector<BvhNode> nodes;
	std::vector<uint32_t> order;
	BvhBuilder::Wide wide; // what the device walks, block indices relative to the model's first block
	bool balanced = false; // built without the SAH because the SAH tree could overflow a lane's stack
	uint32_t leaves = 0, depth = 0;
	// BvhBuilder::wide_cost of the hierarchy as build() left it, and of its boxes as they were last known (the host's refits
	// store it; for a stale entry the device's cost kernel reports it, accel_device.hip); 0 = unknown
	double cost_built = 0.0, cost_now = 0.0;
	void build(const srt_model &m, const srt_triangle *all);
	// The hierarchy SRT_BUILD_DEVICE makes, on the host: `order` = the Morton order, the balanced topology of the model's count
	// folded with balanced = true, the boxes of refit_in_place over that order.
	void build_morton(const srt_model &m, const srt_triangle *all);
	// the same over the median-split order (SRT_BUILD_ORDER_MEDIAN)
	void build_median(const srt_model &m, const srt_triangle *all);
	// The part of it that depends on the count alone: nodes and `wide` of the balanced topology (boxes zero, inner blocks not
	// yet quantised), `order` the identity, stale, order_pending. The device sorts and refits (scene_prep.cpp, accel_device.hip).
	void set_balanced_topology(uint32_t n);
	void refit(const srt_model &m, const srt_triangle *all);
	// New boxes for the wide hierarchy AS IT IS FOLDED: the binary boxes as refit() makes them, then every inner block
	// requantised with the children it has. No re-fold, so root, need, dest, order, tags, first and the block count stay
	// (refit() re-folds, and the fold opens children by box area: a rotation can change its topology). The host statement
	// of what bvh_refit.hip computes on the device.
	void refit_in_place(const srt_model &m, const srt_triangle *all);
	// The model moved under SRT_REFIT_DEVICE: `transform` is the new one, the boxes of `nodes` and `wide.blocks` are those of
	// an earlier one. Whatever is uploaded from a stale entry is refitted on the device behind the upload; build() and
	// refit() recompute everything from the triangles and clear the mark.
	bool stale = false;
	// Built on the device by the srt_update_scene before: `order` is still the identity, the sorted one is on its way back
	// (accel_device.hip srt_accel_build_consume waits for the copy before the next host pass looks at any entry).
	bool order_pending = false;
	bool same_triangles(const srt_model &m, const srt_triangle *all, uint64_t hash) const {
		return m.num_triangles == count && hash == tri_hash && memcmp(tris.data(), all + m.triangle_index, (size_t)count * sizeof(srt_triangle)) == 0;
	}
	bool same_transform(const srt_model &m) const { return memcmp(transform, m.transform, sizeof transform) == 0; }
};

// the hierarchies of the previous srt_update_scene; a handle owns one (srt_tracer::bvh_cache), made when first needed
struct BvhCache {
	std::vector<BvhCacheEntry> entries;
	// SRT_BUILD_DEVICE: the balanced topologies of the last few triangle counts, the most recent first (entries without
	// triangles or order: set_balanced_topology's result, copied into the model's entry)
	std::vector<BvhCacheEntry> topologies;
	const BvhCacheEntry &balanced_topology(uint32_t count);
};

uint64_t hash_triangles(const srt_triangle *tris, size_t count);

#endif
