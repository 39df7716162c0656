// trace_body.inc -- the body of the trace kernel: kernels.hip includes this text inside srt_trace_kernel (SC = GeneralScene)
// and inside srt_trace_scene_kernel (SC = OneGroupScene<CODE, NO_SPEC>; COUNT_TRIS, HAS_MODELS, USE_BVH false and USE_LDS true
// there), after the tunables and helpers it uses (kernels.hip; device_math.h, device_intersect.h, device_shading.h). It is
// included, not called: the general kernels must compile to what they were before scene classes existed, and a body that is
// inlined from a function does not (the inliner's alias scopes reorder the code). kernels.hip "SCENE CLASSES".
	extern __shared__ float4 lds[]; // [2*n_shapes] winner records, [4*n_materials] materials, (sphere / plane scenes: group headers, shape blocks,) sky ring, hit queue
	constexpr bool FAST = SC::FAST;
	static_assert(!FAST || (USE_LDS && !HAS_MODELS && !USE_BVH && !COUNT_TRIS), "scene classes exist for sphere / plane scenes staged in LDS");
	// OneGroupScene: shapes per block, the first shape of each, and the scene's LDS layout with the blocks in front of the
	// materials, [2*N] winner records, [12] shape blocks, [4*n_materials] materials: every address but a material's is a constant
	constexpr uint32_t FK0 = SC::CODE & 255u, FK1 = (SC::CODE >> 8) & 255u, FK2 = (SC::CODE >> 16) & 255u;
	constexpr int FN0 = (int)((FK0 >> 2) & 7u), FN1 = (int)((FK1 >> 2) & 7u), FN2 = (int)((FK2 >> 2) & 7u), FN = FN0 + FN1 + FN2;
	// an axis twin: the plane form, and each block's two slots of it (device_types.h "Axis planes"; 0 everywhere else)
	constexpr uint32_t AXES = SC::AXES, FA0 = AXES & 15u, FA1 = (AXES >> 4) & 15u, FA2 = (AXES >> 8) & 15u;
	constexpr uint32_t SUB = USE_BVH ? SRT_SUB_BVH : HAS_MODELS ? SRT_SUB_MODELS : SRT_SUB_PLAIN;
	const int width = p.rd.width;
	const int lane = threadIdx.x;
	const int ns = p.rd.num_samples;
	const int nb = p.rd.num_bounces;
	const int n_shapes = FAST ? FN : p.sd.num_shapes;
	const bool all_materials_ok = FAST || p.all_materials_ok != 0;
	const bool unit_materials = FAST || p.unit_materials != 0; // the materials carry integer thresholds in place of their three probabilities (bernoulli)
	const bool no_specular = FAST ? SC::NO_SPEC : (p.material_flags & (SRT_MF_NO_SPECULAR | SRT_MF_PLAIN_COLORS)) == (SRT_MF_NO_SPECULAR | SRT_MF_PLAIN_COLORS); // (wave-uniform) see SHADE
	const BlockGroup *__restrict__ runs = p.runs;
	const float *__restrict__ run_data = p.run_data;
	const float *__restrict__ wtris = p.wtris;

	if (FAST) {
		const float4 *__restrict__ gw = reinterpret_cast<const float4 *>(p.winners);
		const float4 *__restrict__ gm = reinterpret_cast<const float4 *>(p.materials);
		const float4 *__restrict__ gd4 = reinterpret_cast<const float4 *>(p.run_data);
		static_assert(2 * FN <= 64, "one pass stages the winner records");
		if (lane < 2 * FN) lds[lane] = gw[lane];
		if (lane < 12) lds[2 * FN + lane] = gd4[lane];
		for (int i = threadIdx.x; i < 4 * p.num_materials; i += 64) lds[2 * FN + 12 + i] = gm[i];
		__syncthreads();
	} else if (USE_LDS) {
		const float4 *__restrict__ gw = reinterpret_cast<const float4 *>(p.winners);
		const float4 *__restrict__ gm = reinterpret_cast<const float4 *>(p.materials);
		for (int i = threadIdx.x; i < 2 * n_shapes; i += 64) lds[i] = gw[i];
		for (int i = threadIdx.x; i < 4 * p.num_materials; i += 64) lds[2 * n_shapes + i] = gm[i];
		if (!HAS_MODELS) { // sphere / plane scenes: group headers and shape blocks too (see EXTEND)
			const float4 *__restrict__ gh4 = reinterpret_cast<const float4 *>(p.runs);
			const float4 *__restrict__ gd4 = reinterpret_cast<const float4 *>(p.run_data);
			float4 *__restrict__ dst = lds + 2 * n_shapes + 4 * p.num_materials;
			for (int i = threadIdx.x; i < p.num_runs; i += 64) dst[i] = gh4[i];
			for (int i = threadIdx.x; i < 12 * p.num_runs; i += 64) dst[p.num_runs + i] = gd4[i];
		}
		__syncthreads();
	}
	// header of the shape group EXTEND tests next; group 0 to begin with (sphere / plane scenes read their shape blocks from LDS)
	uint32_t gh_code = 0;
	int gh_f0 = 0, gh_f1 = 0, gh_f2 = 0;
	if (!FAST && USE_LDS && !HAS_MODELS && p.num_runs > 0) {
		const float4 hv = lds[2 * n_shapes + 4 * p.num_materials];
		gh_code = (uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(hv.x));
		gh_f0 = __builtin_amdgcn_readfirstlane((int)f2u(hv.y)), gh_f1 = __builtin_amdgcn_readfirstlane((int)f2u(hv.z));
		gh_f2 = __builtin_amdgcn_readfirstlane((int)f2u(hv.w));
	}

	// ---- work distribution: one work-item = one (pixel, sample) path -------------------
	// Items of this dispatch: item = q * batch_samples + k, q = packed owned pixel (row-major),
	// sample = first_sample + k; fewer than 2^32 per launch (the host sizes sample batches so).
	// Consecutive items are consecutive samples of one pixel, so the 64 lanes of a wave start out
	// on (nearly) the same camera ray. Persistent waves reserve chunks of p.job_items items from
	// ONE global cursor (the first chunk of a wave is its own: chunk number = workgroup number, so
	// thousands of waves starting together do not queue up on one atomic) and work through them in
	// sub-jobs of SUB items. srt_reduce_kernel adds the radiances up per pixel in sample order.
	const uint32_t total_items = (uint32_t)p.total_items;
	const uint32_t nbs = p.batch_samples;
	const unsigned long long own_chunks_end = (unsigned long long)gridDim.x * p.job_items;
	uint32_t chunk_cur = 0, chunk_end = 0; // wave-uniform
	if ((unsigned long long)blockIdx.x * p.job_items < (unsigned long long)total_items) {
		chunk_cur = blockIdx.x * p.job_items;
		chunk_end = (total_items - chunk_cur < p.job_items) ? total_items : chunk_cur + p.job_items;
	}
	bool queue_dry = (total_items == 0);
	// the sub-job being handed out (wave-uniform): items [sj_next, sj_end); sj_next is sample sj_off of packed pixel sj_qpix
	uint32_t sj_next = 0, sj_end = 0, sj_off = 0, sj_qpix = 0;
	float *__restrict__ ring = reinterpret_cast<float *>(lds + p.stage_off); // [10][64] escaped paths awaiting their sky lookup
	float *__restrict__ hq = ring + 10u * (uint32_t)SRT_RING_CAP; // [hq_fields][HQ] paths that hit, awaiting their bounce (FIFO)
	constexpr uint32_t HQ = USE_BVH ? SRT_HQ_CAP_BVH : HAS_MODELS ? SRT_HQ_CAP_MODELS : SRT_HQ_CAP;
	// Scene classes: what a camera ray's tests make from a shape and the camera's origin alone, once per wave (device_intersect.h
	// "CAMERA PHASES"): the spheres' records {L, c} behind the hit queue, a plane's num in the staged block itself.
	constexpr uint32_t CS1 = srt_class_cam_records(FK0), CS2 = srt_class_cam_records(FK0 | (FK1 << 8)); // first record of block 1 / 2
	float4 *__restrict__ cam_rec = reinterpret_cast<float4 *>(hq + hq_fields(HAS_MODELS) * HQ);
	if (FAST) {
		const auto &c = SRT_COLD(p);
		const f3 cam_org = mk(c.rd.camera_to_world[3].x, c.rd.camera_to_world[3].y, c.rd.camera_to_world[3].z); // as CAMERA loads it
		cam_records_of_block<FK0>(lds + 2 * FN, cam_rec, cam_org, lane);
		cam_records_of_block<FK1>(lds + 2 * FN + 4, cam_rec + CS1, cam_org, lane);
		cam_records_of_block<FK2>(lds + 2 * FN + 8, cam_rec + CS2, cam_org, lane);
		if constexpr (AXES != 0u) {
			cam_axis_numerators<FK0, FA0>(lds + 2 * FN, cam_org, lane);
			cam_axis_numerators<FK1, FA1>(lds + 2 * FN + 4, cam_org, lane);
			cam_axis_numerators<FK2, FA2>(lds + 2 * FN + 8, cam_org, lane);
		}
		__syncthreads();
	}
	// Axis twins (device_intersect.h "AXIS PLANES"): whether the camera's own numerators are inside the guard's box is the same for
	// every camera phase of the launch; its EXTEND phases and those that failed the guard are counted (srt_debug_counters [10], [11])
	bool cam_nums_ok = false; // (wave-uniform)
	uint32_t w_axis_phases = 0, w_axis_failed = 0;
	if constexpr (AXES != 0u) {
		const float4 *__restrict__ lb = lds + 2 * FN;
		float mn = DM_INF_F, sm = 0.0f;
#pragma unroll
		for (int b = 0; b < 3; b++)
#pragma unroll
			for (int i = 0; i < 2; i++)
				if (((AXES >> (4 * b + 2 * i)) & 3u) != 0u) {
					const float a = dm_fabs(reinterpret_cast<const float *>(lb + 4 * b + 2 * i + 1)[3]);
					mn = __builtin_fminf(mn, a), sm = sm + a;
				}
		cam_nums_ok = !any64(!(mn >= 0x1p-60f && sm <= 0x1p50f));
	}
	// NO_SPEC classes (device_shading.h "DIFFUSE WAVES"): SHADE phases are counted, those that ran no per-lane bounce (the short form; or
	// all lanes plain diffuse and on their last bounce, which run no bounce at all) and those whose lanes were all plain diffuse but
	// failed the operand guard (srt_debug_counters [7], [12], [13])
	constexpr bool DIFFUSE_WAVE = FAST && SC::NO_SPEC;
	uint32_t w_diffuse_short = 0, w_diffuse_failed = 0;
	bool cam_phase = false;  // (wave-uniform) every lane of actm took its ray in the REFILL just before: EXTEND runs the camera forms
	unsigned long long w_cam = 0; // diagnostics: such phases << 36 | the rays in them (srt_debug_counters; good for some 8 full-size frames between resets)
#ifdef SRT_REGION_COUNT
	uint32_t *region_ctr = reinterpret_cast<uint32_t *>(hq + hq_fields(HAS_MODELS) * HQ);
	for (int i = lane; i < 2 * SRT_REGION_MAX; i += 64) region_ctr[i] = 0u;
	__syncthreads();
#endif
	// Array-scan kernels: rays waiting for the triangle scan of a big model. A scan costs the wave its triangle count whether
	// one lane takes part or all 64, so a scan is started for a FULL wave of rays only. Every persistent wave owns, in HBM
	// (device_types.h SRT_SCAN_QUEUE_FLOATS):
	//   two scan stacks of SQ records x 20 fields -- the ray with everything closest_intersection has found so far and the
	//   block it continues at; big model number k of the scene uses stack k & 1, so that the rays one stack gives back all
	//   scan the same model (a scene of one or two big models; with more, a stack mixes models and its scans are less full);
	//   one park stack of PK records x 15 fields -- rays that were about to set out when the wave took a scan stack back.
	// In LDS the stacks would cost the kernel most of its waves; a record is written and read once per triangle scan of at
	// least 128 triangles -- microseconds of memory latency against tens of microseconds of scanning. Stores are plain
	// (write-through), loads bypass the vector L1 (a slot is reused, and the L1 keeps no track of this CU's own stores) and
	// wait for the wave's stores first (REFILL below).
	constexpr bool SUSPEND = HAS_MODELS && !USE_BVH;
	constexpr uint32_t SQ = (uint32_t)SRT_SQ_CAP, PK = (uint32_t)SRT_PK_CAP;
	float *__restrict__ sq_base = SUSPEND ? const_cast<float *>((const float *)SRT_COLD(p).scan_queue) + (size_t)SRT_POOL_CTL_WORDS + (SRT_COLD(p).pool_blocks != 0u ? SRT_POOL_REC_FLOATS : (size_t)0) + (size_t)blockIdx.x * (size_t)SRT_SCAN_QUEUE_FLOATS : nullptr;
	float *__restrict__ pk = sq_base + 2u * 20u * SQ;
	uint32_t sq_count0 = 0, sq_count1 = 0, pk_count = 0; // wave-uniform
	// The END of a launch: a wave that has run out of camera rays holds a remainder of fewer than 64 rays per stack, and every
	// triangle scan for them would run with idle lanes -- in 5,000 waves at once, and again after each of their bounces. The
	// waves pool these rays instead (TraceParams.pool_*, one pool per stack): a wave with nothing else left hands its remainder
	// in, then takes a full block of 64 out if there is one, else leaves. The last wave to leave takes what is left.
	// Nobody waits for anybody: a block is taken only once its 64 records have been published. Waves of different XCDs meet
	// here, whose L2s do not see each other's lines: records and radiances go through sc1 (write-through) stores, acknowledged
	// (s_waitcnt vmcnt(0)) before the agent-scope atomic add that publishes them, and are read with sc1 loads -- no cache
	// write-back or invalidation, which cost microseconds apiece and would be paid by every wave at every hand-over.
	const bool use_pool = SUSPEND && SRT_COLD(p).pool_blocks != 0u;
	bool pool_leave = false, pool_last = false; // wave-uniform: this wave has signed off / is the last one and clears the pool
	uint32_t w_pool_taken = 0, w_pool_given = 0, w_pool_last_taken = 0; // diagnostics: blocks taken out, records handed in, blocks taken as the last wave
	uint32_t ring_count = 0, hq_head = 0, hq_count = 0;                        // wave-uniform

	f3 org = mk(0.f, 0.f, 0.f), dir = mk(0.f, 0.f, 0.f), mask = mk(1.f, 1.f, 1.f), color = mk(0.f, 0.f, 0.f);
	uint32_t seed = 0;
	uint32_t item = 0;
	int bounce = 0;
	int best = -1;
	uint32_t best_tri = 0; // index inside the model; with a BVH: (leaf block << 2) | slot
	BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1]; // per lane, in scratch memory (walk_bvh)
	const float4 *__restrict__ bvh_blocks = reinterpret_cast<const float4 *>(p.bvh_blocks);
	unsigned long long actm = 0ull; // (wave-uniform) the lanes that hold a ray awaiting closest_intersection
	unsigned long long resm = 0ull; // (wave-uniform) SUSPEND: of those, the rays taken back from a scan stack or the pool, which scan the model of their block `pos` now
	float tmin = DM_INF_F; // closest hit so far of the ray under way (kept across a suspension)
	uint32_t pos = 0;      // SUSPEND: first shape block this ray still has to see (0 = a fresh ray)
	// rays / sky / paths are counted per WAVE with popcounts of the exec mask (scalar adds, no
	// VGPRs); only the instrumented triangle counters stay per lane.
	// (paths and sky lookups of a wave stay below the launch's 2^32 items; iterations are diagnostics)
	unsigned long long w_rays = 0;
	uint32_t w_sky = 0, w_paths = 0, w_iter = 0, w_shade = 0;
	uint32_t w_scans = 0, w_scan_lanes = 0; // SUSPEND diagnostics, per lane: triangle scans of big models this lane led / took part in
	uint32_t n_tri = 0, n_tri_u = 0;
	uint32_t idle_spins = 0;
	// SHADE runs when hits + queued paths exceed this: a full wave (or more than the queue holds); anything at all once the work cursor is dry
	constexpr uint32_t SHADE_THR = ((uint32_t)SRT_SHADE_MIN - 1u) < HQ ? ((uint32_t)SRT_SHADE_MIN - 1u) : HQ;
	uint32_t shade_thr = queue_dry ? 0u : SHADE_THR;

	SRT_CLK_DECL;
	SRT_REGION(PROLOGUE);
	for (;;) {
		SRT_REGION(LOOP_HEAD);
		unsigned long long hitm = 0ull, missm = 0ull, finm = 0ull; // (wave-uniform) lanes whose ray hit / escaped, whose path ended in this iteration
		uint32_t susp = 0u; // SUSPEND, per lane: 1 + the scan stack the lane's ray went to in this iteration
		int key = -1;       // per lane: >= 0 when the ray hit a shape that has a material
		if (SRT_DIAG_ON) w_iter++;
		SRT_CLK(6);
#ifdef SRT_DUMMY_KIND
#include "issue_probe.h" // (regime probe, development builds only: 100 extra instructions of one kind per loop iteration)
#endif
		// ================= EXTEND: closest_intersection (render.cl:293-378), winner deferred =================
		if (actm != 0ull) {
			constexpr bool MASKED = HAS_MODELS;
			if (!FAST && nb <= 0) { // render.cl:403: no bounce loop at all -> colour 0
				finm = actm;
			} else {
				w_rays += SUSPEND ? popc64(actm & ~resm) : popc64(actm); // a resumed ray was counted when it set out
				const bool resumed = SUSPEND ? in_mask(resm) : false;
				// Sphere / plane scenes: the tests run for all 64 lanes, the lanes without a ray compute on whatever they hold and are
				// sorted out by `actm` afterwards -- no exec-mask bookkeeping around the phase. (With models a lane without a ray must
				// not scan or walk.)
				if (!MASKED || in_mask(actm)) {
					SRT_REGION(EXTEND_SETUP);
					{
						if (!SUSPEND || !resumed) {
							tmin = DM_INF_F;
							best = -1;
							best_tri = 0;
							pos = 0;
						}
						bool part = true;       // SUSPEND: false once the ray has gone to the scan queue
						uint32_t sq_pushed0 = 0, sq_pushed1 = 0; // records pushed by this EXTEND phase so far. Uniform among the lanes in here only:
						                                          // the counts, which the lanes outside this branch read too, are brought up to date after it
						f3 inv = mk(0.f, 0.f, 0.f);
						if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);

					// Groups of three 64-byte blocks of same-type shapes, in array order (device_types.h). The header and
					// the three blocks of a group are fetched with four scalar loads issued together: one scalar-memory
					// round trip per group (a 7-shape scene is one group). The mesh kernels, whose triangle loops need
					// the scalar registers, fetch the blocks of a group one by one instead.
					auto test_block = [&](const Blk16 &b, uint32_t code, int base, uint32_t bidx, int slot) {
						const uint32_t type1 = code & 3u; // shape type + 1; 0 = no block
						const bool on = !SUSPEND || (part && bidx >= pos);
						if (type1 == SRT_SHAPE_SPHERE + 1u) {
							if (on) {
								// (wave-uniform) a run's last block may hold one or two spheres: the fillers' tests are skipped
								if (((code >> 2) & 7u) <= 2u) {
									SRT_REGION_SLOT(EXTEND_SPHERES2, slot);
									test_spheres<2>(b, org, dir, base, tmin, best);
								} else {
									SRT_REGION_SLOT(EXTEND_SPHERES4, slot);
									test_spheres<4>(b, org, dir, base, tmin, best);
								}
							}
						} else if (type1 == SRT_SHAPE_PLANE + 1u) {
							if (on) {
								SRT_REGION_SLOT(EXTEND_PLANES, slot);
								test_planes2(b, (code >> 2) & 7u, org, dir, base, tmin, best);
							}
						} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
							SRT_REGION_SLOT(EXTEND_MODEL, slot);
							// the model's own box first, exactly as the reference (render.cl:316-323), then its triangles
							const bool enter0 = on && test_aabb(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], org, inv, tmin);
							bool scan0 = enter0;
							if (SUSPEND && ((code >> 5) & 1u)) {
								// A big model. Few of a wave's rays enter its box at a time; scanning 10^5 triangles for them would
								// leave the other lanes idle. Those rays wait in the model's scan stack -- with everything
								// closest_intersection has found so far, so that they continue exactly where they left -- until a wave-full
								// has gathered. The scan runs now when the wave holds rays that were taken back for THIS block (a ray that
								// has scanned one big model and enters the next one's box waits again), or when the stack is full.
								const unsigned long long want = ballot64(enter0);
								const uint32_t n_want = (uint32_t)__popcll(want);
								const uint32_t sid = (code >> 6) & 1u; // (wave-uniform) the model's stack
								const uint32_t held = sid ? sq_count1 + sq_pushed1 : sq_count0 + sq_pushed0;
								const bool now = held + n_want > SQ || any64(enter0 && resumed && pos == bidx);
								if (!now) {
									if (enter0) {
										SRT_REGION(EXTEND_SUSPEND);
										float *__restrict__ sq = sq_base + sid * (20u * SQ);
										const uint32_t e = held + __builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
										sq[0 * SQ + e] = org.x, sq[1 * SQ + e] = org.y, sq[2 * SQ + e] = org.z;
										sq[3 * SQ + e] = dir.x, sq[4 * SQ + e] = dir.y, sq[5 * SQ + e] = dir.z;
										sq[6 * SQ + e] = mask.x, sq[7 * SQ + e] = mask.y, sq[8 * SQ + e] = mask.z;
										sq[9 * SQ + e] = color.x, sq[10 * SQ + e] = color.y, sq[11 * SQ + e] = color.z;
										sq[12 * SQ + e] = dm_u2f(seed), sq[13 * SQ + e] = dm_u2f((uint32_t)bounce), sq[14 * SQ + e] = dm_u2f(item);
										sq[15 * SQ + e] = tmin, sq[16 * SQ + e] = dm_u2f((uint32_t)best), sq[17 * SQ + e] = dm_u2f(best_tri);
										sq[18 * SQ + e] = dm_u2f(bidx);
										part = false;
										susp = 1u + sid;
									}
									if (sid) sq_pushed1 += n_want;
									else sq_pushed0 += n_want;
									scan0 = false;
								}
							}
							if (SUSPEND && !COUNT_TRIS && ((code >> 5) & 1u)) {
								// per LANE (this is divergent code): summed over the wave at the end
								const unsigned long long sb = ballot64(scan0);
								if (scan0) {
									w_scan_lanes++;
									if ((sb & ((1ull << lane) - 1ull)) == 0ull) w_scans++; // the scan's first lane counts the scan
								}
							}
							if (scan0) {
								if (USE_BVH) {
									walk_bvh<COUNT_TRIS>(bvh_blocks, bvh_stack, f2u(b.v[3]), org, dir, base, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
								} else {
									if (COUNT_TRIS) n_tri += f2u(b.v[7]);
									test_triangles<COUNT_TRIS>(wtris, f2u(b.v[3]), f2u(b.v[7]), org, dir, base, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
								}
							}
							if (((code >> 2) & 7u) > 1u && on && test_aabb(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], org, inv, tmin)) {
								if (USE_BVH) {
									walk_bvh<COUNT_TRIS>(bvh_blocks, bvh_stack, f2u(b.v[11]), org, dir, base + 1, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
								} else {
									if (COUNT_TRIS) n_tri += f2u(b.v[15]);
									test_triangles<COUNT_TRIS>(wtris, f2u(b.v[11]), f2u(b.v[15]), org, dir, base + 1, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
								}
							}
						}
					};
					const int n_groups = FAST ? 0 : p.num_runs;
					if (FAST) {
						// OneGroupScene: the three blocks of the one group, straight-line (the same tests in the same order)
						const float4 *__restrict__ lb = lds + 2 * FN;
						auto ld_lds = [&](int k) {
							Blk16 b;
							const float4 q0 = lb[4 * k], q1 = lb[4 * k + 1], q2 = lb[4 * k + 2], q3 = lb[4 * k + 3];
							b.v[0] = q0.x, b.v[1] = q0.y, b.v[2] = q0.z, b.v[3] = q0.w, b.v[4] = q1.x, b.v[5] = q1.y, b.v[6] = q1.z, b.v[7] = q1.w;
							b.v[8] = q2.x, b.v[9] = q2.y, b.v[10] = q2.z, b.v[11] = q2.w, b.v[12] = q3.x, b.v[13] = q3.y, b.v[14] = q3.z, b.v[15] = q3.w;
							return b;
						};
						if constexpr (AXES != 0u) {
							// An axis twin: one guard for the phase's planes, voted over the lanes that hold a ray; a wave that passes runs the
							// folded plane tests, any other today's forms below (device_intersect.h "AXIS PLANES").
							constexpr int NP0 = (FK0 & 3u) == SRT_SHAPE_PLANE + 1u ? FN0 : 0, NP1 = (FK1 & 3u) == SRT_SHAPE_PLANE + 1u ? FN1 : 0;
							constexpr int NP2 = (FK2 & 3u) == SRT_SHAPE_PLANE + 1u ? FN2 : 0, NP = NP0 + NP1 + NP2;
							w_axis_phases++;
							if (cam_phase) {
								w_cam += (1ull << 36) + popc64(actm);
								const float one[1] = {1.0f}; // (the numerators were looked at once, in the prologue: cam_nums_ok)
								const bool pass = cam_nums_ok && (ballot64(!axis_operands_ok<1>(one, dir)) & actm) == 0ull;
								w_axis_failed += pass ? 0u : 1u;
								test_block_of_class_axis_cam<FK0, FA0>(lb, cam_rec, pass, 0, dir, actm, tmin, best);
								if (FK1 != 0u) test_block_of_class_axis_cam<FK1, FA1>(lb + 4, cam_rec + CS1, pass, FN0, dir, actm, tmin, best);
								if (FK2 != 0u) test_block_of_class_axis_cam<FK2, FA2>(lb + 8, cam_rec + CS2, pass, FN0 + FN1, dir, actm, tmin, best);
							} else {
								const float *__restrict__ lbf = reinterpret_cast<const float *>(lb);
								float an[NP > 0 ? NP : 1];
								axis_numerators<FK0, FA0>(lbf, org, an);
								axis_numerators<FK1, FA1>(lbf + 16, org, an + NP0);
								axis_numerators<FK2, FA2>(lbf + 32, org, an + NP0 + NP1);
								const bool pass = (ballot64(!axis_operands_ok<NP>(an, dir)) & actm) == 0ull;
								w_axis_failed += pass ? 0u : 1u;
								test_block_of_class_axis<FK0, FA0>(lb, pass, an, 0, org, dir, tmin, best);
								if (FK1 != 0u) test_block_of_class_axis<FK1, FA1>(lb + 4, pass, an + NP0, FN0, org, dir, tmin, best);
								if (FK2 != 0u) test_block_of_class_axis<FK2, FA2>(lb + 8, pass, an + NP0 + NP1, FN0 + FN1, org, dir, tmin, best);
							}
						} else if (cam_phase) {
							// (wave-uniform) fresh camera rays only: the same tests in the same order from the prologue's numbers
							w_cam += (1ull << 36) + popc64(actm);
							test_block_of_class_cam<FK0>(lb, cam_rec, 0, dir, actm, tmin, best);
							if (FK1 != 0u) test_block_of_class_cam<FK1>(lb + 4, cam_rec + CS1, FN0, dir, actm, tmin, best);
							if (FK2 != 0u) test_block_of_class_cam<FK2>(lb + 8, cam_rec + CS2, FN0 + FN1, dir, actm, tmin, best);
						} else {
							test_block_of_class<FK0>(ld_lds(0), 0, org, dir, tmin, best);
							if (FK1 != 0u) test_block_of_class<FK1>(ld_lds(1), FN0, org, dir, tmin, best);
							if (FK2 != 0u) test_block_of_class<FK2>(ld_lds(2), FN0 + FN1, org, dir, tmin, best);
						}
					}
					for (int g = 0; g < n_groups; g++) {
						SRT_REGION(EXTEND_GROUP);
						float gh[4];
						ld_uniform<4, 16>(reinterpret_cast<const float *>(runs + g), gh);
						const uint32_t code = f2u(gh[0]);
						const float *__restrict__ gd = run_data + 48 * g;
						if (!HAS_MODELS && USE_LDS) {
							// Small sphere / plane scenes: the blocks were staged in LDS with the winner records. All lanes read the same
							// address (a broadcast: no bank conflicts) and get the shape data in VGPRs; measured, the scalar-cache
							// round trip of the path below costs a wave ~750 cycles per segment, an LDS read a fraction of that.
							const float4 *__restrict__ lgh = lds + 2 * n_shapes + 4 * p.num_materials;
							const float4 *__restrict__ lb = lgh + n_groups + 12 * g;
							// The header of the group under test lives in scalar registers (gh_*): read BEHIND the previous group's tests, for
							// the group that comes next -- and never again in a scene of one group (up to 12 spheres / 6 planes), whose
							// first block's reads so start at once instead of behind a header read, a wait and four v_readfirstlane.
							const uint32_t lcode = gh_code;
							const int f0 = gh_f0, f1 = gh_f1, f2 = gh_f2;
							auto ld_lds = [&](int k) {
								Blk16 b;
								const float4 q0 = lb[4 * k], q1 = lb[4 * k + 1], q2 = lb[4 * k + 2], q3 = lb[4 * k + 3];
								b.v[0] = q0.x, b.v[1] = q0.y, b.v[2] = q0.z, b.v[3] = q0.w, b.v[4] = q1.x, b.v[5] = q1.y, b.v[6] = q1.z, b.v[7] = q1.w;
								b.v[8] = q2.x, b.v[9] = q2.y, b.v[10] = q2.z, b.v[11] = q2.w, b.v[12] = q3.x, b.v[13] = q3.y, b.v[14] = q3.z, b.v[15] = q3.w;
								return b;
							};
							test_block(ld_lds(0), lcode & 255u, f0, 0u, 0);
							if ((lcode >> 8) & 255u) test_block(ld_lds(1), (lcode >> 8) & 255u, f1, 0u, 1);
							if ((lcode >> 16) & 255u) test_block(ld_lds(2), (lcode >> 16) & 255u, f2, 0u, 2);
							int ng = n_groups;
							asm volatile("" : "+s"(ng)); // (not to be recognised as loop-invariant: unswitching would duplicate the whole loop)
							if (ng > 1) {
								const float4 hv = lgh[g + 1 < n_groups ? g + 1 : 0];
								gh_code = (uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(hv.x));
								gh_f0 = __builtin_amdgcn_readfirstlane((int)f2u(hv.y)), gh_f1 = __builtin_amdgcn_readfirstlane((int)f2u(hv.z));
								gh_f2 = __builtin_amdgcn_readfirstlane((int)f2u(hv.w));
							}
						} else if (!HAS_MODELS) {
							const Blk16 b0 = ld_blk16(gd), b1 = ld_blk16(gd + 16), b2 = ld_blk16(gd + 32);
							test_block(b0, code & 255u, (int)f2u(gh[1]), 0u, 0);
							test_block(b1, (code >> 8) & 255u, (int)f2u(gh[2]), 0u, 1);
							test_block(b2, (code >> 16) & 255u, (int)f2u(gh[3]), 0u, 2);
						} else {
							test_block(ld_blk16(gd), code & 255u, (int)f2u(gh[1]), 3u * g, 0);
							if ((code >> 8) & 255u) test_block(ld_blk16(gd + 16), (code >> 8) & 255u, (int)f2u(gh[2]), 3u * g + 1u, 1);
							if ((code >> 16) & 255u) test_block(ld_blk16(gd + 32), (code >> 16) & 255u, (int)f2u(gh[3]), 3u * g + 2u, 2);
						}
					}
					SRT_REGION(EXTEND_FINISH);
						if (!SUSPEND || part) { // else: the ray waits in the scan queue, with all of its state
							// a shape without a material counts as a miss (render.cl:404: material_index >= 0)
							key = best;
							if (!all_materials_ok) { // (wave-uniform; else every shape of the scene has a material: closest shape = hit)
								key = -1;
								if (best >= 0) key = USE_LDS ? (int)f2u(reinterpret_cast<const float *>(lds)[8 * best + 1]) : p.winners[best].material;
							}
							if (!MASKED) org = org + dir * tmin; // (a lane that hit nothing, or held no ray, has no further use for its origin)
							else if (key >= 0) org = org + dir * tmin; // rayhit->position (render.cl:312,343,362)
						}
					}
				}
				// wave-uniform again
				hitm = ballot64(key >= 0) & actm;
				missm = actm & ~hitm;
				if (SUSPEND) {
					const unsigned long long s0 = ballot64(susp == 1u), s1 = ballot64(susp == 2u); // went to scan stack 0 / 1: neither hit nor escaped yet
					sq_count0 += popc64(s0), sq_count1 += popc64(s1);
					missm &= ~(s0 | s1);
					resm = 0ull;
				}
			}
			actm = 0ull;
		}

		SRT_CLK(0);
		// ---- escaped paths queue for the sky (wave-uniform control flow) ----
		if (missm != 0ull) {
			SRT_REGION(SKY_PUSH);
			constexpr uint32_t RC = SRT_RING_CAP;
			const uint32_t n_miss = popc64(missm);
			const uint32_t rank = lane_rank(missm);
			if (ring_count + n_miss > RC) { // does not fit: the sky lookups of what is queued first (ring_count lanes busy)
				resolve_ring(p, ring, ring_count, lane SRT_RC_ARG);
				ring_count = 0;
			}
			if (RC == 64u) {
				// an empty ring holds a whole wave's escapes: one round, no loop
				if (in_mask(missm)) {
					const uint32_t e = ring_count + rank;
					ring[0 * RC + e] = dir.x, ring[1 * RC + e] = dir.y, ring[2 * RC + e] = dir.z;
					ring[3 * RC + e] = mask.x, ring[4 * RC + e] = mask.y, ring[5 * RC + e] = mask.z;
					ring[6 * RC + e] = color.x, ring[7 * RC + e] = color.y, ring[8 * RC + e] = color.z;
					ring[9 * RC + e] = dm_u2f(item);
				}
				ring_count += n_miss;
			} else {
				const bool missed = in_mask(missm);
				uint32_t done = 0;
				while (done < n_miss) { // more lanes may have escaped than the ring holds
					const uint32_t take = (RC - ring_count) < (n_miss - done) ? (RC - ring_count) : (n_miss - done);
					if (missed && rank >= done && rank < done + take) {
						const uint32_t e = ring_count + (rank - done);
						ring[0 * RC + e] = dir.x, ring[1 * RC + e] = dir.y, ring[2 * RC + e] = dir.z;
						ring[3 * RC + e] = mask.x, ring[4 * RC + e] = mask.y, ring[5 * RC + e] = mask.z;
						ring[6 * RC + e] = color.x, ring[7 * RC + e] = color.y, ring[8 * RC + e] = color.z;
						ring[9 * RC + e] = dm_u2f(item);
					}
					ring_count += take;
					done += take;
					if (done < n_miss) {
						resolve_ring(p, ring, ring_count, lane SRT_RC_ARG);
						ring_count = 0;
					}
				}
			}
			w_sky += n_miss;
		}

		SRT_CLK(1);
		// ================= SHADE or PARK =================
		const uint32_t n_hit = popc64(hitm);
		const uint32_t n_ready = n_hit + hq_count;
		if (n_ready > shade_thr) {
			SRT_REGION(SHADE_HEAD);
			unsigned long long shm = hitm; // the lanes that shade: those with a hit, and the free ones that take the oldest waiting paths
			const uint32_t n_free_s = 64u - n_hit;
			const uint32_t n_pop = n_free_s < hq_count ? n_free_s : hq_count;
			if (n_pop != 0u) {
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
				const unsigned long long fb = ~hitm;
				const uint32_t rank = lane_rank(fb);
				const unsigned long long popm = ballot64(rank < n_pop) & fb;
				if (in_mask(popm)) {
					SRT_REGION(SHADE_POP);
					uint32_t e = hq_head + rank;
					e = e >= HQ ? e - HQ : e;
					org = mk(hq[0 * HQ + e], hq[1 * HQ + e], hq[2 * HQ + e]);
					dir = mk(hq[3 * HQ + e], hq[4 * HQ + e], hq[5 * HQ + e]);
					mask = mk(hq[6 * HQ + e], hq[7 * HQ + e], hq[8 * HQ + e]);
					color = mk(hq[9 * HQ + e], hq[10 * HQ + e], hq[11 * HQ + e]);
					seed = dm_f2u(hq[12 * HQ + e]);
					best = (int)dm_f2u(hq[13 * HQ + e]);
					bounce = (int)dm_f2u(hq[14 * HQ + e]);
					item = dm_f2u(hq[15 * HQ + e]);
					if (HAS_MODELS) best_tri = dm_f2u(hq[16 * HQ + e]);
				}
				asm volatile("" ::: "memory");
				hq_head += n_pop;
				hq_head = hq_head >= HQ ? hq_head - HQ : hq_head;
				hq_count -= n_pop;
				shm |= popm;
			}
			// render.cl:415-416: the last bounce only collects the emission. Lanes on their last bounce run the bounce below along
			// with the others and drop what it computes (the wave pays for it either way; not masking them out saves the
			// exec-mask bookkeeping and the copies of mask / direction the compiler keeps around such a branch) -- unless
			// the whole wave is on its last bounce.
			const unsigned long long lastm = ballot64(bounce == nb - 1) & shm;
			const bool show_normals = !FAST && p.rd.show_normals != 0;
			if (SRT_DIAG_ON || DIFFUSE_WAVE) w_shade++;
			bool diffuse_all = false, diffuse_short = false; // (the same in every lane of shm) NO_SPEC classes: every shading lane is plain diffuse / and no lane runs the per-lane bounce
			if (in_mask(shm)) {
				SRT_REGION(SHADE_WINNER);
				// ---- winner: normal, material (render.cl:311-312,337-343,361-362,372-375); org = hit position ----
				int type, material_index;
				f3 wv;
				float ww, winv;
				uint32_t first_wtri;
				if (USE_LDS) {
					const float4 w0 = lds[2 * best], w1 = lds[2 * best + 1];
					type = (int)f2u(w0.x);
					material_index = (int)f2u(w0.y);
					wv = mk(w0.z, w0.w, w1.x);
					ww = w1.y;
					first_wtri = f2u(w1.z);
					winv = w1.w;
				} else {
					const WinnerRec *__restrict__ wr = p.winners + best;
					type = wr->type;
					material_index = wr->material;
					wv = mk(wr->vx, wr->vy, wr->vz);
					ww = wr->w;
					first_wtri = wr->first_wtri;
					winv = wr->inv_w;
				}
				const f3 pos = org;
				f3 nrm = wv; // a plane's normal as stored
				if (type == SRT_SHAPE_SPHERE) {
					nrm = div3_by_rcp(pos - wv, ww, winv);
				} else if (HAS_MODELS && type != SRT_SHAPE_PLANE) {
					SRT_REGION(SHADE_MESH_NORMAL);
					const srt_model *__restrict__ m = &p.shapes[best].shape.model;
					const float *__restrict__ w = USE_BVH ? p.bvh_blocks + (size_t)(best_tri >> 2) * 32u + (best_tri & 3u) * SRT_BVH_TRI_FLOATS
					                                      : wtris + (size_t)(first_wtri + best_tri) * SRT_WTRI_FLOATS;
					const uint32_t tri_in_model = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
					f3 v0 = mk(w[0], w[1], w[2]);
					f3 e1 = mk(w[3], w[4], w[5]);
					f3 e2 = mk(w[6], w[7], w[8]);
					// barycentric_weights (render.cl:223-241), "shifted" (w2, w0, w1)
					f3 v2 = pos - v0;
					float d00 = dot3(e1, e1), d01 = dot3(e1, e2), d11 = dot3(e2, e2);
					float d20 = dot3(v2, e1), d21 = dot3(v2, e2);
					float den = d00 * d11 - d01 * d01;
					float w0 = (d11 * d20 - d01 * d21) / den;
					float w1 = (d00 * d21 - d01 * d20) / den;
					float w2 = 1.0f - w0 - w1;
					const srt_triangle *__restrict__ tr = p.triangles + (m->triangle_index + tri_in_model);
					f3 n = (ld3(tr->vertices[0].normal) * w2 + ld3(tr->vertices[1].normal) * w0) + ld3(tr->vertices[2].normal) * w1;
					n = mat_by_vec(m->transform, n, 0.0f); // forward matrix, as the reference
					nrm = normalize3(n);
#if SRT_TEXTURED
					// per-triangle materials: everything below that reads a material (emission, thresholds, smoothness, ior, colour,
					// texture binding) reads the triangle's. Any valid index is consistent with the scene's flags: see triangle_material.
					material_index = triangle_material(p.tx, m->triangle_index + tri_in_model, material_index);
#endif
				}
				const bool front = dot3(nrm, dir) < 0.0f;
				nrm = nrm * (front ? 1.0f : -1.0f);

				if (show_normals) { // (wave-uniform)
					color = mk(nrm.x * 0.5f + 0.5f, nrm.y * 0.5f + 0.5f, nrm.z * 0.5f + 0.5f); // render.cl:407-410
				} else {
					SRT_REGION(SHADE_MATERIAL);
					float4 m0, m1, mc, me;
					if (USE_LDS) {
						const float4 *__restrict__ lm = lds + (FAST ? 2 * FN + 12 : 2 * n_shapes) + 4 * material_index;
						m0 = lm[0], m1 = lm[1], mc = lm[2], me = lm[3];
					} else {
						const float4 *__restrict__ gm = reinterpret_cast<const float4 *>(p.materials + material_index);
						m0 = gm[0], m1 = gm[1], mc = gm[2], me = gm[3];
					}
					const float smoothness = m0.x, metallic = m0.y, specular = m0.z, emission_strength = m0.w;
					const float transmittance = m1.x, ior = m1.y;
#if SRT_TEXTURED
					const f3 mcolor = texture_albedo<HAS_MODELS, USE_BVH>(p, p.tx, best, best_tri, pos, material_index, mk(mc.x, mc.y, mc.z));
#else
					const f3 mcolor = mk(mc.x, mc.y, mc.z);
#endif
					if constexpr (DIFFUSE_WAVE) diffuse_all = diffuse_short = diffuse_wave_materials(metallic, transmittance); // (a phase that bounces votes on its operands below)
					color = color + (mask * mk(me.x, me.y, me.z)) * emission_strength; // render.cl:413
					if ((shm & ~lastm) != 0ull) { // (wave-uniform) somebody bounces on: see `lastm` above
						SRT_REGION(SHADE_BOUNCE);
						// cosine weighted direction: 6 draws (render.cl:421, 156-163)
						// The once-in-2^32 cases of a bounce (a count of 0 or 2^32, a dot product of +-0 or NaN) are decided by one vote per
						// WAVE in the scene classes' kernels, and the lanes run without the selects and clamps for them. The general kernels
						// keep the per-lane forms: the second copy of each stretch costs them 4 VGPRs, and the sphere / plane ones among them
						// a wave per SIMD.
						f3 rd_ = normalize3(FAST ? random_normal3(seed) : random_normal3_lane(seed));
						const float rd_side = dot3(nrm, rd_);
						f3 hemi = FAST ? mul_sign_wave(rd_, rd_side) : rd_ * sign_fast(rd_side);
						f3 random_dir = normalize3(nrm + hemi);
						// Diffuse waves (device_shading.h "DIFFUSE WAVES"): every shading lane's material is plain diffuse and the operands pass
						// the guard, voted once per phase: the new direction is random_dir as it is. Any other wave: the per-lane form. @rare
						if constexpr (DIFFUSE_WAVE) diffuse_short = diffuse_all && diffuse_wave_operands(random_dir, dir, nrm, smoothness);
						if (DIFFUSE_WAVE && diffuse_short) {
							bounce_diffuse_wave(random_dir, mcolor, dir, mask, seed);
						} else {
						f3 reflected_dir = reflect3(dir, nrm);
						// the three material draws (render.cl:427-430; nothing else draws in between)
						bool is_metallic, is_specular, is_transparent;
						if (no_specular) {
							// (wave-uniform) No material of the scene is specular: `0 > random_float` is false whatever the generator returns, so
							// the draw is not made -- the state steps over it (the compiler folds the two steps to the transmittance draw into
							// one multiply-add) -- and mix(colour, 1, 0) below is the colour (SRT_MF_PLAIN_COLORS). BASELINE configs[0..4].
							is_metallic = bernoulli(metallic, true, seed);
							seed = seed * 747796405u + 2891336453u; // random_bits' state step, its output unused
							is_specular = false;
							is_transparent = bernoulli(transmittance, true, seed);
						} else if (unit_materials) { // (wave-uniform)
							is_metallic = bernoulli(metallic, true, seed), is_specular = bernoulli(specular, true, seed), is_transparent = bernoulli(transmittance, true, seed);
						} else {
							is_metallic = bernoulli(metallic, false, seed), is_specular = bernoulli(specular, false, seed), is_transparent = bernoulli(transmittance, false, seed);
						}
						f3 rough_dir = mix3(random_dir, reflected_dir, smoothness);
						if (!is_transparent) {
							SRT_REGION(SHADE_OPAQUE);
							dir = mix3(random_dir, rough_dir, (is_metallic || is_specular) ? 1.0f : 0.0f);
							if (no_specular) mask = mask * mcolor; // = mix3(mcolor, 1, 0) for finite colours that are not -0
							else mask = mask * mix3(mcolor, mk(1.0f, 1.0f, 1.0f), is_specular ? 1.0f : 0.0f);
						} else {
							SRT_REGION(SHADE_GLASS);
							f3 in_dir = reflect3(rough_dir, nrm);
							// 1/ior and both Schlick r0 values come precomputed with the material (srt_update_scene)
							float mu = front ? m1.z : ior;
							float r0 = front ? m1.w : mc.w;
							float cos_theta = dm_min(1.0f, dot3(in_dir, neg(nrm)));
							// 1 - x with x >= 0 is 0, or at least 2^-25 in magnitude (x < 0.5: above 0.5; x >= 0.5: a multiple
							// of 2^-24), or inf / NaN: never inside sqrt_ieee's guarded interval (0, 2^-96) -- here and below
							float sin_theta = sqrt_core(1.0f - cos_theta * cos_theta);
							bool reflected = mu * sin_theta > 1.0f;
							if (!reflected) reflected = schlick(r0, cos_theta) > random_float(seed); // short-circuit ||
							if (reflected) {
								dir = rough_dir;
							} else {
								SRT_REGION(SHADE_REFRACT);
								f3 out_perp = (in_dir + nrm * cos_theta) * mu;
								float lsq = (out_perp.x * out_perp.x + out_perp.y * out_perp.y) + out_perp.z * out_perp.z;
								f3 out_parallel = nrm * (-sqrt_core(dm_fabs(1.0f - lsq)));
								dir = out_perp + out_parallel;
								mask = mask * mcolor;
							}
						}
						}
						SRT_REGION(SHADE_TAIL);
						dir = normalize3(dir);
						const float out_side = dot3(nrm, dir);
						org = pos + (FAST ? mul_sign_wave(nrm, out_side) : nrm * sign_fast(out_side)) * 0.001f; // render.cl:462
						bounce++;
					}
				}
			}
			// (the two flags were set under the exec mask shm and are false in the other lanes: a vote makes them the wave's again)
			if constexpr (DIFFUSE_WAVE) w_diffuse_short += any64(diffuse_short) ? 1u : 0u, w_diffuse_failed += any64(diffuse_all && !diffuse_short) ? 1u : 0u;
			// what became of the shaded paths: ended (show_normals, or the last bounce: only its emission counts) or on their way again
			if (show_normals) {
				finm |= shm;
			} else {
				finm |= lastm;
				actm = shm & ~lastm;
			}
			SRT_CLK(2);
		} else if (n_hit != 0u) {
			// PARK: every hit waits in the queue; all lanes are free for new camera rays
			if (in_mask(hitm)) {
				SRT_REGION(PARK);
				uint32_t e = hq_head + hq_count + lane_rank(hitm);
				e = e >= HQ ? e - HQ : e;
				hq[0 * HQ + e] = org.x, hq[1 * HQ + e] = org.y, hq[2 * HQ + e] = org.z;
				hq[3 * HQ + e] = dir.x, hq[4 * HQ + e] = dir.y, hq[5 * HQ + e] = dir.z;
				hq[6 * HQ + e] = mask.x, hq[7 * HQ + e] = mask.y, hq[8 * HQ + e] = mask.z;
				hq[9 * HQ + e] = color.x, hq[10 * HQ + e] = color.y, hq[11 * HQ + e] = color.z;
				hq[12 * HQ + e] = dm_u2f(seed);
				hq[13 * HQ + e] = dm_u2f((uint32_t)best);
				hq[14 * HQ + e] = dm_u2f((uint32_t)bounce);
				hq[15 * HQ + e] = dm_u2f(item);
				if (HAS_MODELS) hq[16 * HQ + e] = dm_u2f(best_tri);
			}
			asm volatile("" ::: "memory");
			hq_count += n_hit;
			SRT_CLK(3);
		}

		// ---- paths that ended in this iteration hand in their radiance ----
		if (finm != 0ull) {
			if (in_mask(finm)) {
				SRT_REGION(HANDIN);
				store_radiance(p.radiance, item, color);
			}
		}

		SRT_CLK(4);
		// ================= REFILL: free lanes take new camera rays =================
		SRT_REGION(REFILL_HEAD);
		uint32_t n_act = popc64(actm); // lanes that hold a ray
		if (SUSPEND) {
			// A scan stack that holds a wave-full is taken back by ALL 64 lanes: the scan then runs without an idle lane. Rays the
			// lanes hold at this point -- bounced or new, about to set out -- are parked and come back into lanes that fall free.
			// At the very end (no camera ray left, nothing else under way) the fuller stack is taken back as it is.
			const bool full0 = sq_count0 >= (uint32_t)SRT_SCAN_FULL, full1 = sq_count1 >= (uint32_t)SRT_SCAN_FULL;
			const bool tail = queue_dry && n_act == 0u && hq_count == 0u && pk_count == 0u;
			auto ld = [&](const float *a) { return dm_u2f(__hip_atomic_load(reinterpret_cast<const uint32_t *>(a), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
			bool took_pool = false;
			if (use_pool && tail && !full0 && !full1 && !pool_leave) {
				SRT_REGION(REFILL_POOL);
				constexpr uint32_t NF = USE_BVH ? 20u : 19u;
				const uint32_t NB = SRT_COLD(p).pool_blocks; // blocks per stack (<= SRT_POOL_BLOCKS, which the layout is made for)
				uint32_t *__restrict__ ctl = reinterpret_cast<uint32_t *>(SRT_COLD(p).scan_queue); // [0,1] records reserved, [2,3] blocks taken, [4] waves gone, [5,6] permits, [16 + stack * NB + block] records published
				float *__restrict__ prec = SRT_COLD(p).scan_queue + SRT_POOL_CTL_WORDS; // [stack][block][field][64]
				if (!pool_last && (sq_count0 | sq_count1) != 0u) {
					// (whoever ends these paths stores their radiance; an item is stored once, so there is nothing of this wave's to order it behind)
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's own stack records have arrived
					for (uint32_t sid = 0; sid < 2u; sid++) {
						const uint32_t k = sid ? sq_count1 : sq_count0;
						if (k == 0u) continue;
						uint32_t base = 0;
						if (lane == 0) base = __hip_atomic_fetch_add(ctl + sid, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
						const uint32_t room = base < NB * 64u ? NB * 64u - base : 0u;
						const uint32_t d = k < room ? k : room; // a full pool: the rays beyond stay with this wave
						const float *__restrict__ src = sq_base + sid * (20u * SQ);
						for (uint32_t r = (uint32_t)lane; r < d; r += 64u) {
							const uint32_t e = k - 1u - r, g = base + r;
							uint32_t *__restrict__ dst = reinterpret_cast<uint32_t *>(prec) + ((size_t)sid * SRT_POOL_BLOCKS + (g >> 6)) * (20u * 64u) + (g & 63u);
							for (uint32_t f = 0; f < NF; f++) __hip_atomic_store(dst + f * 64u, dm_f2u(ld(src + f * SQ + e)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						}
						// records (and the radiances above) have been acknowledged by memory before they are published: lane j adds,
						// for the j-th block the records went into, how many went there (d <= 190: four blocks at most)
						asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
						if (d != 0u) {
							const uint32_t b0 = base >> 6, bj = b0 + (uint32_t)lane;
							const uint32_t lo = bj * 64u > base ? bj * 64u : base, hi = (bj + 1u) * 64u < base + d ? (bj + 1u) * 64u : base + d;
							if ((uint32_t)lane < 4u && hi > lo) (void)__hip_atomic_fetch_add(ctl + 16u + sid * (uint32_t)SRT_POOL_BLOCKS + bj, hi - lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							// a permit for every block this reservation has completed (its last place reserved)
							const uint32_t done = ((base + d) >> 6) - b0;
							if (lane == 0 && done != 0u) (void)__hip_atomic_fetch_add(ctl + 5u + sid, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						}
						if (sid) sq_count1 = k - d;
						else sq_count0 = k - d;
						w_pool_given += d;
					}
				}
				const bool kept = (sq_count0 | sq_count1) != 0u; // (a full pool, or the last wave's own)
				uint32_t got_sid = 2u, got_blk = 0u, got_cnt = 0u;
				if (lane == 0 && !pool_last) {
					// One permit per block whose 64 places have all been reserved (ctl[5 + stack], signed); a wave that gets one
					// draws the number of its block from the head counter. No compare-and-swap loop: with thousands of waves at one
					// counter every success makes all the others fail and try again (measured: 2,100 rounds per attempt).
					for (uint32_t sid = 0; sid < 2u && got_sid == 2u; sid++) {
						if ((int)__hip_atomic_load(ctl + 5u + sid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) continue;
						if ((int)__hip_atomic_fetch_sub(ctl + 5u + sid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) {
							got_sid = sid, got_cnt = 64u;
							got_blk = __hip_atomic_fetch_add(ctl + 2u + sid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						} else {
							(void)__hip_atomic_fetch_add(ctl + 5u + sid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						}
					}
				}
				got_sid = (uint32_t)__builtin_amdgcn_readfirstlane((int)got_sid);
				if (got_sid == 2u && !kept && !pool_last) {
					uint32_t gone = 0;
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (what this wave published has arrived)
					if (lane == 0) gone = __hip_atomic_fetch_add(ctl + 4u, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					gone = (uint32_t)__builtin_amdgcn_readfirstlane((int)gone);
					if (gone == gridDim.x - 1u) pool_last = true; // every other wave has published what it had and is gone
					else pool_leave = true;
				}
				if (got_sid == 2u && !kept && pool_last) {
					if (lane == 0) {
						for (uint32_t sid = 0; sid < 2u && got_sid == 2u; sid++) {
							const uint32_t h = __hip_atomic_load(ctl + 2u + sid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							uint32_t res = __hip_atomic_load(ctl + sid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							res = res < NB * 64u ? res : NB * 64u;
							if (h < NB && res > h * 64u) {
								got_sid = sid, got_blk = h, got_cnt = res - h * 64u < 64u ? res - h * 64u : 64u;
								__hip_atomic_store(ctl + 2u + sid, h + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							}
						}
					}
					got_sid = (uint32_t)__builtin_amdgcn_readfirstlane((int)got_sid);
				}
				if (got_sid != 2u) {
					got_blk = (uint32_t)__builtin_amdgcn_readfirstlane((int)got_blk);
					got_cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)got_cnt);
					// All places of the block are reserved; the waves that reserved the last ones may still be writing (straight-line
					// code between their reservation and its publication: microseconds). Bounded all the same.
					uint32_t spins = 0;
					while (__hip_atomic_load(ctl + 16u + got_sid * (uint32_t)SRT_POOL_BLOCKS + got_blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < got_cnt) {
						__builtin_amdgcn_s_sleep(8);
						if (++spins > (1u << 22)) {
							if (lane == 0) atomicAdd((unsigned long long *)SRT_COLD(p).counters + SRT_CTR_WATCHDOG, 1ull);
							got_cnt = 0u; // (the launch is reported as failed)
							break;
						}
					}
					// The records are read only behind the count that publishes them: nothing lets the compiler move the (relaxed) loads
					// below in front of the loop's, but nothing forbade it either. (The hardware returns a wave's loads in order.)
					asm volatile("" ::: "memory");
					const float *__restrict__ src = prec + ((size_t)got_sid * SRT_POOL_BLOCKS + got_blk) * (20u * 64u) + (uint32_t)lane;
					actm = lanes_below(got_cnt);
					if (in_mask(actm)) {
						org = mk(ld(src + 0 * 64), ld(src + 1 * 64), ld(src + 2 * 64));
						dir = mk(ld(src + 3 * 64), ld(src + 4 * 64), ld(src + 5 * 64));
						mask = mk(ld(src + 6 * 64), ld(src + 7 * 64), ld(src + 8 * 64));
						color = mk(ld(src + 9 * 64), ld(src + 10 * 64), ld(src + 11 * 64));
						seed = dm_f2u(ld(src + 12 * 64)), bounce = (int)dm_f2u(ld(src + 13 * 64)), item = dm_f2u(ld(src + 14 * 64));
						tmin = ld(src + 15 * 64), best = (int)dm_f2u(ld(src + 16 * 64)), best_tri = dm_f2u(ld(src + 17 * 64));
						pos = dm_f2u(ld(src + 18 * 64));
					}
					asm volatile("" ::: "memory");
					resm = actm;
					n_act = got_cnt;
					took_pool = true;
					w_pool_taken++;
					if (pool_last) w_pool_last_taken++;
				}
			}
			const bool rest = tail && !took_pool && (sq_count0 | sq_count1) != 0u;
			if (took_pool) {
				// (the wave is full of rays from the pool)
			} else if ((full0 || full1 || rest) && pk_count + n_act <= PK) {
				SRT_REGION(REFILL_SCANQ);
				if (n_act != 0u) {
					const uint32_t e = pk_count + lane_rank(actm);
					if (in_mask(actm)) {
						pk[0 * PK + e] = org.x, pk[1 * PK + e] = org.y, pk[2 * PK + e] = org.z;
						pk[3 * PK + e] = dir.x, pk[4 * PK + e] = dir.y, pk[5 * PK + e] = dir.z;
						pk[6 * PK + e] = mask.x, pk[7 * PK + e] = mask.y, pk[8 * PK + e] = mask.z;
						pk[9 * PK + e] = color.x, pk[10 * PK + e] = color.y, pk[11 * PK + e] = color.z;
						pk[12 * PK + e] = dm_u2f(seed), pk[13 * PK + e] = dm_u2f((uint32_t)bounce), pk[14 * PK + e] = dm_u2f(item);
					}
					pk_count += n_act;
				}
				const uint32_t sid = full0 ? 0u : full1 ? 1u : (sq_count1 > sq_count0 ? 1u : 0u);
				const uint32_t held = sid ? sq_count1 : sq_count0;
				const uint32_t n_pop = held < 64u ? held : 64u;
				const float *__restrict__ sq = sq_base + sid * (20u * SQ);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the records' stores have arrived (acknowledged by the L2)
				actm = lanes_below(n_pop);
				if (in_mask(actm)) {
					const uint32_t e = held - 1u - (uint32_t)lane;
					org = mk(ld(sq + 0 * SQ + e), ld(sq + 1 * SQ + e), ld(sq + 2 * SQ + e));
					dir = mk(ld(sq + 3 * SQ + e), ld(sq + 4 * SQ + e), ld(sq + 5 * SQ + e));
					mask = mk(ld(sq + 6 * SQ + e), ld(sq + 7 * SQ + e), ld(sq + 8 * SQ + e));
					color = mk(ld(sq + 9 * SQ + e), ld(sq + 10 * SQ + e), ld(sq + 11 * SQ + e));
					seed = dm_f2u(ld(sq + 12 * SQ + e)), bounce = (int)dm_f2u(ld(sq + 13 * SQ + e)), item = dm_f2u(ld(sq + 14 * SQ + e));
					tmin = ld(sq + 15 * SQ + e), best = (int)dm_f2u(ld(sq + 16 * SQ + e)), best_tri = dm_f2u(ld(sq + 17 * SQ + e));
					pos = dm_f2u(ld(sq + 18 * SQ + e));
				}
				asm volatile("" ::: "memory");
				resm = actm;
				if (sid) sq_count1 -= n_pop;
				else sq_count0 -= n_pop;
				n_act = n_pop;
			} else if (pk_count != 0u && n_act != 64u) {
				SRT_REGION(REFILL_UNPARK);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				const uint32_t n_pop = 64u - n_act < pk_count ? 64u - n_act : pk_count;
				const unsigned long long fm = ~actm;
				const uint32_t rank = lane_rank(fm);
				const unsigned long long um = ballot64(rank < n_pop) & fm;
				if (in_mask(um)) {
					const uint32_t e = pk_count - 1u - rank;
					org = mk(ld(pk + 0 * PK + e), ld(pk + 1 * PK + e), ld(pk + 2 * PK + e));
					dir = mk(ld(pk + 3 * PK + e), ld(pk + 4 * PK + e), ld(pk + 5 * PK + e));
					mask = mk(ld(pk + 6 * PK + e), ld(pk + 7 * PK + e), ld(pk + 8 * PK + e));
					color = mk(ld(pk + 9 * PK + e), ld(pk + 10 * PK + e), ld(pk + 11 * PK + e));
					seed = dm_f2u(ld(pk + 12 * PK + e)), bounce = (int)dm_f2u(ld(pk + 13 * PK + e)), item = dm_f2u(ld(pk + 14 * PK + e));
				}
				asm volatile("" ::: "memory");
				pk_count -= n_pop;
				actm |= um;
				n_act += n_pop;
			}
		}
		const uint32_t n_free = 64u - n_act;
		if (FAST) cam_phase = false;
		if (!queue_dry && n_free >= (uint32_t)SRT_REFILL_MIN && (!SUSPEND || pk_count == 0u)) {
			const unsigned long long freem = ~actm;
			const uint32_t rank = lane_rank(freem);
			uint32_t given = 0; // free lanes served so far (wave-uniform)
			uint32_t off = 0, qpix = 0;
			while (given < n_free) {
				SRT_REGION(REFILL_LOOP);
				if (sj_next == sj_end) {
					SRT_REGION(REFILL_OPEN);
					// the current sub-job is handed out (or there is none yet): open the next one of the wave's chunk
					if (chunk_cur == chunk_end) {
						SRT_REGION(REFILL_CURSOR);
						unsigned long long start = total_items;
						if (own_chunks_end < (unsigned long long)total_items) { // else every chunk is some wave's first: nothing to ask the cursor for
							if (lane == 0) start = atomicAdd((unsigned long long *)SRT_COLD(p).queue, (unsigned long long)SRT_COLD(p).job_items);
							// lane 0's value as a scalar (wave-uniform control flow: lane 0 is active), so that everything derived from
							// it -- chunk bounds, sub-job bases -- stays in SGPRs
							const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)start);
							const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(start >> 32));
							start = (((unsigned long long)hi << 32) | lo) + own_chunks_end;
						}
						if (start >= (unsigned long long)total_items) {
							queue_dry = true;
							shade_thr = 0u;
							break;
						}
						chunk_cur = (uint32_t)start;
						const uint32_t job_items = SRT_COLD(p).job_items;
						chunk_end = (total_items - chunk_cur < job_items) ? total_items : chunk_cur + job_items;
					}
					const uint32_t left = chunk_end - chunk_cur;
					const uint32_t n = left < SUB ? left : SUB;
					const uint32_t q0 = chunk_cur / nbs; // one division per sub-job
					sj_next = chunk_cur, sj_end = chunk_cur + n, sj_qpix = q0, sj_off = chunk_cur - q0 * nbs;
					chunk_cur += n;
					continue;
				}
				SRT_REGION(REFILL_TAKE);
				const uint32_t avail = sj_end - sj_next;
				const uint32_t take = avail < n_free - given ? avail : n_free - given;
				const uint32_t r = rank - given; // (rank < given: a huge number)
				const unsigned long long takem = ballot64(r < take) & freem; // the free lanes number given .. given + take - 1
				if (in_mask(takem)) {
					item = sj_next + r;
					off = sj_off + r; // < nbs + SUB
					qpix = sj_qpix;
				}
				sj_next += take, sj_off += take;
				given += take;
				w_paths += take;
			}
			const unsigned long long gotm = ballot64(rank < given) & freem; // every lane served holds a camera ray from here on
			actm |= gotm;
			if (FAST) cam_phase = n_act == 0u; // gotm covers actm: no lane holds an older ray
			if (in_mask(gotm)) {
				SRT_REGION(CAMERA);
				// ---- camera ray (render.cl:488,496-516) ----
				// No per-lane integer division and no IEEE division sequence here: pixel, row and sample come from multiplications
				// by host-made magic numbers (srt_magic_u31), the two quotients by the image size from div_by_rcp.
				const auto &c = SRT_COLD(p);
				// off < nbs + SUB: one pixel further at most when a pixel has at least SUB samples in this batch, else off / nbs by a
				// 16-bit reciprocal (exact below 256 for divisors below 128: the error off * (magic * nbs - 2^16) stays under 2^15)
				static_assert(SUB <= 128u, "off / nbs by the 16-bit reciprocal is exact for off < 256 and nbs < 128 only (tests/csrc/magic_check.cpp)");
				const uint32_t dq = (nbs >= SUB) ? (off >= nbs ? 1u : 0u) : (off * c.nbs_magic16) >> 16;
				const uint32_t q = qpix + dq; // owned pixels < 2^31 (checked by the host)
				const uint32_t sample = c.first_sample + (off - dq * nbs);
				const uint32_t lrow = (__umulhi(q, c.width_magic) + q) >> c.width_shift;
				const int px = (int)(q - lrow * (uint32_t)width);
				int py = (int)lrow;
				if (c.world != 1) { // (wave-uniform) global y of packed local row (include/srt_abi.h srt_set_partition)
					const uint32_t lb = (__umulhi(lrow, c.rpb_magic) + lrow) >> c.rpb_shift;
					py = (int)((lb * (uint32_t)c.world + (uint32_t)c.rank) * (uint32_t)c.rows_per_block + (lrow - lb * (uint32_t)c.rows_per_block));
				}
				const uint32_t id = (uint32_t)px + (uint32_t)py * (uint32_t)width;
				seed = (sample + id * (uint32_t)ns) * c.rd.time * 5304u;
				float ndc_x = div_by_rcp((float)px + random_float(seed), c.f_width, c.inv_f_width);
				float ndc_y = div_by_rcp((float)py + random_float(seed), c.f_height, c.inv_f_height);
				float sx = ((2.f * ndc_x - 1.f) * c.rd.aspect_ratio) * c.rd.fov_scale;
				float sy = (1.f - 2.f * ndc_y) * c.rd.fov_scale;
				const f3 c0 = mk(c.rd.camera_to_world[0].x, c.rd.camera_to_world[0].y, c.rd.camera_to_world[0].z);
				const f3 c1 = mk(c.rd.camera_to_world[1].x, c.rd.camera_to_world[1].y, c.rd.camera_to_world[1].z);
				const f3 c2 = mk(c.rd.camera_to_world[2].x, c.rd.camera_to_world[2].y, c.rd.camera_to_world[2].z);
				org = mk(c.rd.camera_to_world[3].x, c.rd.camera_to_world[3].y, c.rd.camera_to_world[3].z);
				dir = normalize3(mat_cols_by_vec(c0, c1, c2, org, mk(sx, sy, -1.0f), 0.0f)); // (the position column times w = 0 stays: inf * 0 is a NaN the reference has, too)
				mask = mk(1.f, 1.f, 1.f);
				color = mk(0.f, 0.f, 0.f);
				bounce = 0;
			}
		}

		SRT_CLK(5);
		SRT_REGION(LOOP_TAIL);
		if (queue_dry) { // (wave-uniform; while the cursor has work a wave always holds some)
			if (actm == 0ull && hq_count == 0u && (sq_count0 | sq_count1 | pk_count) == 0u) {
				if (!use_pool || pool_leave || pool_last) break; // (with a pool: not before the wave has signed off, REFILL above)
				// Bounded: a wave that spins here without ever getting work leaves with the watchdog counter set instead of hanging.
				if (++idle_spins > (1u << 20)) {
					if (lane == 0) atomicAdd((unsigned long long *)SRT_COLD(p).counters + SRT_CTR_WATCHDOG, 1ull);
					break;
				}
			} else {
				idle_spins = 0;
			}
		}
	}
	// queue dry, no lane holds a ray, nothing parked: the escapes still in the ring are what is left
	SRT_REGION(EPILOGUE);
	if (ring_count != 0u) resolve_ring(p, ring, ring_count, lane SRT_RC_ARG);

	// per-wave counters: this wave's own 64-byte line, no atomics (device_types.h)
	unsigned long long t3 = COUNT_TRIS ? n_tri : w_scans, t4 = COUNT_TRIS ? n_tri_u : w_scan_lanes;
	if (COUNT_TRIS || SUSPEND) {
		for (int off = 32; off > 0; off >>= 1) {
			t3 += __shfl_down(t3, off);
			t4 += __shfl_down(t4, off);
		}
	}
	if (lane == 0) {
		unsigned long long *__restrict__ w = (unsigned long long *)SRT_COLD(p).wave_counters + (size_t)blockIdx.x * SRT_WAVE_CTR_STRIDE;
		w[0] += w_rays;
		w[1] += w_sky;
		w[2] += w_paths;
		if (COUNT_TRIS) {
			w[3] += t3;
			w[4] += t4;
		} else if (SUSPEND) { // diagnostics in the slots the instrumented variant uses for triangle counts
			w[8] += t3;
			w[9] += t4;
#ifndef SRT_PHASE_CLOCK
			w[10] += w_pool_taken, w[11] += w_pool_given, w[12] += (unsigned long long)w_pool_taken * w_pool_taken, w[13] += w_pool_last_taken;
#endif
		}
		if (FAST) w[5] += w_cam;
		if constexpr (AXES != 0u) w[8] += w_axis_phases, w[9] += w_axis_failed; // (the phase clocks' slots: no class kernel is built with them)
		if constexpr (DIFFUSE_WAVE) w[10] += w_diffuse_short, w[11] += w_diffuse_failed; // (likewise)
		w[6] += w_iter;
		w[7] += w_shade;
#ifdef SRT_PHASE_CLOCK
		for (int i = 0; i < 7; i++) w[8 + i] += clk_t[i];
		w[15] += __builtin_amdgcn_s_memtime() - clk_start;
#endif
	}
#ifdef SRT_REGION_COUNT
	__syncthreads();
	{
		unsigned long long *__restrict__ w = (unsigned long long *)SRT_COLD(p).wave_counters + (size_t)blockIdx.x * SRT_WAVE_CTR_STRIDE + 16;
		for (int i = lane; i < 2 * SRT_REGION_MAX; i += 64) w[i] += region_ctr[i];
	}
#endif
