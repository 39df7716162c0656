// closest_hit.inc -- the closest hit of one ray in the scene: srt_trace_kernel's EXTEND (test_block over p.runs) without the
// scan queue. Included as text where a kernel walks -- features_body.inc (the feature kernels), ray_query.hip (the cast) and
// selection.hip (the ID pass) -- so that the three are the same statements and a change to how a model block is tested is
// made once. Text, not a __device__ function: the function form grew all three cast kernels (DESIGN.md 28), an include
// leaves every instruction where it was (scripts/kernel_isa_digest.py).
// In scope: p (TraceParams), org, dir (f3), inv (f3: 1 / dir when HAS_MODELS), tmin (float: the limit to start from, the
// hit's distance afterwards), best (int, -1: nothing yet), best_tri (uint32_t), bvh_stack (BvhStackEntry[]), n_tri, n_tri_u
// (uint32_t counters), HAS_MODELS, USE_BVH; region_ctr under SRT_REGION_COUNT.
// Not included by two walks that differ in substance: srt_occlusion_kernel's block test (occlusion.hip: test_model against
// the constant limit, a ballot after each run) and trace_body.inc's (the queue arguments of walk_bvh and test_triangles).
		auto test_block = [&](const Blk16 &b, uint32_t code, int base) {
			const uint32_t type1 = code & 3u;
			if (type1 == SRT_SHAPE_SPHERE + 1u) {
				if (((code >> 2) & 7u) <= 2u) test_spheres<2>(b, org, dir, base, tmin, best);
				else test_spheres<4>(b, org, dir, base, tmin, best);
			} else if (type1 == SRT_SHAPE_PLANE + 1u) {
				test_planes2(b, (code >> 2) & 7u, org, dir, base, tmin, best);
			} else if (HAS_MODELS && type1 == SRT_SHAPE_MODEL + 1u) {
				if (test_aabb(b.v[0], b.v[1], b.v[2], b.v[4], b.v[5], b.v[6], org, inv, tmin)) {
					if (USE_BVH) walk_bvh<false>(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, f2u(b.v[3]), org, dir, base, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
					else test_triangles<false>(p.wtris, f2u(b.v[3]), f2u(b.v[7]), org, dir, base, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
				}
				if (((code >> 2) & 7u) > 1u && test_aabb(b.v[8], b.v[9], b.v[10], b.v[12], b.v[13], b.v[14], org, inv, tmin)) {
					if (USE_BVH) walk_bvh<false>(reinterpret_cast<const float4 *>(p.bvh_blocks), bvh_stack, f2u(b.v[11]), org, dir, base + 1, tmin, best, best_tri, n_tri, n_tri_u SRT_RC_ARG);
					else test_triangles<false>(p.wtris, f2u(b.v[11]), f2u(b.v[15]), org, dir, base + 1, tmin, best, best_tri, n_tri_u SRT_RC_ARG);
				}
			}
		};
		for (int g = 0; g < p.num_runs; g++) {
			float gh[4];
			ld_uniform<4, 16>(reinterpret_cast<const float *>(p.runs + g), gh);
			const uint32_t code = f2u(gh[0]);
			const float *__restrict__ gd = p.run_data + 48 * g;
			test_block(ld_blk16(gd), code & 255u, (int)f2u(gh[1]));
			if ((code >> 8) & 255u) test_block(ld_blk16(gd + 16), (code >> 8) & 255u, (int)f2u(gh[2]));
			if ((code >> 16) & 255u) test_block(ld_blk16(gd + 32), (code >> 16) & 255u, (int)f2u(gh[3]));
		}
