// features_body.inc -- the body of srt_features_kernel and srt_features_ids_kernel (kernels.hip includes it once for each, so
// that the two are the same statements in the same place: a shared __device__ function schedules the first differently).
// In scope: fp (FeatureParams), HAS_MODELS, USE_BVH; SRT_FEATURES_IDS 0 / 1; with 1 also shape_ids (uint32_t *): the shape
// index of feature sample 0 per pixel, 0xffffffff for a miss or a shape without a material, a plain store. SRT_FEATURES_IDS 2
// (srt_features_tris_kernel) is 1 and tri_ids (uint32_t *): the index inside its model of the triangle that sample hit (what
// winner_normal takes), 0xffffffff also for a sphere or a plane.
	const TraceParams &p = fp.tp;
	const uint32_t q = blockIdx.x * 64u + threadIdx.x;
	if (q >= fp.num_pixels) return;
#ifdef SRT_REGION_COUNT
	__shared__ uint32_t region_ctr[2 * SRT_REGION_MAX]; // (development builds: the shared helpers count regions; nobody reads these)
#endif
	const int width = p.rd.width;
	// q is the lane's pixel in the handle's packed rows (fp.num_pixels = owned pixels). Full frame: that is the pixel id. A
	// member of a device group (world != 1) finds the global y of its packed row as srt_trace_kernel's CAMERA does; seed,
	// jitter and camera ray below come from the global pixel id, the sums go to the packed place q.
	const uint32_t lrow = (__umulhi(q, p.width_magic) + q) >> p.width_shift; // q / width
	const int px = (int)(q - lrow * (uint32_t)width);
	int py = (int)lrow;
	uint32_t id = q;
	if (p.world != 1) {
		const uint32_t lb = (__umulhi(lrow, p.rpb_magic) + lrow) >> p.rpb_shift;
		py = (int)((lb * (uint32_t)p.world + (uint32_t)p.rank) * (uint32_t)p.rows_per_block + (lrow - lb * (uint32_t)p.rows_per_block));
		id = (uint32_t)px + (uint32_t)py * (uint32_t)width;
	}
	const uint32_t ns = (uint32_t)p.rd.num_samples;
	const f3 c0 = mk(p.rd.camera_to_world[0].x, p.rd.camera_to_world[0].y, p.rd.camera_to_world[0].z);
	const f3 c1 = mk(p.rd.camera_to_world[1].x, p.rd.camera_to_world[1].y, p.rd.camera_to_world[1].z);
	const f3 c2 = mk(p.rd.camera_to_world[2].x, p.rd.camera_to_world[2].y, p.rd.camera_to_world[2].z);
	const f3 cam = mk(p.rd.camera_to_world[3].x, p.rd.camera_to_world[3].y, p.rd.camera_to_world[3].z);
	BvhStackEntry bvh_stack[USE_BVH ? SRT_BVH_STACK_CAP + 1 : 1];
	uint32_t n_tri = 0, n_tri_u = 0;
	f3 nsum = mk(0.f, 0.f, 0.f), asum = mk(0.f, 0.f, 0.f);
	float tsum = 0.f, hits = 0.f;
#if SRT_FEATURES_IDS
	uint32_t id0 = 0xffffffffu;
#endif
#if SRT_FEATURES_IDS == 2
	uint32_t tri0 = 0xffffffffu;
#endif
	for (uint32_t sample = 0; sample < fp.feature_samples; sample++) {
		// ---- camera ray: srt_trace_kernel CAMERA ----
		uint32_t seed = (sample + id * ns) * p.rd.time * 5304u;
		const float ndc_x = div_by_rcp((float)px + random_float(seed), p.f_width, p.inv_f_width);
		const float ndc_y = div_by_rcp((float)py + random_float(seed), p.f_height, p.inv_f_height);
		const float sx = ((2.f * ndc_x - 1.f) * p.rd.aspect_ratio) * p.rd.fov_scale;
		const float sy = (1.f - 2.f * ndc_y) * p.rd.fov_scale;
		const f3 org = cam;
		const f3 dir = normalize3(mat_cols_by_vec(c0, c1, c2, cam, mk(sx, sy, -1.0f), 0.0f));
		// ---- closest_intersection: srt_trace_kernel EXTEND (test_block), without the scan queue ----
		float tmin = DM_INF_F;
		int best = -1;
		uint32_t best_tri = 0;
		f3 inv = mk(0.f, 0.f, 0.f);
		if (HAS_MODELS) inv = mk(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
#include "closest_hit.inc"
		// a shape without a material counts as a miss (render.cl:404)
		const int material = best >= 0 ? p.winners[best].material : -1;
		if (material >= 0) {
			f3 nrm = winner_normal<HAS_MODELS, USE_BVH>(p, best, best_tri, org + dir * tmin);
			const bool front = dot3(nrm, dir) < 0.0f;
			nrm = nrm * (front ? 1.0f : -1.0f);
			nsum = nsum + nrm;
			tsum = tsum + tmin;
			const srt_float3 &mc = p.materials[material].color;
#if SRT_TEXTURED
			// per-triangle materials: the albedo is that of the material the trace kernel shades the hit with (the shape id stays the shape's)
			const int shaded = hit_material<HAS_MODELS, USE_BVH>(p, fp.tx, best, best_tri, material);
			const srt_float3 &tc = p.materials[shaded].color;
			(void)mc;
			asum = asum + texture_albedo<HAS_MODELS, USE_BVH>(p, fp.tx, best, best_tri, org + dir * tmin, shaded, mk(tc.x, tc.y, tc.z));
#else
			asum = asum + mk(mc.x, mc.y, mc.z);
#endif
			hits = hits + 1.0f;
#if SRT_FEATURES_IDS
			if (sample == 0) id0 = (uint32_t)best;
#endif
#if SRT_FEATURES_IDS == 2
			if (HAS_MODELS && sample == 0 && p.winners[best].type == SRT_SHAPE_MODEL)
				tri0 = USE_BVH ? bvh_tri_in_model(reinterpret_cast<const float4 *>(p.bvh_blocks), best_tri) : best_tri;
#endif
		} else {
			asum = asum + mk(1.f, 1.f, 1.f);
		}
	}
#if SRT_FEATURES_IDS
	shape_ids[q] = id0;
#endif
#if SRT_FEATURES_IDS == 2
	tri_ids[q] = tri0;
#endif
	float4 *nd = reinterpret_cast<float4 *>(fp.normal_depth) + q;
	float4 *ah = reinterpret_cast<float4 *>(fp.albedo_hits) + q;
	float4 a = *nd, b = *ah;
	a.x += nsum.x, a.y += nsum.y, a.z += nsum.z, a.w += tsum;
	b.x += asum.x, b.y += asum.y, b.z += asum.z, b.w += hits;
	*nd = a;
	*ah = b;
