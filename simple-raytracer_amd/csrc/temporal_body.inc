// temporal_body.inc -- the body of srt_temporal_setup_kernel (SRT_TEMPORAL_MOTION 0) and srt_temporal_motion_kernel (1);
// temporal.hip includes it once for each. With 0 the preprocessed text is the set-up kernel as it was before object motion,
// so its instructions are too. In scope: p (TemporalParams); with 1 also mp (MotionParams). SRT_TEMPORAL_MOTION 2
// (srt_temporal_deform_kernel) is 1 and the DEFORMED state, with vp (VertexParams) in scope; what only it has sits between
// `#if SRT_TEMPORAL_MOTION == 2` and its `#endif`, so the moved kernel's preprocessed text is what it was.
// SRT_TEMPORAL_ILLUM 1 (srt_set_denoise_history_illumination; the three *_illum_kernel): a counted tap of the projected 2x2 is
// rescaled from its own first-hit albedo to this pixel's before it is summed, so the history is reprojected as illumination.
// What only they have sits between `#if SRT_TEMPORAL_ILLUM` and its `#else` / `#endif`: with 0 the text is what it was.
// SRT_TEMPORAL_CLAMP 1 (srt_set_denoise_history_clamp; the six *_clamp_kernel, cp (ClampParams) in scope): the history colour is
// clamped into the bounds srt_temporal_bounds_kernel made of the frame, between `#if SRT_TEMPORAL_CLAMP` and its `#else`.
	const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (x >= p.width || y >= p.height) return;
	const uint32_t i = (uint32_t)y * (uint32_t)p.width + (uint32_t)x;
	// ---- the spatial set-up (srt_denoise_setup_kernel's expressions, divisor T) ----
	const float4 c = p.canvas[i], nd = p.normal_depth[i], ah = p.albedo_hits[i];
	const float m = p.moments[i];
	const float4 cc = make_float4(c.x / p.T, c.y / p.T, c.z / p.T, 0.f);
	const float l = lum(cc.x, cc.y, cc.z);
	const float m2c = m / p.T;
	float v = m2c - l * l;
	v = v > 0.f ? v : 0.f;
	v = v / p.P;
	if (!__builtin_isfinite(v)) v = 0.f;
	const float hits = ah.w;
	float nx = 0.f, ny = 0.f, nz = 0.f, z = 0.f;
	if (hits > 0.f) {
		const float len = sqrtf(nd.x * nd.x + nd.y * nd.y + nd.z * nd.z);
		if (len > 0.f) nx = nd.x / len, ny = nd.y / len, nz = nd.z / len;
		z = nd.w / hits;
	}
	const float4 g0 = make_float4(nx, ny, nz, z);
	const float4 g1 = make_float4(ah.x / p.F, ah.y / p.F, ah.z / p.F, hits / p.F);
#if SRT_TEMPORAL_ILLUM
	// the pixel's divisor as srt_denoise_demodulate_kernel forms it (a NaN channel: eps); only a fully covered pixel's colour
	// is albedo x illumination (hits / F is exactly 1 when every feature sample hit)
	const float dpr = fmaxf(g1.x, SRT_DEMOD_EPS), dpg = fmaxf(g1.y, SRT_DEMOD_EPS), dpb = fmaxf(g1.z, SRT_DEMOD_EPS);
	const float lp = lum(dpr, dpg, dpb);
	const bool full_p = g1.w == 1.0f;
#endif

	// ---- reprojection ----
	float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sh = 0.f, s1 = 0.f, s2 = 0.f;
#if SRT_TEMPORAL_MOTION
	// the pixel's shape s and its state: a static shape keeps the arithmetic below, a moved one maps X through A_s and
	// compares the taps' normals with normalise(B_s N_p)
	uint32_t sid = 0xffffffffu;
	const float *mrow = nullptr;
	float bnx = nx, bny = ny, bnz = nz;
	bool live = p.mode != TP_NONE && g1.w > 0.f && finite3(cc), moved = false;
#if SRT_TEMPORAL_MOTION == 2
	bool deformed = false;
	float p0x = 0.f, p0y = 0.f, p0z = 0.f, q0x = 0.f, q0y = 0.f, q0z = 0.f, e1x = 0.f, e1y = 0.f, e1z = 0.f, e2x = 0.f, e2y = 0.f, e2z = 0.f;
	float f1x = 0.f, f1y = 0.f, f1z = 0.f, f2x = 0.f, f2y = 0.f, f2z = 0.f, a11 = 0.f, a12 = 0.f, a22 = 0.f, det = 1.f;
#endif
	if (live) {
		sid = mp.ids[i];
		live = sid < mp.n_shapes;
		if (live) {
			const uint32_t *row = mp.table + (size_t)sid * SRT_MOTION_WORDS;
			const uint32_t state = row[0];
			mrow = reinterpret_cast<const float *>(row + 1);
			live = state != SRT_MOTION_NO_HISTORY;
			moved = state == SRT_MOTION_MOVED;
			if (moved) {
				const float *b = mrow + 12;
				const float tx = (b[0] * nx + b[1] * ny) + b[2] * nz, ty = (b[3] * nx + b[4] * ny) + b[5] * nz, tz = (b[6] * nx + b[7] * ny) + b[8] * nz;
				const float len = sqrtf((tx * tx + ty * ty) + tz * tz);
				live = len > 0.f && __builtin_isfinite(len);
				bnx = tx / len, bny = ty / len, bnz = tz / len;
			}
#if SRT_TEMPORAL_MOTION == 2
			// a deformed model: the pixel's triangle as it stands now (P) and as it stood in the history frame (Q). It projects
			// and takes only its own shape's taps, as a moved shape does; N_h = normalise((nu f1 + nv f2) + c gh)
			deformed = state == SRT_MOTION_DEFORMED;
			if (deformed) {
				moved = true;
				const uint32_t tri = vp.tris[i];
				live = tri < vp.first[sid + 1] - vp.first[sid]; // (0xffffffff: no triangle)
				if (live) {
					const float *P = vp.rows + (size_t)(row[1] + tri) * 9, *Q = vp.h_rows + (size_t)(row[1] + tri) * 9;
					p0x = P[0], p0y = P[1], p0z = P[2];
					q0x = Q[0], q0y = Q[1], q0z = Q[2];
					e1x = P[3] - p0x, e1y = P[4] - p0y, e1z = P[5] - p0z;
					e2x = P[6] - p0x, e2y = P[7] - p0y, e2z = P[8] - p0z;
					f1x = Q[3] - q0x, f1y = Q[4] - q0y, f1z = Q[5] - q0z;
					f2x = Q[6] - q0x, f2y = Q[7] - q0y, f2z = Q[8] - q0z;
					a11 = (e1x * e1x + e1y * e1y) + e1z * e1z;
					a12 = (e1x * e2x + e1y * e2y) + e1z * e2z;
					a22 = (e2x * e2x + e2y * e2y) + e2z * e2z;
					det = a11 * a22 - a12 * a12;
					const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
					const float hx = f1y * f2z - f1z * f2y, hy = f1z * f2x - f1x * f2z, hz = f1x * f2y - f1y * f2x;
					const float lc = sqrtf((cx * cx + cy * cy) + cz * cz), lh = sqrtf((hx * hx + hy * hy) + hz * hz);
					live = det > 0.f && __builtin_isfinite(det) && lc > 0.f && __builtin_isfinite(lc) && lh > 0.f && __builtin_isfinite(lh);
					const float ne1 = (nx * e1x + ny * e1y) + nz * e1z, ne2 = (nx * e2x + ny * e2y) + nz * e2z;
					const float nu = (a22 * ne1 - a12 * ne2) / det, nv = (a11 * ne2 - a12 * ne1) / det;
					const float cn = (nx * (cx / lc) + ny * (cy / lc)) + nz * (cz / lc);
					const float tx = (nu * f1x + nv * f2x) + cn * (hx / lh), ty = (nu * f1y + nv * f2y) + cn * (hy / lh), tz = (nu * f1z + nv * f2z) + cn * (hz / lh);
					const float len = sqrtf((tx * tx + ty * ty) + tz * tz);
					live = live && len > 0.f && __builtin_isfinite(len);
					bnx = tx / len, bny = ty / len, bnz = tz / len;
				}
			}
#endif
		}
	}
	const bool identity = p.mode == TP_IDENTITY && !moved;
	if (live) {
#else
	if (p.mode != TP_NONE && g1.w > 0.f && finite3(cc)) {
#endif
		float D = z;
		int x0 = x, y0 = y;
		float ax = 0.f, ay = 0.f;
		bool any = true;
#if SRT_TEMPORAL_MOTION
		if (p.mode == TP_PROJECT || moved) {
#else
		if (p.mode == TP_PROJECT) {
#endif
			// the camera ray through the pixel's centre (trace_body.inc CAMERA with 0.5 for the jitter; its division through the
			// host's reciprocal is the IEEE quotient)
			const float ndc_x = ((float)x + 0.5f) / p.f_width, ndc_y = ((float)y + 0.5f) / p.f_height;
			const float sx = ((2.f * ndc_x - 1.f) * p.aspect) * p.fov;
			const float sy = (1.f - 2.f * ndc_y) * p.fov;
			const float rx = ((p.c0[0] * sx + p.c1[0] * sy) + p.c2[0] * -1.0f) + p.cam[0] * 0.0f;
			const float ry = ((p.c0[1] * sx + p.c1[1] * sy) + p.c2[1] * -1.0f) + p.cam[1] * 0.0f;
			const float rz = ((p.c0[2] * sx + p.c1[2] * sy) + p.c2[2] * -1.0f) + p.cam[2] * 0.0f;
			const float rs = dm_rsqrtf(rx * rx + ry * ry + rz * rz);
			const float dx = rx * rs, dy = ry * rs, dz = rz * rs;
#if SRT_TEMPORAL_MOTION
			float wx = p.cam[0] + z * dx, wy = p.cam[1] + z * dy, wz = p.cam[2] + z * dz;
#if SRT_TEMPORAL_MOTION == 2
			bool xh_ok = true;
			if (deformed) { // the same barycentric place on the history's triangle (the affine map of the triangle's plane)
				const float ddx = wx - p0x, ddy = wy - p0y, ddz = wz - p0z;
				const float de1 = (ddx * e1x + ddy * e1y) + ddz * e1z, de2 = (ddx * e2x + ddy * e2y) + ddz * e2z;
				const float u = (a22 * de1 - a12 * de2) / det, v2 = (a11 * de2 - a12 * de1) / det;
				wx = (q0x + u * f1x) + v2 * f2x, wy = (q0y + u * f1y) + v2 * f2y, wz = (q0z + u * f1z) + v2 * f2z;
				xh_ok = __builtin_isfinite(wx) && __builtin_isfinite(wy) && __builtin_isfinite(wz);
			} else
#endif
			if (moved) {
				const float hx = ((mrow[0] * wx + mrow[1] * wy) + mrow[2] * wz) + mrow[3];
				const float hy = ((mrow[4] * wx + mrow[5] * wy) + mrow[6] * wz) + mrow[7];
				const float hz = ((mrow[8] * wx + mrow[9] * wy) + mrow[10] * wz) + mrow[11];
				wx = hx, wy = hy, wz = hz;
			}
			const float ex = wx - p.cam_h[0], ey = wy - p.cam_h[1], ez = wz - p.cam_h[2];
#else
			const float ex = (p.cam[0] + z * dx) - p.cam_h[0], ey = (p.cam[1] + z * dy) - p.cam_h[1], ez = (p.cam[2] + z * dz) - p.cam_h[2];
#endif
			D = sqrtf(ex * ex + ey * ey + ez * ez);
			const float vx = (p.rinv[0] * ex + p.rinv[1] * ey) + p.rinv[2] * ez;
			const float vy = (p.rinv[3] * ex + p.rinv[4] * ey) + p.rinv[5] * ez;
			const float vz = (p.rinv[6] * ex + p.rinv[7] * ey) + p.rinv[8] * ez;
			const float qx = vx / -vz, qy = vy / -vz;
			const float fx = ((qx / (p.aspect_h * p.fov_h) + 1.f) / 2.f) * p.f_width - 0.5f;
			const float fy = ((1.f - qy / p.fov_h) / 2.f) * p.f_height - 0.5f;
			// in front of the history camera, and a 2x2 that touches the image (this also keeps the conversions in range)
			any = vz < 0.f && fx > -1.f && fx < p.f_width && fy > -1.f && fy < p.f_height;
#if SRT_TEMPORAL_MOTION == 2
			any = any && xh_ok;
#endif
			if (any) {
				const float flx = floorf(fx), fly = floorf(fy);
				x0 = (int)flx, y0 = (int)fly;
				ax = fx - flx, ay = fy - fly;
			}
		}
		if (any) {
			for (int k = 0; k < 4; k++) {
				const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
				const float w = (k & 1 ? ax : 1.f - ax) * (k >> 1 ? ay : 1.f - ay);
#if SRT_TEMPORAL_MOTION
				if (identity && k) break;
#else
				if (p.mode == TP_IDENTITY && k) break;
#endif
				if (qx < 0 || qx >= p.width || qy < 0 || qy >= p.height) continue;
				const uint32_t j = (uint32_t)qy * (uint32_t)p.width + (uint32_t)qx;
				const float4 hg1 = p.h_guide[2 * j + 1];
				const float4 hc = p.h_cc[j];
				if (!(hg1.w > 0.f) || !finite3(hc)) continue;
#if SRT_TEMPORAL_MOTION
				// a moved shape's tap must show that shape; a static one's must not show a shape that has left
				const uint32_t hs = mp.h_ids[j];
				if (moved ? hs != sid : (hs < mp.n_shapes && mp.table[(size_t)hs * SRT_MOTION_WORDS] != SRT_MOTION_STATIC)) continue;
				const float4 hg0 = p.h_guide[2 * j];
				if (!(bnx * hg0.x + bny * hg0.y + bnz * hg0.z >= p.normal_threshold)) continue;
#else
				const float4 hg0 = p.h_guide[2 * j];
				if (!(nx * hg0.x + ny * hg0.y + nz * hg0.z >= p.normal_threshold)) continue;
#endif
				if (!(fabsf(hg0.w - D) <= p.depth_threshold * D)) continue;
				const float2 hm = p.h_m[j];
				sw += w;
#if SRT_TEMPORAL_ILLUM
				// r = D_p / D_h per channel, rl = lum(D_p) / lum(D_h); a partly covered pixel or tap stays in colour (it holds sky
				// light no albedo scaled), and so does the identity tap: the pixel itself
				float rr = 1.f, rg = 1.f, rb = 1.f, rl = 1.f;
#if SRT_TEMPORAL_MOTION
				if (full_p && hg1.w == 1.0f && !identity) {
#else
				if (full_p && hg1.w == 1.0f && p.mode != TP_IDENTITY) {
#endif
					const float dhr = fmaxf(hg1.x, SRT_DEMOD_EPS), dhg = fmaxf(hg1.y, SRT_DEMOD_EPS), dhb = fmaxf(hg1.z, SRT_DEMOD_EPS);
					rr = dpr / dhr, rg = dpg / dhg, rb = dpb / dhb;
					rl = lp / lum(dhr, dhg, dhb);
				}
				sr += w * (hc.x * rr), sg += w * (hc.y * rg), sb += w * (hc.z * rb);
				sh += w * hc.w;
				s1 += w * (hm.x * rl), s2 += w * ((hm.y * rl) * rl);
#else
				sr += w * hc.x, sg += w * hc.y, sb += w * hc.z;
				sh += w * hc.w;
				s1 += w * hm.x, s2 += w * hm.y;
#endif
			}
		}
	}

	// ---- integration ----
	float h = 0.f;
	if (sw >= 0.01f) h = fminf(sh / sw, p.limit);
	float4 o = make_float4(cc.x, cc.y, cc.z, v);
	float m1 = l, m2 = m2c, n = p.P;
	if (h > 0.f) {
		n = p.P + h;
#if SRT_TEMPORAL_CLAMP
		// the history colour x_h is complete here (gathered, and rescaled under SRT_TEMPORAL_ILLUM): each channel into
		// [mu - gamma sigma, mu + gamma sigma] of this pixel's bounds (sum of weights 0: no clamp). By comparisons, so a NaN on
		// either side moves nothing; when no channel moved every value below is what it is without the clamp
		float hr = sr / sw, hgc = sg / sw, hb = sb / sw, h1 = s1 / sw, h2 = s2 / sw;
		const float4 b0 = cp.bounds[i];
		if (b0.w > 0.f) {
			const float4 b1 = cp.bounds[cp.num_pixels + i];
			const float er = cp.gamma * b1.x, eg = cp.gamma * b1.y, eb = cp.gamma * b1.z;
			const float lor = b0.x - er, hir = b0.x + er, log_ = b0.y - eg, hig = b0.y + eg, lob = b0.z - eb, hib = b0.z + eb;
			bool mv = false;
			if (hr < lor) hr = lor, mv = true;
			else if (hr > hir) hr = hir, mv = true;
			if (hgc < log_) hgc = log_, mv = true;
			else if (hgc > hig) hgc = hig, mv = true;
			if (hb < lob) hb = lob, mv = true;
			else if (hb > hib) hb = hib, mv = true;
			if (mv) { // the moments follow the colour and keep their variance
				float hv = h2 - h1 * h1;
				hv = hv > 0.f ? hv : 0.f;
				h1 = lum(hr, hgc, hb);
				h2 = hv + h1 * h1;
			}
		}
#else
		const float hr = sr / sw, hgc = sg / sw, hb = sb / sw, h1 = s1 / sw, h2 = s2 / sw;
#endif
		o.x = (p.P * cc.x + h * hr) / n;
		o.y = (p.P * cc.y + h * hgc) / n;
		o.z = (p.P * cc.z + h * hb) / n;
		m1 = (p.P * l + h * h1) / n;
		m2 = (p.P * m2c + h * h2) / n;
		float V = m2 - m1 * m1;
		V = V > 0.f ? V : 0.f;
		V = V / n;
		o.w = __builtin_isfinite(V) ? V : 0.f;
	}
	p.o_cc[i] = make_float4(o.x, o.y, o.z, fminf(n, p.limit));
	p.o_m[i] = make_float2(m1, m2);
	p.o_guide[2 * i] = g0;
	p.o_guide[2 * i + 1] = g1;
	if (p.out) p.out[i] = o;
	if (p.argb) p.argb[i] = tonemap(o.x, o.y, o.z);
