// bvh_host.cpp -- the host BVH builder (bvh_host.h): SAH build, refit, four-wide fold with its byte quantiser, the per-model cache
// entry, and the two host-only entry points of include/srt_abi.h that hand its results out. Standard library only.
#include "bvh_host.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <future>
#include <system_error>

// World-space vertices as the pre-pass kernel computes them (render.cl:114-120 order); boxes
// are padded by 2^-12 of the model's diagonal: a hit the float Moller-Trumbore test accepts
// lies within rounding error of its triangle, and must still be inside every box above it.
void BvhBuilder::load(const srt_model &m, const srt_triangle *all) {
	const uint32_t n = m.num_triangles;
	tris.resize(n);
	is_finite.assign(n, 1);
	auto xf = [&](const srt_float3 &v, float out[3]) {
		const srt_float4 *t = m.transform;
		out[0] = ((t[0].x * v.x + t[1].x * v.y) + t[2].x * v.z) + t[3].x * 1.0f;
		out[1] = ((t[0].y * v.x + t[1].y * v.y) + t[2].y * v.z) + t[3].y * 1.0f;
		out[2] = ((t[0].z * v.x + t[1].z * v.y) + t[2].z * v.z) + t[3].z * 1.0f;
	};
	float mlo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mhi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (uint32_t j = 0; j < n; j++) {
		const srt_triangle &tr = all[m.triangle_index + j];
		float p[3][3];
		for (int k = 0; k < 3; k++) xf(tr.vertices[k].pos, p[k]);
		Tri &t = tris[j];
		t.j = j;
		bool finite = true;
		for (int a = 0; a < 3; a++) {
			// the kernel's triangle is (p0, p0 + e1, p0 + e2) with e = p_k - p0 rounded: cover both
			const float q1 = p[0][a] + (p[1][a] - p[0][a]), q2 = p[0][a] + (p[2][a] - p[0][a]);
			t.lo[a] = std::min(std::min(std::min(p[0][a], p[1][a]), std::min(p[2][a], q1)), q2);
			t.hi[a] = std::max(std::max(std::max(p[0][a], p[1][a]), std::max(p[2][a], q1)), q2);
			finite = finite && std::isfinite(t.lo[a]) && std::isfinite(t.hi[a]);
		}
		if (!finite) { // hostile input: a box that every ray enters, so the triangle is always tested
			for (int a = 0; a < 3; a++) t.lo[a] = -FLT_MAX, t.hi[a] = FLT_MAX, t.c[a] = 0.0f;
			is_finite[j] = 0;
			continue;
		}
		for (int a = 0; a < 3; a++) {
			t.c[a] = 0.5f * t.lo[a] + 0.5f * t.hi[a];
			mlo[a] = std::min(mlo[a], t.lo[a]);
			mhi[a] = std::max(mhi[a], t.hi[a]);
		}
	}
	for (int a = 0; a < 3; a++) ext_lo[a] = mlo[a], ext_hi[a] = mhi[a];
	double d2 = 0.0;
	for (int a = 0; a < 3; a++)
		if (mhi[a] >= mlo[a]) d2 += ((double)mhi[a] - mlo[a]) * ((double)mhi[a] - mlo[a]);
	const float pad = (float)std::min(std::sqrt(d2) * (1.0 / 4096.0), (double)FLT_MAX);
	for (Tri &t : tris)
		for (int a = 0; a < 3; a++) {
			if (t.lo[a] == -FLT_MAX) continue;
			// widen by pad plus two ulps (the slab arithmetic rounds, too); stays finite
			t.lo[a] = std::max(-FLT_MAX, std::nextafter(std::nextafter(t.lo[a] - pad, -INFINITY), -INFINITY));
			t.hi[a] = std::min(FLT_MAX, std::nextafter(std::nextafter(t.hi[a] + pad, INFINITY), INFINITY));
		}
}

// Subtree over tris[b, e) appended to `out` (indices inside `out`; a node's skip = the index behind its subtree, which
// for the subtree's last nodes is out.size() at return). The two halves of a large range are built by two threads into
// vectors of their own and appended in order -- same nodes in the same order as the one-thread build, the ranges of
// `tris` the threads partition are disjoint -- down to `par` levels: 10^5 triangles 42 -> 13 ms on the GPU box's cores.
BvhBuilder::Stats BvhBuilder::build_into(std::vector<BvhNode> &out, uint32_t b, uint32_t e, uint32_t depth, int par) {
	Stats st;
	const uint32_t self = (uint32_t)out.size();
	out.emplace_back();
	st.max_depth = depth;
	float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	float clo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, chi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
	for (uint32_t i = b; i < e; i++)
		for (int a = 0; a < 3; a++) {
			lo[a] = std::min(lo[a], tris[i].lo[a]), hi[a] = std::max(hi[a], tris[i].hi[a]);
			clo[a] = std::min(clo[a], tris[i].c[a]), chi[a] = std::max(chi[a], tris[i].c[a]);
		}
	for (int a = 0; a < 3; a++) out[self].lo[a] = lo[a], out[self].hi[a] = hi[a];
	const uint32_t n = e - b;
	if (n <= SRT_BVH_LEAF_MAX) {
		out[self].leaf = (n << 28) | (rec_base + b);
		out[self].skip = (uint32_t)out.size();
		st.leaves = 1;
		return st;
	}
	// binned SAH over the three axes
	constexpr int NB = 16;
	int best_axis = -1, best_bin = 0;
	float best_cost = INFINITY;
	if (depth < sah_depth) {
		for (int a = 0; a < 3; a++) {
			const float ext = chi[a] - clo[a];
			if (!(ext > 0.0f) || !std::isfinite(ext)) continue;
			const float scale = (float)NB / ext;
			uint32_t cnt[NB] = {0};
			float blo[NB][3], bhi[NB][3];
			for (int k = 0; k < NB; k++)
				for (int c = 0; c < 3; c++) blo[k][c] = FLT_MAX, bhi[k][c] = -FLT_MAX;
			for (uint32_t i = b; i < e; i++) {
				int k = (int)((tris[i].c[a] - clo[a]) * scale);
				k = k < 0 ? 0 : (k >= NB ? NB - 1 : k);
				cnt[k]++;
				for (int c = 0; c < 3; c++) blo[k][c] = std::min(blo[k][c], tris[i].lo[c]), bhi[k][c] = std::max(bhi[k][c], tris[i].hi[c]);
			}
			float rarea[NB];
			uint32_t rcnt[NB];
			float rl[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, rh[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
			uint32_t rc = 0;
			for (int k = NB - 1; k > 0; k--) {
				for (int c = 0; c < 3; c++) rl[c] = std::min(rl[c], blo[k][c]), rh[c] = std::max(rh[c], bhi[k][c]);
				rc += cnt[k];
				rarea[k] = rc ? half_area(rl, rh) : 0.0f;
				rcnt[k] = rc;
			}
			float ll[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, lh[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
			uint32_t lc = 0;
			for (int k = 0; k < NB - 1; k++) { // split after bin k
				for (int c = 0; c < 3; c++) ll[c] = std::min(ll[c], blo[k][c]), lh[c] = std::max(lh[c], bhi[k][c]);
				lc += cnt[k];
				if (lc == 0 || rcnt[k + 1] == 0) continue;
				const float cost = half_area(ll, lh) * (float)lc + rarea[k + 1] * (float)rcnt[k + 1];
				if (cost < best_cost) best_cost = cost, best_axis = a, best_bin = k;
			}
		}
	}
	uint32_t mid;
	if (best_axis >= 0) {
		const int a = best_axis;
		const float scale = (float)NB / (chi[a] - clo[a]);
		const float c0 = clo[a];
		auto it = std::partition(tris.begin() + b, tris.begin() + e, [&](const Tri &t) {
			int k = (int)((t.c[a] - c0) * scale);
			k = k < 0 ? 0 : (k >= NB ? NB - 1 : k);
			return k <= best_bin;
		});
		mid = (uint32_t)(it - tris.begin());
	} else {
		mid = b; // no usable split (coincident centroids, overflow, depth cap): halve by index
	}
	if (mid == b || mid == e) {
		int a = 0;
		for (int c = 1; c < 3; c++)
			if (chi[c] - clo[c] > chi[a] - clo[a]) a = c;
		mid = b + n / 2;
		std::nth_element(tris.begin() + b, tris.begin() + mid, tris.begin() + e, [a](const Tri &x, const Tri &y) { return x.c[a] < y.c[a]; });
	}
	out[self].leaf = 0;
	Stats sl, sr;
	if (par > 0 && n >= 8192) {
		std::vector<BvhNode> left, right;
		std::future<Stats> fut;
		try {
			fut = std::async(std::launch::async, [&] { return build_into(left, b, mid, depth + 1, par - 1); });
		} catch (const std::system_error &) { // no thread to be had: this one does both halves
		}
		sr = build_into(right, mid, e, depth + 1, par - 1);
		sl = fut.valid() ? fut.get() /* (rethrows what the other thread threw) */ : build_into(left, b, mid, depth + 1, 0);
		for (std::vector<BvhNode> *sub : {&left, &right}) {
			const uint32_t off = (uint32_t)out.size();
			out.insert(out.end(), sub->begin(), sub->end());
			for (size_t i = off; i < out.size(); i++) out[i].skip += off;
		}
	} else {
		sl = build_into(out, b, mid, depth + 1, 0);
		sr = build_into(out, mid, e, depth + 1, 0);
	}
	out[self].skip = (uint32_t)out.size();
	st.leaves = sl.leaves + sr.leaves;
	st.max_depth = std::max(sl.max_depth, sr.max_depth);
	return st;
}
uint32_t BvhBuilder::build(uint32_t b, uint32_t e, uint32_t depth) {
	const uint32_t self = (uint32_t)nodes.size();
	const Stats st = build_into(nodes, b, e, depth, par);
	leaves += st.leaves;
	if (st.max_depth > max_depth) max_depth = st.max_depth;
	return self;
}

// New boxes for an existing topology (nodes relative to the model, `order` = triangle of each
// record): the model moved but its triangles did not. Children follow their parent in the
// array, so one backward sweep has every child's box ready before its parent's. O(n).
void BvhBuilder::refit(const srt_model &m, const srt_triangle *all) {
	load(m, all);
	const uint32_t n = (uint32_t)nodes.size();
	for (uint32_t i = n; i-- > 0;) {
		BvhNode &nd = nodes[i];
		float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
		if (nd.leaf) {
			const uint32_t first = nd.leaf & 0x0fffffffu, cnt = nd.leaf >> 28;
			for (uint32_t r = first; r < first + cnt; r++) {
				const Tri &t = tris[order[r]]; // load() leaves tris in triangle order
				for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], t.lo[a]), hi[a] = std::max(hi[a], t.hi[a]);
			}
		} else {
			const uint32_t left = i + 1, right = nodes[left].skip == SRT_BVH_END ? n : nodes[left].skip;
			for (uint32_t c : {left, right})
				for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], nodes[c].lo[a]), hi[a] = std::max(hi[a], nodes[c].hi[a]);
		}
		for (int a = 0; a < 3; a++) nd.lo[a] = lo[a], nd.hi[a] = hi[a];
	}
}

// The boxes of an inner block as bytes (device_types.h): bound = fmaf(q, 2^e, origin) per axis, rounded outwards and CHECKED in
// exactly that arithmetic, the grid coarsened until every upper bound fits a byte. Non-finite extents (hostile input in
// all-embracing boxes) end on the coarsest grid, where upper bounds overflow to +inf: still a box that contains the child.
template <class Fma>
static inline __attribute__((always_inline)) void quantise_body(const std::vector<BvhNode> &c, const uint32_t *kids, uint32_t nk, uint32_t tags, uint32_t first, uint32_t *blk, Fma fmaf_any) {
	float origin[3];
	uint32_t expo[3];
	uint8_t qlo[3][4], qhi[3][4];
	auto pow2 = [](int e) { // 2^e as a float, -126 <= e <= 127
		const uint32_t bits = (uint32_t)(e + 127) << 23;
		float f;
		memcpy(&f, &bits, 4);
		return f;
	};
	for (int a = 0; a < 3; a++) {
		origin[a] = FLT_MAX;
		float top = -FLT_MAX;
		for (uint32_t k = 0; k < nk; k++) origin[a] = std::min(origin[a], c[kids[k]].lo[a]), top = std::max(top, c[kids[k]].hi[a]);
		if (!(origin[a] == origin[a])) origin[a] = -FLT_MAX; // (NaN boxes of hostile input)
		int e = -126;
		const float extent = top - origin[a];
		if (extent > 0.0f) {
			int ex = 0;
			(void)std::frexp(extent / 255.0f, &ex); // extent / 255 = m * 2^ex, m in [0.5, 1): 2^ex is the first power of two above it
			e = std::isfinite(extent) ? ex : 126;
		}
		for (;; e++) {
			if (e < -126) e = -126;
			if (e > 127) e = 127;
			const float scale = pow2(e);
			const double inv_scale = std::ldexp(1.0, -e); // (exact; in double so that 2^126 has a reciprocal)
			bool fits = true;
			for (uint32_t k = 0; k < nk && fits; k++) {
				const float lo = c[kids[k]].lo[a], hi = c[kids[k]].hi[a];
				const double fl = ((double)lo - (double)origin[a]) * inv_scale; // >= 0: origin is the smallest lo
				int ql = fl >= 255.0 ? 255 : (fl > 0.0 ? (int)fl : 0);       // (NaN: 0)
				while (ql > 0 && !(fmaf_any((float)ql, scale, origin[a]) <= lo)) ql--;
				const double fh = ((double)hi - (double)origin[a]) * inv_scale;
				int qh = fh > 255.0 ? 256 : (fh > 0.0 ? (int)fh + ((double)(int)fh < fh ? 1 : 0) : 0);
				if (!(fh == fh)) qh = 256;
				while (qh <= 255 && !(fmaf_any((float)qh, scale, origin[a]) >= hi)) qh++;
				if (qh > 255) fits = false;
				qlo[a][k] = (uint8_t)ql, qhi[a][k] = (uint8_t)(qh & 255);
			}
			if (fits || e == 127) { // (e == 127: 255 * 2^127 overflows every finite bound; keep what we have, q = 255 gives +inf)
				if (!fits)
					for (uint32_t k = 0; k < nk; k++) qhi[a][k] = 255;
				expo[a] = (uint32_t)(e + 127);
				break;
			}
		}
	}
	for (int a = 0; a < 3; a++) memcpy(&blk[a], &origin[a], 4);
	blk[3] = expo[0] | (expo[1] << 8) | (expo[2] << 16) | (nk << 24);
	for (int a = 0; a < 3; a++) {
		blk[4 + a] = 0u, blk[7 + a] = 0u;
		for (uint32_t k = 0; k < 4; k++) {
			blk[4 + a] |= (uint32_t)(k < nk ? qlo[a][k] : 255u) << (8 * k); // (an empty slot: lo above hi; the walk counts the slots)
			blk[7 + a] |= (uint32_t)(k < nk ? qhi[a][k] : 0u) << (8 * k);
		}
	}
	blk[10] = tags;
	blk[11] = first;
}
// The check wants fmaf as the device rounds it. glibc's fmaf is a call into a software path on some hosts (85 ns: 45 ms of a
// 10^5-triangle hierarchy's 528,000 checks); a CPU with FMA does it in one instruction, inlined into a copy of the function.
__attribute__((target("fma"))) static void quantise_hw(const std::vector<BvhNode> &c, const uint32_t *kids, uint32_t nk, uint32_t tags, uint32_t first, uint32_t *blk) {
	quantise_body(c, kids, nk, tags, first, blk, [](float a, float b, float x) __attribute__((target("fma"))) { return __builtin_fmaf(a, b, x); });
}
static void quantise(const std::vector<BvhNode> &c, const uint32_t *kids, uint32_t nk, uint32_t tags, uint32_t first, uint32_t *blk) {
	static const bool hw = __builtin_cpu_supports("fma");
	if (hw) quantise_hw(c, kids, nk, tags, first, blk);
	else quantise_body(c, kids, nk, tags, first, blk, [](float a, float b, float x) { return std::fmaf(a, b, x); });
}
// fills block `self` (already allocated) from node ci; returns the reference to it
uint32_t BvhBuilder::fold_node(const std::vector<BvhNode> &c, uint32_t ci, uint32_t self, bool balanced, Wide &w, uint32_t &need) {
	const BvhNode &nd = c[ci];
	if (nd.leaf) {
		const uint32_t first = nd.leaf & 0x0fffffffu, cnt = nd.leaf >> 28;
		for (uint32_t k = 0; k < cnt; k++) w.dest[first + k] = (self << 2) | k;
		need = 0;
		return SRT_BVH_LEAF_BIT | (cnt << 28) | self;
	}
	w.inner.push_back(self);
	uint32_t kids[4], nk = 0;
	const uint32_t left = ci + 1u, right = c[left].skip;
	kids[nk++] = left, kids[nk++] = right;
	if (balanced) {
		uint32_t g[4], ng = 0;
		for (uint32_t k = 0; k < 2; k++)
			if (c[kids[k]].leaf) g[ng++] = kids[k];
			else g[ng++] = kids[k] + 1u, g[ng++] = c[kids[k] + 1u].skip;
		nk = ng;
		for (uint32_t k = 0; k < ng; k++) kids[k] = g[k];
	} else {
		while (nk < 4) {
			int open = -1;
			float area = -1.0f;
			for (uint32_t k = 0; k < nk; k++) {
				if (c[kids[k]].leaf) continue;
				const float a = half_area(c[kids[k]].lo, c[kids[k]].hi);
				if (open < 0 || a > area) open = (int)k, area = a; // NaN / inf areas (hostile input) still pick somebody
			}
			if (open < 0) break;
			const uint32_t o = kids[open];
			kids[open] = o + 1u;
			kids[nk++] = c[o + 1u].skip;
		}
	}
	// the children's blocks lie side by side: the walk finds child k at first + k
	const uint32_t first = (uint32_t)(w.blocks.size() / 32);
	w.blocks.resize(w.blocks.size() + 32 * (size_t)nk, 0u);
	uint32_t deepest = 0;
	uint32_t tags = 0;
	for (uint32_t k = 0; k < 4; k++) {
		if (k >= nk) {
			tags |= k << (8 * k);
			continue;
		}
		uint32_t sub = 0;
		const uint32_t ref = fold_node(c, kids[k], first + k, balanced, w, sub); // may grow w.blocks: index, do not keep pointers
		if (sub > deepest) deepest = sub;
		tags |= SRT_BVH_TAG(ref, k) << (8 * k);
	}
	w.jobs.push_back({self, {kids[0], kids[1], nk > 2 ? kids[2] : 0u, nk > 3 ? kids[3] : 0u}, nk, tags, first});
	need = deepest + (nk - 1u);
	return self;
}
void BvhBuilder::fold_wide(const std::vector<BvhNode> &c, uint32_t records, bool balanced, Wide &w) {
	w.blocks.clear(), w.inner.clear();
	w.dest.assign(records, 0u);
	w.root = SRT_BVH_NONE, w.need = 0;
	if (c.empty()) return;
	w.blocks.reserve(32 * c.size()); // (every node of the binary hierarchy becomes at most one block)
	w.inner.reserve(c.size() / 2 + 1), w.jobs.reserve(c.size() / 2 + 1);
	w.blocks.resize(32, 0u);
	w.jobs.clear();
	w.root = fold_node(c, 0u, 0u, balanced, w, w.need);
	// the blocks' boxes: every inner block by itself (reads the binary nodes, writes its own 48 bytes), large hierarchies on up
	// to eight threads (10^5 triangles: 22k blocks x 24 bounds rounded outwards and checked)
	uint32_t *blocks = w.blocks.data();
	const size_t nj = w.jobs.size();
	auto run = [&](size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; i++) {
			const Wide::Job &j = w.jobs[i];
			quantise(c, j.kids, j.nk, j.tags, j.first, blocks + 32 * (size_t)j.self);
		}
	};
	const size_t parts = nj >= 4096 ? 8 : 1;
	std::vector<std::future<void>> futs;
	try {
		for (size_t t = 1; t < parts; t++) futs.push_back(std::async(std::launch::async, run, nj * t / parts, nj * (t + 1) / parts));
	} catch (const std::system_error &) { // no more threads: the rest is done here
	}
	run(0, nj / parts);
	for (size_t t = futs.size() + 1; t < parts; t++) run(nj * t / parts, nj * (t + 1) / parts);
	for (auto &f : futs) f.get();
	w.sched.clear(), w.level_off.clear();
}

double BvhBuilder::wide_cost(const std::vector<BvhNode> &c, const Wide &w) {
	if (c.empty() || w.root == SRT_BVH_NONE) return 0.0;
	const double root_h = half_area_d(c[0].lo, c[0].hi);
	double sum = 0.0;
	if (c[0].leaf) sum = root_h * (double)(c[0].leaf >> 28);
	for (const Wide::Job &j : w.jobs) {
		float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
		for (uint32_t k = 0; k < j.nk; k++) {
			const BvhNode &kid = c[j.kids[k]];
			for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], kid.lo[a]), hi[a] = std::max(hi[a], kid.hi[a]);
			if (kid.leaf) sum += half_area_d(kid.lo, kid.hi) * (double)(kid.leaf >> 28);
		}
		sum += half_area_d(lo, hi) * (double)j.nk;
	}
	return cost_of(sum, root_h);
}

void BvhBuilder::Wide::ensure_schedule() {
	if (!level_off.empty() || jobs.empty()) return;
	std::vector<uint32_t> height(blocks.size() / 32, 0u); // leaf blocks: 0
	uint32_t top = 0;
	for (const Job &j : jobs) { // children come before their parent
		uint32_t h = 0;
		for (uint32_t k = 0; k < j.nk; k++) h = std::max(h, height[j.first + k]);
		height[j.self] = h + 1u;
		top = std::max(top, h + 1u);
	}
	level_off.assign(top + 1u, 0u);
	for (const Job &j : jobs) level_off[height[j.self]]++;
	for (uint32_t h = 1, sum = 0; h <= top; h++) { // level_off[h] = end of level h, level_off[h - 1] = its start
		sum += level_off[h];
		level_off[h] = sum;
	}
	sched.resize(jobs.size());
	std::vector<uint32_t> at(level_off.begin(), level_off.end() - 1);
	for (const Job &j : jobs) sched[at[height[j.self] - 1u]++] = j.self;
}

// Appends the model's nodes and triangle order; returns the root's index.
uint32_t BvhBuilder::run(const srt_model &m, const srt_triangle *all, uint32_t first_record) {
	rec_base = first_record;
	load(m, all);
	const uint32_t n0 = (uint32_t)nodes.size();
	build(0, (uint32_t)tris.size(), 1);
	const uint32_t n1 = (uint32_t)nodes.size();
	for (uint32_t i = n0; i < n1; i++)
		if (nodes[i].skip == n1) nodes[i].skip = SRT_BVH_END;
	for (const Tri &t : tris) order.push_back(t.j);
	return n0;
}

uint32_t BvhBuilder::morton_code(const float c[3], const float mlo[3], const float mhi[3]) {
	uint32_t q[3];
	for (int a = 0; a < 3; a++) {
		q[a] = 0u;
		const float ext = mhi[a] - mlo[a];
		if (!(ext > 0.0f) || !std::isfinite(ext)) continue;
		const float f = (c[a] - mlo[a]) * (1024.0f / ext);
		q[a] = f >= 1023.0f ? 1023u : (f > 0.0f ? (uint32_t)(int)f : 0u); // = clamp((int)f, 0, 1023); a NaN (0 * inf) gives 0
	}
	uint32_t code = 0u;
	for (int i = 0; i < 10; i++) code |= (((q[0] >> i) & 1u) << (3 * i + 2)) | (((q[1] >> i) & 1u) << (3 * i + 1)) | (((q[2] >> i) & 1u) << (3 * i));
	return code;
}
void BvhBuilder::morton_order(std::vector<uint32_t> &out) const {
	std::vector<uint64_t> keys(tris.size());
	for (size_t j = 0; j < tris.size(); j++) // (load() leaves tris in triangle order)
		keys[j] = ((uint64_t)(is_finite[j] ? morton_code(tris[j].c, ext_lo, ext_hi) : MORTON_NONFINITE) << 32) | (uint64_t)j;
	std::sort(keys.begin(), keys.end());
	out.resize(keys.size());
	for (size_t r = 0; r < keys.size(); r++) out[r] = (uint32_t)keys[r];
}
uint32_t BvhBuilder::median_key(float c, float clo, float ext) {
	if (!(ext > 0.0f) || !std::isfinite(ext)) return 0u;
	const float f = (c - clo) * (65536.0f / ext);
	return f >= 65535.0f ? 65535u : (f > 0.0f ? (uint32_t)(int)f : 0u);
}
void BvhBuilder::median_order(std::vector<uint32_t> &out) const {
	const uint32_t n = (uint32_t)tris.size();
	if (srt_build_median_levels(n) > SRT_BUILD_MEDIAN_MAX_LEVELS) return morton_order(out);
	out.resize(n);
	for (uint32_t r = 0; r < n; r++) out[r] = r; // (load() leaves tris in triangle order)
	std::vector<uint32_t> keys(n);                // per triangle, of the range it is in
	std::vector<std::pair<uint32_t, uint32_t>> todo;
	todo.emplace_back(0u, n);
	while (!todo.empty()) { // (a range reads what its ancestors left: the order among the ranges of a depth does not matter)
		const uint32_t b = todo.back().first, e = todo.back().second, cnt = e - b;
		todo.pop_back();
		if (cnt <= SRT_BVH_LEAF_MAX) continue;
		float clo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, chi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
		for (uint32_t r = b; r < e; r++) {
			if (!is_finite[out[r]]) continue;
			for (int a = 0; a < 3; a++) clo[a] = std::min(clo[a], tris[out[r]].c[a]), chi[a] = std::max(chi[a], tris[out[r]].c[a]);
		}
		float ext[3];
		for (int a = 0; a < 3; a++) ext[a] = chi[a] - clo[a];
		int a = 0;
		for (int k = 1; k < 3; k++)
			if (ext[k] > ext[a]) a = k;
		for (uint32_t r = b; r < e; r++) keys[out[r]] = is_finite[out[r]] ? median_key(tris[out[r]].c[a], clo[a], ext[a]) : MEDIAN_NONFINITE;
		std::stable_sort(out.begin() + b, out.begin() + e, [&keys](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
		todo.emplace_back(b, b + cnt / 2), todo.emplace_back(b + cnt / 2, e);
	}
}
static BvhBuilder::Stats balanced_into(std::vector<BvhNode> &out, uint32_t b, uint32_t e, uint32_t depth) {
	BvhBuilder::Stats st;
	const uint32_t self = (uint32_t)out.size(), n = e - b;
	out.emplace_back();
	memset(&out[self], 0, sizeof(BvhNode));
	st.max_depth = depth;
	if (n <= SRT_BVH_LEAF_MAX) {
		out[self].leaf = (n << 28) | b;
		st.leaves = 1;
	} else {
		const BvhBuilder::Stats sl = balanced_into(out, b, b + n / 2, depth + 1), sr = balanced_into(out, b + n / 2, e, depth + 1);
		st.leaves = sl.leaves + sr.leaves;
		st.max_depth = std::max(sl.max_depth, sr.max_depth);
	}
	out[self].skip = (uint32_t)out.size();
	return st;
}
BvhBuilder::Stats BvhBuilder::balanced_topology(uint32_t count, std::vector<BvhNode> &out) {
	out.clear();
	if (count == 0) return Stats();
	out.reserve(count); // (at most 2 * ceil(count / 2) - 1 nodes)
	const Stats st = balanced_into(out, 0u, count, 1u);
	const uint32_t end = (uint32_t)out.size();
	for (BvhNode &nd : out)
		if (nd.skip == end) nd.skip = SRT_BVH_END;
	return st;
}

void BvhCacheEntry::set_balanced_topology(uint32_t n) {
	const BvhBuilder::Stats st = BvhBuilder::balanced_topology(n, nodes);
	leaves = st.leaves, depth = st.max_depth;
	balanced = true;
	BvhBuilder::fold_wide(nodes, n, true, wide); // (quantises the zero boxes: every inner block is requantised by the refit)
	order.resize(n);
	for (uint32_t r = 0; r < n; r++) order[r] = r;
	stale = true, order_pending = true;
	cost_built = cost_now = 0.0;
}
void BvhCacheEntry::build_morton(const srt_model &m, const srt_triangle *all) {
	set_balanced_topology(m.num_triangles);
	{
		std::vector<BvhNode> none;
		std::vector<uint32_t> unused;
		BvhBuilder bb(none, unused);
		bb.load(m, all);
		bb.morton_order(order);
	}
	order_pending = false;
	refit_in_place(m, all); // (clears `stale`)
	cost_built = cost_now;
}
void BvhCacheEntry::build_median(const srt_model &m, const srt_triangle *all) {
	set_balanced_topology(m.num_triangles);
	{
		std::vector<BvhNode> none;
		std::vector<uint32_t> unused;
		BvhBuilder bb(none, unused);
		bb.load(m, all);
		bb.median_order(order);
	}
	order_pending = false;
	refit_in_place(m, all); // (clears `stale`)
	cost_built = cost_now;
}
const BvhCacheEntry &BvhCache::balanced_topology(uint32_t count) {
	for (size_t k = 0; k < topologies.size(); k++)
		if (topologies[k].count == count) {
			std::rotate(topologies.begin(), topologies.begin() + k, topologies.begin() + k + 1);
			return topologies.front();
		}
	if (topologies.size() >= 4) topologies.pop_back();
	topologies.emplace(topologies.begin());
	topologies.front().count = count;
	topologies.front().set_balanced_topology(count);
	topologies.front().wide.ensure_schedule();
	return topologies.front();
}

// (re)builds nodes/order from the model and folds them; the fallback keeps every walk inside SRT_BVH_STACK_CAP
void BvhCacheEntry::build(const srt_model &m, const srt_triangle *all) {
	stale = false;
	for (int attempt = balanced ? 1 : 0; attempt < 2; attempt++) {
		nodes.clear(), order.clear();
		BvhBuilder bb(nodes, order);
		if (attempt) bb.sah_depth = 0;
		bb.run(m, all, 0u);
		leaves = bb.leaves, depth = bb.max_depth;
		balanced = attempt != 0;
		BvhBuilder::fold_wide(nodes, m.num_triangles, balanced, wide);
		if (wide.need <= SRT_BVH_STACK_CAP) break; // a balanced tree of < 2^28 triangles needs at most 3 * 15
	}
	cost_built = cost_now = BvhBuilder::wide_cost(nodes, wide);
}
void BvhCacheEntry::refit(const srt_model &m, const srt_triangle *all) {
	stale = false;
	BvhBuilder bb(nodes, order);
	bb.refit(m, all);
	BvhBuilder::fold_wide(nodes, m.num_triangles, balanced, wide);
	if (wide.need > SRT_BVH_STACK_CAP) build(m, all); // the new boxes fold differently: start over
	else cost_now = 0.0;                               // (unknown until somebody asks: scene_prep.cpp under SRT_DEFORM_REFIT)
}
void BvhCacheEntry::refit_in_place(const srt_model &m, const srt_triangle *all) {
	stale = false;
	BvhBuilder bb(nodes, order);
	bb.refit(m, all);
	for (const BvhBuilder::Wide::Job &j : wide.jobs) quantise(nodes, j.kids, j.nk, j.tags, j.first, wide.blocks.data() + 32 * (size_t)j.self);
	cost_now = BvhBuilder::wide_cost(nodes, wide);
}

// 64-bit FNV-1a over 8-byte words (records are 96 B)
uint64_t hash_triangles(const srt_triangle *tris, size_t count) {
	uint64_t h = 0xcbf29ce484222325ull;
	const size_t words = count * sizeof(srt_triangle) / 8;
	for (size_t i = 0; i < words; i++) {
		uint64_t w;
		memcpy(&w, reinterpret_cast<const char *>(tris) + 8 * i, 8);
		h = (h ^ w) * 0x100000001b3ull;
	}
	return h;
}

extern "C" {

int srt_bvh_build_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, srt_bvh_node *nodes_out, size_t nodes_cap,
                       uint32_t *order_out, size_t order_cap, size_t *n_nodes) {
	if (!model || !n_nodes || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		std::vector<BvhNode> nodes;
		std::vector<uint32_t> order;
		if (m.num_triangles > 0) {
			BvhBuilder bb(nodes, order);
			bb.run(m, triangles, 0u);
		}
		*n_nodes = nodes.size();
		if (nodes_out) memcpy(nodes_out, nodes.data(), std::min(nodes.size(), nodes_cap) * sizeof(BvhNode));
		if (order_out) memcpy(order_out, order.data(), std::min(order.size(), order_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, int force_balanced, uint32_t *blocks_out,
                      size_t blocks_cap, uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, int *balanced) {
	if (!model || !n_blocks || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		BvhCacheEntry ent;
		ent.balanced = force_balanced != 0;
		if (m.num_triangles > 0) ent.build(m, triangles);
		*n_blocks = ent.wide.blocks.size() / 32;
		if (root) *root = ent.wide.root;
		if (stack_need) *stack_need = ent.wide.need;
		if (balanced) *balanced = ent.balanced ? 1 : 0;
		if (blocks_out) memcpy(blocks_out, ent.wide.blocks.data(), std::min(ent.wide.blocks.size(), blocks_cap * 32) * sizeof(uint32_t));
		if (dest_out) memcpy(dest_out, ent.wide.dest.data(), std::min(ent.wide.dest.size(), dest_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_wide_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, int force_balanced, uint32_t *order_out, size_t order_cap) {
	if (!model || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		BvhCacheEntry ent;
		ent.balanced = force_balanced != 0;
		if (m.num_triangles > 0) ent.build(m, triangles);
		if (order_out) memcpy(order_out, ent.order.data(), std::min(ent.order.size(), order_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_refit_wide_host(const srt_shape *built, const srt_shape *moved, const srt_triangle *triangles, size_t n_triangles, int force_balanced,
                            uint32_t *blocks_out, size_t blocks_cap, size_t *n_blocks, uint32_t *root) {
	if (!built || !moved || !n_blocks || built->type != SRT_SHAPE_MODEL || moved->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = built->shape.model, &mv = moved->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	if (mv.triangle_index != m.triangle_index || mv.num_triangles != m.num_triangles) return SRT_ERR_INVALID; // only the transform may differ
	try {
		BvhCacheEntry ent;
		ent.balanced = force_balanced != 0;
		if (m.num_triangles > 0) {
			ent.build(m, triangles);
			ent.refit_in_place(mv, triangles);
		}
		*n_blocks = ent.wide.blocks.size() / 32;
		if (root) *root = ent.wide.root;
		if (blocks_out) memcpy(blocks_out, ent.wide.blocks.data(), std::min(ent.wide.blocks.size(), blocks_cap * 32) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_morton_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *order_out, size_t order_cap) {
	if (!model || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		std::vector<BvhNode> none;
		std::vector<uint32_t> order;
		BvhBuilder bb(none, order);
		bb.load(m, triangles);
		bb.morton_order(order);
		if (order_out && !order.empty()) memcpy(order_out, order.data(), std::min(order.size(), order_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_morton_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *blocks_out, size_t blocks_cap,
                             uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, double *cost) {
	if (!model || !n_blocks || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		BvhCacheEntry ent;
		if (m.num_triangles > 0) ent.build_morton(m, triangles);
		*n_blocks = ent.wide.blocks.size() / 32;
		if (root) *root = ent.wide.root;
		if (stack_need) *stack_need = ent.wide.need;
		if (cost) *cost = ent.cost_built;
		if (blocks_out && !ent.wide.blocks.empty()) memcpy(blocks_out, ent.wide.blocks.data(), std::min(ent.wide.blocks.size(), blocks_cap * 32) * sizeof(uint32_t));
		if (dest_out && !ent.wide.dest.empty()) memcpy(dest_out, ent.wide.dest.data(), std::min(ent.wide.dest.size(), dest_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_median_order_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *order_out, size_t order_cap) {
	if (!model || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		std::vector<BvhNode> none;
		std::vector<uint32_t> order;
		BvhBuilder bb(none, order);
		bb.load(m, triangles);
		bb.median_order(order);
		if (order_out && !order.empty()) memcpy(order_out, order.data(), std::min(order.size(), order_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_median_wide_host(const srt_shape *model, const srt_triangle *triangles, size_t n_triangles, uint32_t *blocks_out, size_t blocks_cap,
                             uint32_t *dest_out, size_t dest_cap, size_t *n_blocks, uint32_t *root, uint32_t *stack_need, double *cost) {
	if (!model || !n_blocks || model->type != SRT_SHAPE_MODEL || (n_triangles && !triangles)) return SRT_ERR_INVALID;
	const srt_model &m = model->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return SRT_ERR_INVALID;
	try {
		BvhCacheEntry ent;
		if (m.num_triangles > 0) ent.build_median(m, triangles);
		*n_blocks = ent.wide.blocks.size() / 32;
		if (root) *root = ent.wide.root;
		if (stack_need) *stack_need = ent.wide.need;
		if (cost) *cost = ent.cost_built;
		if (blocks_out && !ent.wide.blocks.empty()) memcpy(blocks_out, ent.wide.blocks.data(), std::min(ent.wide.blocks.size(), blocks_cap * 32) * sizeof(uint32_t));
		if (dest_out && !ent.wide.dest.empty()) memcpy(dest_out, ent.wide.dest.data(), std::min(ent.wide.dest.size(), dest_cap) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

// the checks the two calls below share; `m`, `mv`: the two models
static bool deformed_args_ok(const srt_shape *built, const srt_triangle *built_triangles, const srt_shape *now, const srt_triangle *now_triangles, size_t n_triangles) {
	if (!built || !now || built->type != SRT_SHAPE_MODEL || now->type != SRT_SHAPE_MODEL || (n_triangles && (!built_triangles || !now_triangles))) return false;
	const srt_model &m = built->shape.model, &mv = now->shape.model;
	if ((uint64_t)m.triangle_index + m.num_triangles > n_triangles || m.num_triangles > 0x0fffffffu) return false;
	return mv.triangle_index == m.triangle_index && mv.num_triangles == m.num_triangles; // the transform and the triangles' bytes may differ
}

int srt_bvh_refit_deformed_wide_host(const srt_shape *built, const srt_triangle *built_triangles, const srt_shape *now, const srt_triangle *now_triangles,
                                     size_t n_triangles, int force_balanced, uint32_t *blocks_out, size_t blocks_cap, size_t *n_blocks, uint32_t *root) {
	if (!n_blocks || !deformed_args_ok(built, built_triangles, now, now_triangles, n_triangles)) return SRT_ERR_INVALID;
	const srt_model &m = built->shape.model;
	try {
		BvhCacheEntry ent;
		ent.balanced = force_balanced != 0;
		if (m.num_triangles > 0) {
			ent.build(m, built_triangles);
			ent.refit_in_place(now->shape.model, now_triangles);
		}
		*n_blocks = ent.wide.blocks.size() / 32;
		if (root) *root = ent.wide.root;
		if (blocks_out) memcpy(blocks_out, ent.wide.blocks.data(), std::min(ent.wide.blocks.size(), blocks_cap * 32) * sizeof(uint32_t));
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

int srt_bvh_wide_cost_host(const srt_shape *built, const srt_triangle *built_triangles, const srt_shape *now, const srt_triangle *now_triangles,
                           size_t n_triangles, int force_balanced, double *cost_built, double *cost_now) {
	if (!cost_built || !cost_now || !deformed_args_ok(built, built_triangles, now, now_triangles, n_triangles)) return SRT_ERR_INVALID;
	const srt_model &m = built->shape.model;
	try {
		BvhCacheEntry ent;
		ent.balanced = force_balanced != 0;
		if (m.num_triangles > 0) {
			ent.build(m, built_triangles);
			ent.refit_in_place(now->shape.model, now_triangles);
		}
		*cost_built = ent.cost_built, *cost_now = ent.cost_now;
	} catch (...) { // std::bad_alloc: no C++ exception may cross the C ABI
		return SRT_ERR_INVALID;
	}
	return SRT_OK;
}

} // extern "C"
