// trace_plan.h — the launch plan of srt_trace as arithmetic: how many samples a batch holds, how a failed allocation shrinks it,
// which samples, buffers and stream batch b of a dispatch takes, how large the chunks of a launch are and how many waves it
// starts. Integers in, small structs out; no HIP and no handle. The steps of srt_trace_fused (srt_abi.hip) call these and do
// what needs the device: reserve_radiance asks for the budget and allocates (plan_batch, plan_batch_halved), wave_slots asks
// for the resident waves, reserve_scan_stacks sizes the scan stacks (plan_scan_waves), launch_batch enqueues one batch
// (plan_batch_slice, plan_launch). The development overrides (-DSRT_DEV_KNOBS builds, read by srt_abi.hip dev_env()) arrive
// as arguments: 0 = not set.
#ifndef SRT_TRACE_PLAN_H
#define SRT_TRACE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifndef SRT_SCAN_PAIRS_PER_LAUNCH
#define SRT_SCAN_PAIRS_PER_LAUNCH 8e12 // srt_trace: ray-triangle pairs one array-scan launch may come to (sample batches)
#endif

// ---- batches of samples: radiance[pixel][sample] must fit the HBM budget ----------
// Samples per batch before anything is allocated. scan_pairs (SRT_SCAN_PAIRS) and force_batch (SRT_FORCE_BATCH): development.
static inline uint32_t plan_batch(size_t pixels, int ns, size_t budget, uint64_t scan_tris, double scan_pairs, int force_batch) {
	uint32_t batch = ns > 0 ? (uint32_t)ns : 0u;
	if (pixels > 0 && batch > 0) {
		size_t fit = budget / (pixels * 12);
		if (fit < 1) fit = 1;
		// the trace kernel numbers the work-items of a launch with 32 bits
		const size_t fit32 = (size_t)0xfffffff0u / pixels;
		if (fit32 < fit) fit = fit32 ? fit32 : 1;
		if (fit < batch) batch = (uint32_t)fit;
		// Array scan of large meshes: a ray that enters a model's box tests every triangle, so one launch over all samples
		// can run for a long time (BASELINE configs[4]: 5.8 s; a denser mesh or more samples: minutes) -- longer than a
		// compute queue should be held. Sample batches bound a launch by SRT_SCAN_PAIRS_PER_LAUNCH ray-triangle pairs counted
		// as if EVERY path entered every box once (~1 s at the measured 9e12 such pairs per second; a launch whose paths all
		// bounce ten times inside a box takes ten times that). A batch ends in a long tail -- the last rays scan a few lanes
		// at a time -- which is why batches overlap (below) and are not made smaller than this: configs[4] at full size,
		// batches of 8 / 16 / 32 samples one after the other 15.0 / - / 7.9 s, overlapped 8.5 / 6.8 / 6.4 s.
		if (scan_tris > 4096) {
			const double per_sample = (double)pixels * (double)scan_tris;
			double pairs = SRT_SCAN_PAIRS_PER_LAUNCH;
			if (scan_pairs > 0.0) pairs = scan_pairs;
			const double cap = pairs / per_sample;
			const uint32_t cap_u = cap < 1.0 ? 1u : (cap > 1e9 ? 0xffffffffu : (uint32_t)cap);
			if (cap_u < batch) batch = cap_u;
		}
		if (force_batch > 0 && (uint32_t)force_batch < batch) batch = (uint32_t)force_batch; // (development: sample batches smaller than the memory asks for)
		// several batches alternate between TWO radiance buffers (below): both must fit the budget
		if (batch < (uint32_t)ns && (size_t)batch * 2 > fit) batch = (uint32_t)(fit / 2 ? fit / 2 : 1);
		if (batch > 4 && (batch & 3u)) batch &= ~3u; // keep the reduce kernel's 16-byte loads aligned
	}
	return batch;
}

// the batch to try after the device could not give the radiance buffers of this one
static inline uint32_t plan_batch_halved(uint32_t batch) { return batch > 8 ? ((batch / 2) & ~3u) : batch / 2; }

static inline uint32_t plan_num_batches(int ns, uint32_t batch) { return batch ? ((uint32_t)ns + batch - 1) / batch : 0u; }

// floats per radiance buffer: a multiple of 4, so that the second buffer's float4 stores stay 16-byte aligned for any pixel count and batch size
static inline size_t plan_radiance_stride(size_t pixels, uint32_t batch) { return ((pixels * (size_t)batch * 3 + 4) + 3) & ~(size_t)3; }

// array scan: the persistent waves the largest launch of a dispatch starts (one block of scan / park stacks each)
static inline size_t plan_scan_waves(int slots, size_t pixels, uint32_t batch) {
	size_t scan_waves = (size_t)slots;
	const unsigned long long most_items = (unsigned long long)pixels * batch;
	const unsigned long long need = (most_items + 63ull) / 64ull;
	if (need < (unsigned long long)scan_waves) scan_waves = (size_t)(need ? need : 1ull);
	return scan_waves;
}

// Batch b of the n_batches = plan_num_batches(ns, batch) a dispatch of ns samples runs as: its samples (the last batch may be
// ragged), its work-items, and which of the two sets of everything a launch writes (radiance buffer, work cursor, per-wave
// counter lines, scan stacks) and of the two batch streams it uses -- set 0 always when the dispatch is one batch.
struct BatchSlice {
	int parity;                     // 0 / 1: even / odd batches of a dispatch of several
	uint32_t first_sample;          // sample index of the batch's first sample
	uint32_t samples;               // samples per pixel in this batch (nbs)
	unsigned long long total_items; // pixels x samples
};

static inline BatchSlice plan_batch_slice(uint32_t b, uint32_t n_batches, size_t pixels, int ns, uint32_t batch) {
	BatchSlice bs;
	bs.parity = n_batches > 1 ? (int)(b & 1u) : 0;
	bs.first_sample = b * batch;
	bs.samples = (uint32_t)ns - bs.first_sample < batch ? (uint32_t)ns - bs.first_sample : batch;
	bs.total_items = (unsigned long long)pixels * bs.samples;
	return bs;
}

struct LaunchPlan {
	uint32_t job_items;   // items a wave takes from the work cursor per atomic
	int num_waves;        // persistent waves of the launch
	uint32_t nbs_magic16; // 16-bit reciprocal of the batch's sample count (tests/csrc/magic_check.cpp)
};

// One launch over total_items = pixels x nbs samples. sub_items: srt_sub_job_items(); slots: resident waves of the device
// (at most SRT_WAVE_CTR_SLOTS). items_per_wave_dev (SRT_ITEMS_PER_WAVE) and cap_subs_dev (SRT_JOB_CAP_SUBS): development.
static inline LaunchPlan plan_launch(unsigned long long total_items, uint32_t nbs, unsigned long long sub_items, int num_cus, int slots, bool has_models,
                                     bool bvh_active, int items_per_wave_dev, int cap_subs_dev) {
	LaunchPlan lp;
	lp.nbs_magic16 = nbs ? (65536u + nbs - 1u) / nbs : 0u;
	// chunks per atomic: ~8 per resident wave for balance, whole sub-jobs (so that every sub-job starts
	// 16-byte aligned in the radiance buffer), at most 5 of them. A dispatch too small for that
	// (an interactive 960x540 frame at 2 spp is 200 items per wave) gets ONE chunk per wave instead:
	// measured 0.39 -> 0.35 ms against two rounds of single sub-jobs.
	const unsigned long long sub = sub_items;
	// A small dispatch ends in the tail of its longest paths, during which every resident wave still
	// issues whole iterations for a few live lanes: round 2 measured fewer, faster waves as the winner there
	// (960x540x2spp: 2 / 3 / 4 / 5 waves per SIMD = 0.28 / 0.27 / 0.30 / 0.31 ms, hence "at least ~320 items per wave");
	// with round 4's loop (full SHADE phases, cheap bookkeeping) every resident wave pays again down to ~190 items
	// each. Never fewer than 2 waves per SIMD.
	unsigned long long items_per_wave = 192ull; // (round 4's kernel, 960x540x2 spp: 128 / 192 / 256 / 320 / 448 items per wave = 0.104 / 0.104 / 0.104 / 0.117 / 0.143 ms)
	if (items_per_wave_dev > 0) items_per_wave = (unsigned long long)items_per_wave_dev;
	unsigned long long slots_b = total_items / items_per_wave;
	if (slots_b < (unsigned long long)num_cus * 8ull) slots_b = (unsigned long long)num_cus * 8ull;
	if (slots_b > (unsigned long long)slots) slots_b = (unsigned long long)slots;
	unsigned long long job = (total_items / (slots_b * 8ull) / sub) * sub;
	if (job < sub) job = ((total_items + slots_b - 1ull) / slots_b + sub - 1ull) / sub * sub;
	if (job < sub) job = sub;
	// Scenes with models: what a chunk costs varies wildly with where it lies (pixels on a glass mesh: ten walks or scans
	// per path; sky pixels: none), and the launch ends when the wave with the last expensive chunk does. Small chunks
	// shorten that tail, but a wave that hops between distant pixels loses the coherence of neighbouring rays (BVH blocks,
	// scans shared by a wave-full): about 2.5 pixels' worth of samples per chunk, between 2 and 8 sub-jobs (BVH: 16). Measured, chunks
	// of 1 / 2 / 5 sub-jobs: BVH walk of the 10^5-triangle mesh at 16 spp 5.1 / 5.0 / 7.2 ms, at 256 spp 63.9 / 46.8 / 39.0;
	// array scan of the two 968-triangle meshes at 32 spp 20.2 / 16.0 / 18.1. At full size (round 3, profiles/README.md),
	// chunks of 4 / 5 / 6 / 8 / 12 / 16 sub-jobs: configs[2] array scan (512 spp, sub-jobs of 64) 134.7 / 128.0 / 124.1 / 121.7 /
	// 125.1 / 130.6 ms, configs[2] BVH (sub-jobs of 128) 43.1 / 40.6 / 38.8 / 37.1 / 37.5 / 38.9 ms; configs[4] BVH (256 spp:
	// 2.5 pixels = 5 sub-jobs) 37.4 / 36.3 / 35.9 / 37.8 / 41.2 / 46.7 ms; configs[4] array scan (36 samples per launch: 2) 1 / 2 / 3
	// sub-jobs 4,524 / 4,508 / 4,593 ms.
	unsigned long long cap_subs = 5ull;
	if (has_models) {
		cap_subs = (5ull * nbs / 2ull + sub - 1ull) / sub;
		// (BVH, sub-jobs of 64: chunks of 10 / 16 sub-jobs configs[2] 39.3 / 35.7 ms, configs[4] 35.7-36.5 / 36.5 ms; sub-jobs of 128
		// and 8: 37.0 / 36.3. Round 4's walks, chunks of 6 / 8 / 10 / 12 / 16 / 24 / 32 sub-jobs -- float boxes: configs[2] 47.1 / 40.7 /
		// 37.5 / 35.8 / 33.7 / 33.5 / 36.0 ms, configs[4] 36.0 / 33.6 / 32.4 / 32.2 / 33.4 / 36.9 / 41.0; boxes as bytes: 46.7 / 40.3 / 37.0 /
		// 35.3 / 33.2 / 33.7 / 35.4 and 33.9 / 31.6 / 30.6 / 31.2 / 31.7 / 36.4 / 40.2: two and a half pixels' worth, at most 16)
		const unsigned long long most = bvh_active ? 16ull : 8ull;
		cap_subs = cap_subs < 2ull ? 2ull : (cap_subs > most ? most : cap_subs);
	}
	if (cap_subs_dev > 0) cap_subs = (unsigned long long)cap_subs_dev;
	const unsigned long long job_cap = cap_subs * sub;
	if (job > job_cap) job = job_cap;
	lp.job_items = (uint32_t)job;
	const unsigned long long waves_needed = (total_items + 63ull) / 64ull;
	lp.num_waves = (int)(waves_needed < slots_b ? waves_needed : slots_b);
	return lp;
}

#endif
