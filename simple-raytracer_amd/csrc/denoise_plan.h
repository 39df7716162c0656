// denoise_plan.h — what the denoiser's setters set, and what follows from it, as arithmetic: which launches a filter makes
// (plan_filter), which temporal set-up runs (plan_setup), and the key a staging set of temporal.hip is made under
// (staging_key). Settings in, small structs out; no HIP and no handle (tests/csrc/host_units_check.cpp compiles it with g++).
#ifndef SRT_DENOISE_PLAN_H
#define SRT_DENOISE_PLAN_H

#include <float.h>
#include <stdint.h>

#include <tuple>

#include "../../include/srt_abi.h"

// Everything the srt_set_denoise* setters set (denoise.hip, temporal.hip); one member of the handle
struct DenoiseSettings {
	bool on = false;         // srt_set_denoise
	srt_denoise_params p{};
	bool demod = false;      // srt_set_denoise_demodulation: the passes filter colour / albedo (K >= 1)
	uint32_t sv_min = 0;     // srt_set_denoise_spatial_variance: pixels with fewer samples take their variance from their 7x7 neighbourhood (0: off)
	bool temporal = false;   // srt_set_denoise_temporal
	srt_temporal_params tp{};
	bool illum = false;      // srt_set_denoise_history_illumination: the set-ups rescale a history tap by D_p / D_h
	float clamp_gamma = 0.f; // srt_set_denoise_history_clamp: the set-ups clamp the history colour into mu +- gamma sigma (0: off)
	bool feedback = false;   // srt_set_denoise_history_feedback: pass 1 (K >= 1) writes its colour into the staging set
	bool object_motion = false, vertex_motion = false; // srt_set_denoise_object_motion, and its per-triangle part
	// turning a stage off turns off what is a mode of it (the parameters stay: the next enable sets them)
	void temporal_off() { temporal = illum = feedback = object_motion = vertex_motion = false, clamp_gamma = 0.f; }
	void off() { temporal_off(), on = demod = false, sv_min = 0; }
};

// What a filter launches (denoise.hip filter_front): K passes, the demodulate launch and demodulated passes, the
// spatial-variance launch, pass 1 in its feedback form; and the albedo weight of the passes and of the clamp's bounds launch
struct FilterPlan {
	int K = 0;
	bool demod = false, spatial_var = false, feedback = false;
	float inv_sigma_a2 = 0.f;
};

static inline FilterPlan plan_filter(const DenoiseSettings &s) {
	FilterPlan f;
	f.K = s.p.iterations;
	f.demod = s.demod && f.K >= 1;
	f.spatial_var = s.sv_min > 0 && f.K >= 1;
	f.feedback = s.feedback && s.temporal && f.K >= 1; // pass 1's colour goes into the set the temporal set-up staged
	// in double, clamped to FLT_MAX: in float the square underflows for sigma_albedo below ~5.4e-20 and the inverse is
	// inf, which turns every tap's 0 * inf albedo term into NaN (no pixel filtered); clamped, equal albedos still cost 0
	const double inv = 1.0 / ((double)s.p.sigma_albedo * (double)s.p.sigma_albedo);
	f.inv_sigma_a2 = (float)(inv < (double)FLT_MAX ? inv : (double)FLT_MAX);
	return f;
}

// Which temporal set-up runs (temporal.hip launch_setup), a filter's and a clear's alike. motion_level 0: no shape moved (or
// no object motion, or no history), 1: the per-shape maps, 2: a deformed mesh's vertex tables too; illum: an ILLUM variant;
// clamp: the bounds launch and a CLAMP variant (without a history nothing new is launched)
struct SetupPlan {
	int motion_level = 0;
	bool illum = false, clamp = false;
};

static inline SetupPlan plan_setup(const DenoiseSettings &s, bool history_valid, bool any_moved, bool any_deformed) {
	SetupPlan u;
	const bool motion = s.object_motion && history_valid && any_moved;
	u.motion_level = !motion ? 0 : (s.vertex_motion && any_deformed) ? 2 : 1;
	u.illum = s.illum;
	u.clamp = s.clamp_gamma > 0.f && history_valid;
	return u;
}

// What a staging set is made under. Two keys are equal only if the launches that make the set -- the temporal set-up, the
// bounds launch under the clamp, the filter's front up to pass 1 under the feedback -- are the same kernel instantiations
// with equal parameter blocks, device pointers aside. `serial` stands for what is traced (srt_denoise_count bumps it); a
// field those launches do not read under the plan stays zero, so that changing it leaves the key equal.
struct StagingKey {
	uint64_t serial = 0;
	bool history_valid = false, illum = false, feedback = false, demod = false, pass1_last = false;
	int32_t history_limit = 0, motion_level = 0;
	uint32_t sv_min = 0;
	float normal_threshold = 0.f, depth_threshold = 0.f, clamp_gamma = 0.f, sigma_l = 0.f, sigma_n = 0.f, sigma_z = 0.f, inv_sigma_a2 = 0.f;
	auto tie() const {
		return std::tie(serial, history_valid, illum, feedback, demod, pass1_last, history_limit, motion_level, sv_min, normal_threshold, depth_threshold,
		                clamp_gamma, sigma_l, sigma_n, sigma_z, inv_sigma_a2);
	}
	bool operator==(const StagingKey &o) const { return tie() == o.tie(); }
};

static inline StagingKey staging_key(const DenoiseSettings &s, bool history_valid, bool any_moved, bool any_deformed, uint64_t serial) {
	StagingKey k;
	k.serial = serial;
	if (!s.temporal) return k; // no set-up, no staging set
	const FilterPlan f = plan_filter(s);
	const SetupPlan u = plan_setup(s, history_valid, any_moved, any_deformed);
	k.history_valid = history_valid, k.illum = u.illum, k.motion_level = u.motion_level;
	k.history_limit = s.tp.history_limit, k.normal_threshold = s.tp.normal_threshold, k.depth_threshold = s.tp.depth_threshold;
	if (u.clamp) k.clamp_gamma = s.clamp_gamma;
	// the weights of the bounds launch, and of the front's spatial-variance launch and pass 1
	if (u.clamp || f.feedback) k.sigma_n = s.p.sigma_normal, k.sigma_z = s.p.sigma_depth, k.inv_sigma_a2 = f.inv_sigma_a2;
	if (f.feedback) { // pass 1's instantiation (K = 1: it is the last pass too) and the rest of what the front reads
		k.feedback = true, k.demod = f.demod, k.pass1_last = f.K == 1, k.sigma_l = s.p.sigma_luminance;
		if (f.spatial_var) k.sv_min = s.sv_min;
	}
	return k;
}

#endif
