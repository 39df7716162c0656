// query_host.h -- the host scaffold the query units share (ray_query.hip, occlusion.hip, selection.hip's ID pass): the check of
// a call's count and flags, the timed span around its launches, the scene as a query kernel takes it, the pick of a kernel's
// <HAS_MODELS, USE_BVH> instantiation with the one-wave-per-64 launch, and the staging allocation (query_stage.h).
#ifndef SRT_QUERY_HOST_H
#define SRT_QUERY_HOST_H

#include <cstring>
#include <string>

#include "query_stage.h"
#include "srt_internal.h"

namespace {

int query_check_count(srt_tracer *t, const char *who, size_t n, uint32_t flags) {
	if (flags & ~SRT_RAYS_UNIT_DIRECTIONS) return fail(t, SRT_ERR_INVALID, std::string(who) + ": unknown flag bits");
	if (n >= ((size_t)1 << 31)) return fail(t, SRT_ERR_INVALID, std::string(who) + ": n must stay below 2^31 rays");
	return SRT_OK;
}

// the timers' span around a query's launches (srt_last_ray_query_ms)
int query_span_begin(srt_tracer *t) {
	t->rq_span.timed = false;
	if (t->timers_in_render) SRT_HIP(t, t->rq_span.begin(t->stream));
	return SRT_OK;
}
int query_span_end(srt_tracer *t) {
	if (t->timers_in_render) SRT_HIP(t, t->rq_span.end(t->stream));
	return SRT_OK;
}

// the scene buffers as a dispatch's, for a kernel that reads no camera: the render data only sizes trace_params_of's camera fields
TraceParams query_scene_params(const srt_tracer *t) {
	srt_render_data rd;
	memset(&rd, 0, sizeof rd);
	rd.width = rd.height = 1;
	return srt_trace_params_for_query(t, &rd);
}

// one lane per item, one wave per workgroup
template <class P>
void query_launch(void (*kernel)(const P), const P &params, uint32_t n, hipStream_t stream) {
	hipLaunchKernelGGL(kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, params);
}
// the instantiation of the kernel template K for the scene of tp, picked as srt_launch_features picks its own
#define SRT_QUERY_KERNEL(K, tp) (!((tp).num_models > 0) ? K<false, false> : (tp).use_bvh != 0 ? K<true, true> : K<true, false>)

// the staging allocation for a call of n items, laid out by query_stage(n)
int query_reserve_stage(srt_tracer *t, size_t n, QueryStage *stage) {
	SRT_HIP(t, hipStreamSynchronize(t->stream)); // (a grown buffer replaces one a queued launch may still use)
	*stage = query_stage(n);
	SRT_HIP(t, t->rq_stage.reserve(stage->total));
	return SRT_OK;
}

} // namespace

#endif
