// frame_pipeline.hip — a two-deep frame pipeline for the interactive loop (/root/reference/src/main.cpp:277-337): the
// interactive loop's render() with frame N's read-back under frame N+1's trace (srt_render_pipelined, srt_pipeline_flush).
#include <cstring>
#include <new>

#include "srt_internal.h"

// per-handle state of this unit, made by the first srt_render_pipelined
struct SrtPipeline {
	hipStream_t copy_stream = nullptr;
	uint8_t *pinned[2] = {nullptr, nullptr};
	uint8_t *dev_argb[2] = {nullptr, nullptr};
	size_t frame_bytes = 0;
	hipEvent_t resolved[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
	long long frames_enqueued = 0, frames_delivered = 0;
};

void srt_pipeline_release(srt_tracer *t) {
	SrtPipeline *c = t->pipeline;
	if (!c) return;
	if (c->copy_stream) {
		(void)hipStreamSynchronize(c->copy_stream);
		(void)hipStreamDestroy(c->copy_stream);
	}
	for (int i = 0; i < 2; i++) {
		if (c->pinned[i]) (void)hipHostFree(c->pinned[i]);
		if (c->dev_argb[i]) (void)hipFree(c->dev_argb[i]);
	}
	for (int i = 0; i < 2; i++) {
		if (c->resolved[i]) (void)hipEventDestroy(c->resolved[i]);
		if (c->copied[i]) (void)hipEventDestroy(c->copied[i]);
	}
	delete c;
	t->pipeline = nullptr;
}

extern "C" {

int srt_render_pipelined(srt_tracer *t, const srt_render_data *options, uint32_t ticks_stopped, uint8_t *argb_out, long long *frame_delivered) {
	if (!t) return SRT_ERR_INVALID;
	if (!argb_out) return fail(t, SRT_ERR_INVALID, "srt_render_pipelined: argb_out is NULL");
	if (!t->pipeline) t->pipeline = new (std::nothrow) SrtPipeline();
	SrtPipeline *c = t->pipeline;
	if (!c) return fail(t, SRT_ERR_INVALID, "out of host memory");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t bytes = (size_t)t->owned_rows * t->width * 4;
	if (!c->copy_stream || c->frame_bytes != bytes) {
		if (c->frames_enqueued != c->frames_delivered) return fail(t, SRT_ERR_STATE, "srt_render_pipelined: partition changed with a frame in flight (srt_pipeline_flush first)");
		if (!c->copy_stream) SRT_HIP(t, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
		for (int i = 0; i < 2; i++) {
			if (c->pinned[i]) (void)hipHostFree(c->pinned[i]);
			if (c->dev_argb[i]) (void)hipFree(c->dev_argb[i]);
			c->pinned[i] = c->dev_argb[i] = nullptr;
			SRT_HIP(t, hipHostMalloc(reinterpret_cast<void **>(&c->pinned[i]), bytes ? bytes : 4, hipHostMallocDefault));
			SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&c->dev_argb[i]), bytes ? bytes : 4));
			if (!c->resolved[i]) SRT_HIP(t, hipEventCreateWithFlags(&c->resolved[i], hipEventDisableTiming));
			if (!c->copied[i]) SRT_HIP(t, hipEventCreateWithFlags(&c->copied[i], hipEventDisableTiming));
		}
		c->frame_bytes = bytes;
	}
	// enqueue frame N: trace + resolve into this frame's own ARGB buffer on the handle's stream, its copy on the copy stream
	const int slot = (int)(c->frames_enqueued & 1);
	int rc = srt_trace_fused(t, options, c->dev_argb[slot], ticks_stopped); // the last reduction resolves into this frame's own image
	if (rc != SRT_OK) return rc;
	if ((rc = srt_exposure_apply_frame(t, ticks_stopped, c->dev_argb[slot])) != SRT_OK) return rc; // exposure.hip: nothing while the feature is off
	if ((rc = srt_selection_apply_frame(t, c->dev_argb[slot])) != SRT_OK) return rc;               // selection.hip: likewise
	SRT_HIP(t, hipEventRecord(c->resolved[slot], t->stream));
	if ((rc = srt_noise_after_resolve(t)) != SRT_OK) return rc; // noise_meter.hip: nothing while the feature is off; the frame's copy does not wait for it
	SRT_HIP(t, hipStreamWaitEvent(c->copy_stream, c->resolved[slot], 0));
	SRT_HIP(t, hipMemcpyAsync(c->pinned[slot], c->dev_argb[slot], bytes, hipMemcpyDeviceToHost, c->copy_stream));
	SRT_HIP(t, hipEventRecord(c->copied[slot], c->copy_stream));
	c->frames_enqueued++;
	// deliver frame N-1 (its trace, resolve and copy ran while the host prepared frame N)
	if (frame_delivered) *frame_delivered = -1;
	if (c->frames_enqueued - c->frames_delivered == 2) {
		const int prev = (int)(c->frames_delivered & 1);
		SRT_HIP(t, hipEventSynchronize(c->copied[prev]));
		memcpy(argb_out, c->pinned[prev], bytes);
		if (frame_delivered) *frame_delivered = c->frames_delivered;
		c->frames_delivered++;
	}
	return SRT_OK;
}

int srt_pipeline_flush(srt_tracer *t, uint8_t *argb_out, long long *frame_delivered) {
	if (!t) return SRT_ERR_INVALID;
	SrtPipeline *c = t->pipeline;
	if (frame_delivered) *frame_delivered = -1;
	if (!c || c->frames_enqueued == c->frames_delivered) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	while (c->frames_enqueued != c->frames_delivered) { // at most two; the caller gets the newest
		const int prev = (int)(c->frames_delivered & 1);
		SRT_HIP(t, hipEventSynchronize(c->copied[prev]));
		if (argb_out) memcpy(argb_out, c->pinned[prev], c->frame_bytes);
		if (frame_delivered) *frame_delivered = c->frames_delivered;
		c->frames_delivered++;
	}
	return SRT_OK;
}

} // extern "C"
