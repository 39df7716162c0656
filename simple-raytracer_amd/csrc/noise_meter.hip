// noise_meter.hip -- noise metering and render-until-converged (include/srt_abi.h srt_set_noise_meter): one pass
// over the canvas and the denoiser's moments turns every pixel into a relative standard error of the mean, bins it, and counts
// the pixels below the threshold. Zeroing the record, the kernel and the record's copy into pinned memory are enqueued on the
// handle's stream; the percentile and the stopping rule are host arithmetic on the copy once its event has passed, so nothing
// here waits for the stream. srt_render_until keeps one interval of dispatches queued behind the check it waits for.
#include <hip/hip_runtime.h>

#include <cmath>

#include "srt_internal.h"
#include "device_math.h" // ballot64, sqrt_ieee
#include "tonemap.h"     // lum, as the moments use it (frame.hip)

// ---------------------------------------------------------------------------------
// The record: SRT_NOISE_RECORD_WORDS dwords, zeroed before every launch
//   hist[256], metered, left_out, below   what the workgroups add into (259 words)
//   T, P, permille, min_samples, threshold, check_every   the metering's stamp, written by the launch's first lane: the host reads
//                                         a record without knowing what the handle has done since it was enqueued
// ---------------------------------------------------------------------------------
#define SRT_NZ_BINS 256
#define SRT_NZ_METERED 256
#define SRT_NZ_LEFT_OUT 257
#define SRT_NZ_BELOW 258
#define SRT_NZ_STAMP 259
#define SRT_NOISE_RECORD_WORDS 265
static_assert(SRT_NOISE_RECORD_WORDS * sizeof(uint32_t) == 1060, "the record is 1,060 bytes");
// Blocks at the most, as srt_exposure_hist_kernel: every block ends with up to 259 global atomics
#define SRT_NZ_GRID_CAP 1024

struct NoiseMeterParams {
	const float4 *canvas;
	const float *moments;
	uint32_t *record;
	uint32_t *argb; // VIEW only
	float Tf, Pf, threshold, floor;
	uint32_t num_pixels;
	int32_t threshold_bin; // VIEW only
	uint32_t stamp[6];
};

// Eight bins per octave over 2^-24 .. 2^8 from the bit pattern of a finite r >= 0: exponent and the three top mantissa bits
__host__ __device__ __forceinline__ int noise_bin(uint32_t bits) {
	const int b = (int)(bits >> 20) - ((127 - 24) << 3);
	return b < 0 ? 0 : b > SRT_NZ_BINS - 1 ? SRT_NZ_BINS - 1 : b;
}

// 256 lanes, a pixel per lane and trip, the trips wave-uniform (the votes need whole waves). A histogram per wave in LDS; where
// the metered lanes of a wave agree on the bin -- a converged region, a flat background -- one lane adds their number. The three
// counts are sums of ballot popcounts, kept in scalar registers until the end. One merge per workgroup into the record.
template <bool VIEW>
__global__ __launch_bounds__(256) void srt_noise_meter_kernel(const NoiseMeterParams p) {
	__shared__ uint32_t bins[4][SRT_NZ_BINS];
	__shared__ uint32_t counts[4][3];
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	for (int k = 0; k < 4; k++) bins[k][threadIdx.x] = 0u;
	__syncthreads();
	if (blockIdx.x == 0 && threadIdx.x < 6) p.record[SRT_NZ_STAMP + threadIdx.x] = p.stamp[threadIdx.x];
	uint32_t n_metered = 0u, n_left_out = 0u, n_below = 0u;
	const size_t stride = (size_t)gridDim.x * 256u;
	for (size_t base = (size_t)blockIdx.x * 256u; base < p.num_pixels; base += stride) {
		const size_t i = base + threadIdx.x;
		const bool active = i < p.num_pixels;
		float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
		float mom = 0.f;
		if (active) c = p.canvas[i], mom = p.moments[i];
		const float L = lum(c.x / p.Tf, c.y / p.Tf, c.z / p.Tf);
		const float m2 = mom / p.Tf;
		float v = m2 - L * L;
		v = (v > 0.0f) ? v : 0.0f;
		const float se = sqrt_ieee(v / p.Pf);
		const float d = (L > p.floor) ? L : p.floor;
		const float r = se / d;
		const bool metered = active && __builtin_isfinite(L) && __builtin_isfinite(m2) && __builtin_isfinite(r);
		const int bin = noise_bin(__float_as_uint(r));
		const unsigned long long mm = ballot64(metered);
		n_metered += (uint32_t)__popcll(mm);
		n_left_out += (uint32_t)__popcll(ballot64(active && !metered));
		n_below += (uint32_t)__popcll(ballot64(metered && r <= p.threshold));
		if (mm) {
			const int first = __ffsll((long long)mm) - 1;
			const int b0 = __builtin_amdgcn_readlane(bin, first);
			if (ballot64(metered && bin != b0) == 0ull) {
				if ((int)lane == first) atomicAdd(&bins[wave][b0], (uint32_t)__popcll(mm));
			} else if (metered) {
				atomicAdd(&bins[wave][bin], 1u);
			}
		}
		if (VIEW && active) {
			int dd = bin - p.threshold_bin + 32;
			dd = dd < 0 ? 0 : dd > 64 ? 64 : dd;
			const uint32_t R = (uint32_t)(dd * 255 / 64);
			p.argb[i] = metered ? (255u | (R << 8) | ((255u - R) << 16)) : (255u | (255u << 8) | (255u << 24));
		}
	}
	if (lane == 0) counts[wave][0] = n_metered, counts[wave][1] = n_left_out, counts[wave][2] = n_below;
	__syncthreads();
	const uint32_t n = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
	if (n) atomicAdd(&p.record[threadIdx.x], n);
	if (threadIdx.x < 3) {
		const uint32_t s = counts[0][threadIdx.x] + counts[1][threadIdx.x] + counts[2][threadIdx.x] + counts[3][threadIdx.x];
		if (s) atomicAdd(&p.record[SRT_NZ_METERED + threadIdx.x], s);
	}
}

namespace {

// 2^(k/8) rounded to float (include/srt_abi.h SRT_NOISE_EIGHTHS)
const float kEighths[8] = SRT_NOISE_EIGHTHS;

bool finite_in(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

int check_params(const srt_noise_params &p) {
	if (!finite_in(p.threshold, 0x1p-24f, 0x1p8f)) return SRT_ERR_INVALID;
	if (!finite_in(p.luminance_floor, 0x1p-20f, 0x1p20f)) return SRT_ERR_INVALID;
	if (p.permille < 1 || p.permille > 1000) return SRT_ERR_INVALID;
	if (p.min_samples < 1u) return SRT_ERR_INVALID;
	if (p.check_every < 1 || p.check_every > 65536) return SRT_ERR_INVALID;
	if (p.reserved[0] != 0 || p.reserved[1] != 0) return SRT_ERR_INVALID;
	return SRT_OK;
}

uint32_t float_bits(float v) {
	uint32_t u;
	memcpy(&u, &v, 4);
	return u;
}

NoiseMeterParams kernel_params(const srt_noise_params &np, const float *canvas, const float *moments, uint32_t *record, uint32_t *argb, size_t num_pixels,
                               uint32_t T, uint32_t P) {
	NoiseMeterParams kp;
	memset(&kp, 0, sizeof kp);
	kp.canvas = reinterpret_cast<const float4 *>(canvas);
	kp.moments = moments;
	kp.record = record;
	kp.argb = argb;
	kp.Tf = (float)T, kp.Pf = (float)P;
	kp.threshold = np.threshold, kp.floor = np.luminance_floor;
	kp.num_pixels = (uint32_t)num_pixels;
	kp.threshold_bin = noise_bin(float_bits(np.threshold));
	kp.stamp[0] = T, kp.stamp[1] = P, kp.stamp[2] = (uint32_t)np.permille, kp.stamp[3] = np.min_samples;
	kp.stamp[4] = float_bits(np.threshold), kp.stamp[5] = (uint32_t)np.check_every;
	return kp;
}

void launch(const NoiseMeterParams &kp, hipStream_t stream) {
	unsigned gx = (unsigned)(((size_t)kp.num_pixels + 255) / 256);
	if (gx > SRT_NZ_GRID_CAP) gx = SRT_NZ_GRID_CAP;
	if (gx < 1) gx = 1;
	if (kp.argb) hipLaunchKernelGGL(srt_noise_meter_kernel<true>, dim3(gx), dim3(256), 0, stream, kp);
	else hipLaunchKernelGGL(srt_noise_meter_kernel<false>, dim3(gx), dim3(256), 0, stream, kp);
}

// the percentile and the stopping rule of one record (host arithmetic; include/srt_abi.h)
void evaluate(const uint32_t *rec, srt_noise_result *out) {
	memset(out, 0, sizeof *out);
	out->metered = rec[SRT_NZ_METERED], out->left_out = rec[SRT_NZ_LEFT_OUT], out->below = rec[SRT_NZ_BELOW];
	out->dispatches = rec[SRT_NZ_STAMP], out->samples = rec[SRT_NZ_STAMP + 1];
	const uint32_t permille = rec[SRT_NZ_STAMP + 2], min_samples = rec[SRT_NZ_STAMP + 3];
	out->level_bin = -1;
	if (out->metered) {
		const uint64_t target = ((uint64_t)out->metered * permille + 999u) / 1000u;
		uint64_t cum = 0;
		int bin = SRT_NZ_BINS - 1;
		for (int k = 0; k < SRT_NZ_BINS; k++) {
			cum += rec[k];
			if (cum >= target) {
				bin = k;
				break;
			}
		}
		out->level_bin = bin;
		out->level = std::ldexp(kEighths[(bin + 1) & 7], ((bin + 1) >> 3) - 24);
	}
	out->converged = (out->metered > 0 && out->samples >= min_samples && (uint64_t)out->below * 1000u >= (uint64_t)permille * out->metered) ? 1 : 0;
}

// why a handle cannot be metered now (NULL: it can)
const char *refusal(const srt_tracer *t) {
	if (!t->nz->on) return "the noise meter is off (srt_set_noise_meter)";
	if (t->world > 1) return "not available on a partitioned handle";
	if (!t->dn.on) return "the denoiser is off: nothing accumulates the moments (srt_set_denoise; iterations = 0 is enough)";
	if (t->dn_T == 0 || t->dn_P == 0) return "nothing traced since the last clear";
	return nullptr;
}

void report(const NoiseState *nz, int slot, srt_noise_result *result, uint32_t *hist) {
	const uint32_t *rec = nz->back[slot].host;
	if (result) evaluate(rec, result);
	if (hist) memcpy(hist, rec, SRT_NZ_BINS * sizeof(uint32_t));
}

} // namespace

int srt_noise_meter_enqueue(srt_tracer *t, uint8_t *view_argb) {
	NoiseState *nz = t->nz;
	uint32_t *rec = nz->record.ptr;
	const int slot = (int)(nz->enqueued & 1u);
	SRT_HIP(t, hipMemsetAsync(rec, 0, SRT_NOISE_RECORD_WORDS * sizeof(uint32_t), t->stream));
	launch(kernel_params(nz->p, t->canvas, t->dn_mom.ptr, rec, reinterpret_cast<uint32_t *>(view_argb), full_pixels(t), t->dn_T, t->dn_P), t->stream);
	SRT_HIP(t, hipGetLastError());
	SRT_HIP(t, nz->back[slot].copy(rec, SRT_NOISE_RECORD_WORDS, t->stream));
	nz->enqueued++;
	return SRT_OK;
}

int srt_noise_after_resolve(srt_tracer *t) {
	NoiseState *nz = t->nz;
	nz->last_ran = false;
	if (!nz->on || refusal(t) || t->dn_T % (uint32_t)nz->p.check_every != 0) return SRT_OK;
	nz->last_ran = true;
	return srt_noise_meter_enqueue(t, nullptr);
}

extern "C" {

int srt_noise_defaults(srt_noise_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->enable = 1;
	out->threshold = 0.05f;
	out->luminance_floor = 0.01f;
	out->permille = 950;
	out->min_samples = 16;
	out->check_every = 4;
	return SRT_OK;
}

int srt_noise_check_host(const srt_noise_params *p) { return p ? check_params(*p) : SRT_ERR_INVALID; }

int srt_noise_evaluate_host(const uint32_t hist[256], const uint32_t counts[3], uint32_t T, uint32_t P, const srt_noise_params *params, srt_noise_result *result) {
	if (!hist || !counts || !params || !result || check_params(*params)) return SRT_ERR_INVALID;
	uint32_t rec[SRT_NOISE_RECORD_WORDS];
	memset(rec, 0, sizeof rec);
	memcpy(rec, hist, SRT_NZ_BINS * sizeof(uint32_t));
	memcpy(rec + SRT_NZ_METERED, counts, 3 * sizeof(uint32_t));
	rec[SRT_NZ_STAMP] = T, rec[SRT_NZ_STAMP + 1] = P, rec[SRT_NZ_STAMP + 2] = (uint32_t)params->permille, rec[SRT_NZ_STAMP + 3] = params->min_samples;
	evaluate(rec, result);
	return SRT_OK;
}

int srt_set_noise_meter(srt_tracer *t, const srt_noise_params *p) {
	if (!t) return SRT_ERR_INVALID;
	NoiseState *nz = t->nz;
	if (!p || !p->enable) { // off: the sites enqueue what they enqueue without the feature; a metering in flight stays readable
		nz->on = false;
		nz->last_ran = false;
		return SRT_OK;
	}
	if (check_params(*p))
		return fail(t, SRT_ERR_INVALID, "srt_set_noise_meter: threshold in [2^-24, 2^8], luminance_floor in [2^-20, 2^20], both finite, permille 1..1000, "
		                                "min_samples >= 1, check_every 1..65536, reserved 0");
	if (t->world > 1) return fail(t, SRT_ERR_STATE, "srt_set_noise_meter: not available on a partitioned handle (srt_set_partition world > 1)");
	if (!t->dn.on) return fail(t, SRT_ERR_STATE, "srt_set_noise_meter: the denoiser is off: nothing accumulates the moments (srt_set_denoise; iterations = 0 is enough)");
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, nz->record.reserve(SRT_NOISE_RECORD_WORDS));
	for (int k = 0; k < 2; k++) SRT_HIP(t, nz->back[k].reserve(SRT_NOISE_RECORD_WORDS));
	nz->p = *p;
	nz->on = true;
	return SRT_OK;
}

int srt_meter_noise(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	if (const char *why = refusal(t)) return fail(t, SRT_ERR_STATE, std::string("srt_meter_noise: ") + why);
	SRT_HIP(t, hipSetDevice(t->device));
	return srt_noise_meter_enqueue(t, nullptr);
}

int srt_resolve_noise_view(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	if (const char *why = refusal(t)) return fail(t, SRT_ERR_STATE, std::string("srt_resolve_noise_view: ") + why);
	SRT_HIP(t, hipSetDevice(t->device));
	return srt_noise_meter_enqueue(t, t->argb.ptr);
}

int srt_poll_noise(srt_tracer *t, srt_noise_result *result, uint32_t hist[256], int *ready) {
	if (!t || !ready) return SRT_ERR_INVALID;
	NoiseState *nz = t->nz;
	*ready = 0;
	if (nz->enqueued == 0) return SRT_OK; // nothing metered yet: a front-end that only polls sees "not ready"
	const int slot = (int)((nz->enqueued - 1) & 1u);
	if (nz->back[slot].pending) {
		SRT_HIP(t, hipSetDevice(t->device));
		const hipError_t e = hipEventQuery(nz->back[slot].done);
		if (e == hipErrorNotReady) return SRT_OK;
		SRT_HIP(t, e);
		nz->back[slot].pending = false;
	}
	*ready = 1;
	report(nz, slot, result, hist);
	return SRT_OK;
}

int srt_read_noise(srt_tracer *t, srt_noise_result *result, uint32_t hist[256]) {
	if (!t) return SRT_ERR_INVALID;
	NoiseState *nz = t->nz;
	if (nz->enqueued == 0) return fail(t, SRT_ERR_STATE, "srt_read_noise: nothing metered on this handle (srt_meter_noise)");
	const int slot = (int)((nz->enqueued - 1) & 1u);
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, nz->back[slot].wait()); // the copy's event alone
	report(nz, slot, result, hist);
	return SRT_OK;
}

int srt_last_meter_ran(const srt_tracer *t, int *ran) {
	if (!t || !ran) return SRT_ERR_INVALID;
	*ran = t->nz->last_ran ? 1 : 0;
	return SRT_OK;
}

int srt_render_until(srt_tracer *t, const srt_render_data *options, uint32_t time_stride, uint32_t max_dispatches, uint8_t *argb_out, srt_noise_result *result,
                     uint32_t *dispatches_done) {
	if (!t) return SRT_ERR_INVALID;
	if (!options || !argb_out || !result || !dispatches_done || max_dispatches == 0)
		return fail(t, SRT_ERR_INVALID, "srt_render_until: NULL argument or max_dispatches == 0");
	NoiseState *nz = t->nz;
	if (!nz->on) return fail(t, SRT_ERR_STATE, "srt_render_until: the noise meter is off (srt_set_noise_meter)");
	if (t->world > 1) return fail(t, SRT_ERR_STATE, "srt_render_until: not available on a partitioned handle");
	if (!t->dn.on) return fail(t, SRT_ERR_STATE, "srt_render_until: the denoiser is off: nothing accumulates the moments (srt_set_denoise)");
	SRT_HIP(t, hipSetDevice(t->device));
	memset(result, 0, sizeof *result);
	result->level_bin = -1;
	*dispatches_done = 0;
	const uint32_t every = (uint32_t)nz->p.check_every;
	srt_render_data rd = *options;
	int waiting = -1; // the slot of the check that is enqueued and not looked at yet
	bool stop = false;
	uint32_t done = 0;
	while (done < max_dispatches && !stop) {
		rd.time = options->time + done * time_stride;
		if (const int rc = srt_trace(t, &rd)) return rc;
		done++;
		if (t->dn_T % every != 0 || t->dn_P < nz->p.min_samples) continue;
		// check k goes behind this dispatch; the host then looks at check k - 1, whose interval the device has had queued since
		const int slot = (int)(nz->enqueued & 1u);
		if (const int rc = srt_noise_meter_enqueue(t, nullptr)) return rc;
		if (waiting >= 0) {
			SRT_HIP(t, nz->back[waiting].wait());
			evaluate(nz->back[waiting].host, result);
			stop = result->converged != 0;
		}
		waiting = slot;
	}
	if (!stop && waiting >= 0) { // max_dispatches: the outstanding check is the last one
		SRT_HIP(t, nz->back[waiting].wait());
		evaluate(nz->back[waiting].host, result);
	}
	*dispatches_done = done;
	// the frame through the handle's ordinary resolving path: the filter (K = 0: the plain resolve's bytes), exposure and bloom
	if (const int rc = srt_resolve_denoised(t, t->dn_T)) return rc;
	return srt_read_argb(t, argb_out);
}

int srt_selftest_noise_meter(srt_tracer *t, const float *canvas_host, const float *moments_host, uint32_t num_pixels, uint32_t T, uint32_t P,
                             const srt_noise_params *params, uint32_t hist_out[256], uint32_t counts_out[3], uint8_t *view_out) {
	if (!t) return SRT_ERR_INVALID;
	if (!canvas_host || !moments_host || !params || !hist_out || !counts_out || num_pixels == 0 || num_pixels > (1u << 24) || T == 0 || P == 0 || check_params(*params))
		return fail(t, SRT_ERR_INVALID, "srt_selftest_noise_meter: bad arguments");
	SRT_HIP(t, hipSetDevice(t->device));
	const size_t n = num_pixels, canvas_bytes = n * 16, plane_bytes = ((n * 4 + 15) / 16) * 16, rec_bytes = ((SRT_NOISE_RECORD_WORDS * 4 + 15) / 16) * 16;
	char *d = nullptr; // [canvas | moments | record | view]
	SRT_HIP(t, hipMalloc(reinterpret_cast<void **>(&d), canvas_bytes + 2 * plane_bytes + rec_bytes));
	float *d_canvas = reinterpret_cast<float *>(d), *d_mom = reinterpret_cast<float *>(d + canvas_bytes);
	uint32_t *d_rec = reinterpret_cast<uint32_t *>(d + canvas_bytes + plane_bytes), *d_view = reinterpret_cast<uint32_t *>(d + canvas_bytes + plane_bytes + rec_bytes);
	uint32_t rec[SRT_NOISE_RECORD_WORDS];
	hipError_t e = hipMemcpyAsync(d_canvas, canvas_host, canvas_bytes, hipMemcpyHostToDevice, t->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_mom, moments_host, n * 4, hipMemcpyHostToDevice, t->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_rec, 0, rec_bytes + plane_bytes, t->stream);
	if (e == hipSuccess) {
		launch(kernel_params(*params, d_canvas, d_mom, d_rec, view_out ? d_view : nullptr, n, T, P), t->stream);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(rec, d_rec, sizeof rec, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess && view_out) e = hipMemcpyAsync(view_out, d_view, n * 4, hipMemcpyDeviceToHost, t->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(t, SRT_ERR_HIP, std::string("srt_selftest_noise_meter: ") + hipGetErrorString(e));
	memcpy(hist_out, rec, SRT_NZ_BINS * sizeof(uint32_t));
	memcpy(counts_out, rec + SRT_NZ_METERED, 3 * sizeof(uint32_t));
	return SRT_OK;
}

} // extern "C"
