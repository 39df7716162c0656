// exposure.hip -- exposure for the resolve (include/srt_abi.h srt_set_exposure): a luminance histogram of the frame,
// a one-workgroup meter that turns it into the exposure scalar, and the resolve that multiplies with that scalar. The scalar
// lives in device memory and the resolve reads it from there, so a frame -- a pipelined one included -- never waits for the host.
// Everything is enqueued on the handle's stream behind the site's own (plain) resolve, whose ARGB image it overwrites.
#include <hip/hip_runtime.h>

#include <cmath>

#include "srt_internal.h"
#include "tonemap.h" // lum (the histogram), tonemap (the exposed resolve)

// ---------------------------------------------------------------------------------
// The device record: SRT_EXPOSURE_RECORD_WORDS dwords per handle
//   acc[258]   what srt_exposure_hist_kernel adds into: 256 bins, metered pixels, pixels left out (zeroed before every launch)
//   kept[258]  the last metered frame's copy of acc (srt_read_exposure)
//   state      the adaptation state, log2 of the exposure before the bias (float), and whether it holds a metered frame's
//   log2_exposure, exposure   what srt_exposure_resolve_kernel multiplies with, and its log2
// ---------------------------------------------------------------------------------
#define SRT_EX_BINS 256
#define SRT_EX_ACC 0
#define SRT_EX_KEPT 258
#define SRT_EX_STATE 516
#define SRT_EX_HAVE_STATE 517
#define SRT_EX_LOG2 518
#define SRT_EX_EXPOSURE 519
#define SRT_EXPOSURE_RECORD_WORDS 520
// Blocks of srt_exposure_hist_kernel at the most: four per CU of a 256-CU device. Every block ends with up to 256 global
// atomics, so a frame is spread over few blocks whose lanes stride (1920x1080: eight pixels per lane)
#define SRT_EX_HIST_GRID_CAP 1024

struct ExposureHistParams {
	const float4 *source;
	uint32_t *acc;
	float divisor; // (float)num_steps; 1 for the denoised image, which is divided already
	uint32_t num_pixels;
};

struct ExposureMeterParams {
	uint32_t *record;
	float ev, key, adapt, min_ev, max_ev;
	uint32_t low_permille, high_permille;
};

struct ExposureResolveParams {
	const float4 *source;
	uint32_t *argb;
	const float *exposure; // device memory: the meter's result, or 2^ev as srt_set_exposure wrote it
	float divisor;
	uint32_t num_pixels;
};

// Four bins per octave over 2^-32 .. 2^32 from the bit pattern of a finite L > 0: exponent and the two top mantissa bits
__device__ __forceinline__ int exposure_bin(float L) {
	const int b = (int)(__float_as_uint(L) >> 21) - ((127 - 32) << 2);
	return b < 0 ? 0 : b > SRT_EX_BINS - 1 ? SRT_EX_BINS - 1 : b;
}

// One lane per pixel, grid-stride. A histogram per wave in LDS (4 x 256 dwords per workgroup), the non-zero bins of all four
// added to the global record at the end. Integer sums: the result does not depend on the order.
__global__ __launch_bounds__(256) void srt_exposure_hist_kernel(const ExposureHistParams p) {
	__shared__ uint32_t bins[4][SRT_EX_BINS];
	__shared__ uint32_t left_out[4];
	const uint32_t wave = threadIdx.x >> 6;
	for (int k = 0; k < 4; k++) bins[k][threadIdx.x] = 0u;
	if (threadIdx.x < 4) left_out[threadIdx.x] = 0u;
	__syncthreads();
	uint32_t out = 0u;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.num_pixels; i += gridDim.x * blockDim.x) {
		const float4 c = p.source[i];
		const float L = lum(c.x / p.divisor, c.y / p.divisor, c.z / p.divisor);
		if (L > 0.0f && __builtin_isfinite(L)) atomicAdd(&bins[wave][exposure_bin(L)], 1u);
		else out++;
	}
	if (out) atomicAdd(&left_out[wave], out);
	__syncthreads();
	const uint32_t n = bins[0][threadIdx.x] + bins[1][threadIdx.x] + bins[2][threadIdx.x] + bins[3][threadIdx.x];
	if (n) {
		atomicAdd(&p.acc[threadIdx.x], n);
		atomicAdd(&p.acc[SRT_EX_BINS], n); // metered pixels
	}
	if (threadIdx.x == 0) {
		const uint32_t o = left_out[0] + left_out[1] + left_out[2] + left_out[3];
		if (o) atomicAdd(&p.acc[SRT_EX_BINS + 1], o);
	}
}

// One workgroup of 256 lanes, a lane per bin: keeps the histogram for srt_read_exposure, scans it, and lane 0 takes the
// trimmed mean in double in ascending bin order, then the adaptation step. N == 0 (nothing metered) leaves the state alone.
__global__ __launch_bounds__(256) void srt_exposure_meter_kernel(const ExposureMeterParams p) {
	__shared__ uint32_t incl[SRT_EX_BINS];
	const uint32_t b = threadIdx.x;
	const uint32_t own = p.record[SRT_EX_ACC + b];
	p.record[SRT_EX_KEPT + b] = own;
	if (b < 2) p.record[SRT_EX_KEPT + SRT_EX_BINS + b] = p.record[SRT_EX_ACC + SRT_EX_BINS + b];
	incl[b] = own;
	__syncthreads();
	for (uint32_t d = 1; d < SRT_EX_BINS; d <<= 1) { // inclusive prefix sum (the frame has fewer than 2^31 pixels)
		const uint32_t add = b >= d ? incl[b - d] : 0u;
		__syncthreads();
		incl[b] += add;
		__syncthreads();
	}
	if (b != 0) return;
	const uint32_t N = incl[SRT_EX_BINS - 1];
	float state = __uint_as_float(p.record[SRT_EX_STATE]);
	if (N) {
		// the kept mass [lo, hi) of the pixels in ascending luminance; at least one pixel
		const uint64_t lo = (uint64_t)N * p.low_permille / 1000u;
		uint64_t hi = (uint64_t)N * p.high_permille / 1000u;
		if (hi < lo + 1) hi = lo + 1;
		double sum = 0.0;
		uint64_t mass = 0;
		for (uint32_t k = 0; k < SRT_EX_BINS; k++) {
			const uint64_t first = k ? incl[k - 1] : 0u, last = incl[k]; // the bin holds pixels [first, last)
			const uint64_t from = first > lo ? first : lo, to = last < hi ? last : hi;
			if (to > from) {
				sum += (double)(to - from) * (((double)k + 0.5) / 4.0 - 32.0);
				mass += to - from;
			}
		}
		double target = log2((double)p.key) - sum / (double)mass;
		target = target < (double)p.min_ev ? (double)p.min_ev : target > (double)p.max_ev ? (double)p.max_ev : target;
		const double s = p.record[SRT_EX_HAVE_STATE] ? (double)state + (target - (double)state) * (double)p.adapt : target;
		state = (float)s;
		p.record[SRT_EX_STATE] = __float_as_uint(state);
		p.record[SRT_EX_HAVE_STATE] = 1u;
	}
	const float l2 = (float)((double)state + (double)p.ev);
	p.record[SRT_EX_LOG2] = __float_as_uint(l2);
	p.record[SRT_EX_EXPOSURE] = __float_as_uint((float)exp2((double)l2));
}

// srt_resolve_kernel with the exposure between the division and the tone map: products unfused (the unit is built with
// -ffp-contract=off); at exposure 1.0f the bytes are the plain resolve's
__global__ __launch_bounds__(256) void srt_exposure_resolve_kernel(const ExposureResolveParams p) {
	const float e = *p.exposure;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < p.num_pixels; i += gridDim.x * blockDim.x) {
		const float4 c = p.source[i];
		p.argb[i] = tonemap((c.x / p.divisor) * e, (c.y / p.divisor) * e, (c.z / p.divisor) * e);
	}
}

namespace {

bool finite_within(float v, float bound) { return std::isfinite(v) && std::fabs(v) <= bound; }

int check_params(const srt_exposure_params &p) {
	if (p.mode != SRT_EXPOSURE_MANUAL && p.mode != SRT_EXPOSURE_AUTO) return SRT_ERR_INVALID;
	if (!finite_within(p.ev, 32.0f)) return SRT_ERR_INVALID;
	if (!(std::isfinite(p.key) && p.key > 0.0f)) return SRT_ERR_INVALID;
	if (p.low_permille < 0 || p.low_permille > 999) return SRT_ERR_INVALID;
	if (p.high_permille <= p.low_permille || p.high_permille > 1000) return SRT_ERR_INVALID;
	if (!(p.adapt > 0.0f && p.adapt <= 1.0f)) return SRT_ERR_INVALID;
	if (!finite_within(p.min_ev, 32.0f) || !finite_within(p.max_ev, 32.0f) || p.min_ev > p.max_ev) return SRT_ERR_INVALID;
	for (int k = 0; k < 3; k++)
		if (p.reserved[k] != 0) return SRT_ERR_INVALID;
	return SRT_OK;
}

uint32_t float_bits(float v) {
	uint32_t u;
	memcpy(&u, &v, 4);
	return u;
}

// the record, made and zeroed (exposure 1) when the feature is first enabled
int reserve_record(srt_tracer *t) {
	ExposureState *ex = t->ex;
	if (ex->record.ptr) return SRT_OK;
	SRT_HIP(t, ex->record.reserve(SRT_EXPOSURE_RECORD_WORDS));
	SRT_HIP(t, hipMemsetAsync(ex->record.ptr, 0, SRT_EXPOSURE_RECORD_WORDS * sizeof(uint32_t), t->stream));
	SRT_HIP(t, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ex->record.ptr + SRT_EX_EXPOSURE), (int)float_bits(1.0f), 1, t->stream));
	return SRT_OK;
}

int forget_state(srt_tracer *t) {
	ExposureState *ex = t->ex;
	if (!ex->record.ptr) return SRT_OK;
	SRT_HIP(t, hipSetDevice(t->device));
	SRT_HIP(t, hipMemsetAsync(ex->record.ptr + SRT_EX_STATE, 0, 2 * sizeof(uint32_t), t->stream)); // state 0, have_state 0
	return SRT_OK;
}

} // namespace

int srt_exposure_apply(srt_tracer *t, const float *source, float divisor, uint32_t w, uint32_t h, bool picture, uint8_t *argb) {
	ExposureState *ex = t->ex;
	const size_t num_pixels = (size_t)w * h;
	ex->last_exposed = ex->on;
	const bool bloom = srt_bloom_begin(t, picture, num_pixels);
	if (bloom && !ex->on) return srt_bloom_resolve(t, source, divisor, nullptr, w, h, argb); // (x * 1.0f is x)
	if (!ex->on || num_pixels == 0) return SRT_OK;
	uint32_t *rec = ex->record.ptr;
	if (ex->p.mode == SRT_EXPOSURE_AUTO) {
		SRT_HIP(t, hipMemsetAsync(rec + SRT_EX_ACC, 0, (SRT_EX_BINS + 2) * sizeof(uint32_t), t->stream));
		ExposureHistParams hp;
		hp.source = reinterpret_cast<const float4 *>(source);
		hp.acc = rec + SRT_EX_ACC;
		hp.divisor = divisor;
		hp.num_pixels = (uint32_t)num_pixels;
		unsigned gx = (unsigned)((num_pixels + 255) / 256);
		if (gx > SRT_EX_HIST_GRID_CAP) gx = SRT_EX_HIST_GRID_CAP;
		hipLaunchKernelGGL(srt_exposure_hist_kernel, dim3(gx), dim3(256), 0, t->stream, hp);
		ExposureMeterParams mp;
		mp.record = rec;
		mp.ev = ex->p.ev, mp.key = ex->p.key, mp.adapt = ex->p.adapt, mp.min_ev = ex->p.min_ev, mp.max_ev = ex->p.max_ev;
		mp.low_permille = (uint32_t)ex->p.low_permille, mp.high_permille = (uint32_t)ex->p.high_permille;
		hipLaunchKernelGGL(srt_exposure_meter_kernel, dim3(1), dim3(256), 0, t->stream, mp);
	}
	// bloom.hip's composite is the exposed resolve plus the glow: the frame is not written a third time
	if (bloom) return srt_bloom_resolve(t, source, divisor, reinterpret_cast<const float *>(rec + SRT_EX_EXPOSURE), w, h, argb);
	ExposureResolveParams rp;
	rp.source = reinterpret_cast<const float4 *>(source);
	rp.argb = reinterpret_cast<uint32_t *>(argb);
	rp.exposure = reinterpret_cast<const float *>(rec + SRT_EX_EXPOSURE);
	rp.divisor = divisor;
	rp.num_pixels = (uint32_t)num_pixels;
	unsigned gx = (unsigned)((num_pixels + 255) / 256);
	if (gx > 4096) gx = 4096; // as srt_launch_resolve
	hipLaunchKernelGGL(srt_exposure_resolve_kernel, dim3(gx), dim3(256), 0, t->stream, rp);
	SRT_HIP(t, hipGetLastError());
	return SRT_OK;
}

extern "C" {

int srt_exposure_defaults(srt_exposure_params *out) {
	if (!out) return SRT_ERR_INVALID;
	memset(out, 0, sizeof *out);
	out->enable = 1;
	out->mode = SRT_EXPOSURE_AUTO;
	out->ev = 0.0f;
	out->key = 0.18f;
	out->low_permille = 100;
	out->high_permille = 950;
	out->adapt = 1.0f;
	out->min_ev = -16.0f;
	out->max_ev = 16.0f;
	return SRT_OK;
}

int srt_exposure_check_host(const srt_exposure_params *p) { return p ? check_params(*p) : SRT_ERR_INVALID; }

int srt_set_exposure(srt_tracer *t, const srt_exposure_params *p) {
	if (!t) return SRT_ERR_INVALID;
	ExposureState *ex = t->ex;
	if (!p || !p->enable) { // off: the sites launch what they launch without the feature, and the adaptation starts anew
		ex->on = false;
		ex->last_exposed = false;
		return forget_state(t);
	}
	if (check_params(*p))
		return fail(t, SRT_ERR_INVALID, "srt_set_exposure: mode 0 / 1, |ev| <= 32, key > 0, 0 <= low < high <= 1000 permille, 0 < adapt <= 1, "
		                                "-32 <= min_ev <= max_ev <= 32, all finite, reserved 0");
	SRT_HIP(t, hipSetDevice(t->device));
	if (const int rc = reserve_record(t)) return rc;
	if (p->mode == SRT_EXPOSURE_MANUAL) { // no metering: the slot the resolve reads holds 2^ev from here on
		const float e = (float)std::exp2((double)p->ev);
		SRT_HIP(t, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ex->record.ptr + SRT_EX_LOG2), (int)float_bits(p->ev), 1, t->stream));
		SRT_HIP(t, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ex->record.ptr + SRT_EX_EXPOSURE), (int)float_bits(e), 1, t->stream));
	}
	ex->p = *p;
	ex->on = true;
	return SRT_OK;
}

int srt_reset_exposure(srt_tracer *t) {
	if (!t) return SRT_ERR_INVALID;
	return forget_state(t);
}

int srt_read_exposure(srt_tracer *t, float *log2_exposure, float *exposure, uint32_t hist[256], uint32_t counts[2]) {
	if (!t) return SRT_ERR_INVALID;
	uint32_t rec[SRT_EXPOSURE_RECORD_WORDS];
	memset(rec, 0, sizeof rec);
	rec[SRT_EX_EXPOSURE] = float_bits(1.0f); // a handle that never enabled the feature
	SRT_HIP(t, hipSetDevice(t->device));
	if (t->ex->record.ptr) SRT_HIP(t, hipMemcpyAsync(rec, t->ex->record.ptr, sizeof rec, hipMemcpyDeviceToHost, t->stream));
	SRT_HIP(t, hipStreamSynchronize(t->stream));
	if (log2_exposure) memcpy(log2_exposure, rec + SRT_EX_LOG2, 4);
	if (exposure) memcpy(exposure, rec + SRT_EX_EXPOSURE, 4);
	if (hist) memcpy(hist, rec + SRT_EX_KEPT, SRT_EX_BINS * sizeof(uint32_t));
	if (counts) memcpy(counts, rec + SRT_EX_KEPT + SRT_EX_BINS, 2 * sizeof(uint32_t));
	return SRT_OK;
}

int srt_last_resolve_exposed(const srt_tracer *t, int *exposed) {
	if (!t || !exposed) return SRT_ERR_INVALID;
	*exposed = t->ex->last_exposed ? 1 : 0;
	return SRT_OK;
}

} // extern "C"
