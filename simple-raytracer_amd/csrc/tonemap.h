// tonemap.h — the per-pixel device helpers the resolve and the denoiser share (frame.hip, denoise.hip, temporal.hip):
// srt_resolve_kernel's ACES fit and byte conversion, the tonemap as srt_denoise_setup_kernel and the passes write it,
// luminance and the finite-colour test. aces1 and to_uchar exist once; the expression around them (divide, fit, sqrt, * 255,
// pack) is written out three times: srt_resolve_kernel and srt_reduce_kernel<false>'s fused resolve in frame.hip divide by
// (float)num_steps and call sqrt_ieee, tonemap() below takes a divided colour and calls __builtin_sqrtf. The three are held
// equal byte for byte, the denoiser's K = 0 bytes being the plain resolve's, by tests/test_gpu_tonemap_edges.py on canvas
// values at every byte boundary and at the non-finite ends (tests/tonemap_cases.py), not by construction.
// Not part of the public ABI.
#ifndef SRT_TONEMAP_H
#define SRT_TONEMAP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detmath.h"

namespace {

__device__ __forceinline__ float aces1(float x) {
	const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
	return dm_clamp((x * (x * a + b)) / (x * (x * c + d) + e), 0.0f, 1.0f);
}
__device__ __forceinline__ uint32_t to_uchar(float v) { return (v == v) ? ((uint32_t)(int)v & 255u) : 0u; }
// srt_resolve_kernel's expressions on an already divided colour (sqrt_ieee there is the correctly rounded square root, as
// __builtin_sqrtf is with hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); memory order A, R, G, B
__device__ __forceinline__ uint32_t tonemap(float x, float y, float z) {
	const float r = __builtin_sqrtf(aces1(x)), g = __builtin_sqrtf(aces1(y)), b = __builtin_sqrtf(aces1(z));
	return 255u | (to_uchar(r * 255.0f) << 8) | (to_uchar(g * 255.0f) << 16) | (to_uchar(b * 255.0f) << 24);
}
__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }
__device__ __forceinline__ bool finite3(float4 c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }

} // namespace

#endif
