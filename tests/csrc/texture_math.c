/* Host build of csrc/detmath.h for tests/texture_ref.py and tests/sky_ref.py: the detmath routines the texture sampler, the sky
 * sampler and the sun lobe use, over arrays. */
#include <stddef.h>
#include <stdint.h>

#include "detmath.h"

void tex_atan2pif(const float *y, const float *x, float *out, size_t n) {
	for (size_t i = 0; i < n; i++) out[i] = dm_atan2pif(y[i], x[i]);
}

/* t: n x 4 texel values (T00, T10, T01, T11), w: n x 4 weights (w00, w10, w01, w11) */
void tex_bilinear(const float *w, const float *t, float *out, size_t n) {
	for (size_t i = 0; i < n; i++) out[i] = dm_bilinear(w[4 * i], t[4 * i], w[4 * i + 1], t[4 * i + 1], w[4 * i + 2], t[4 * i + 2], w[4 * i + 3], t[4 * i + 3]);
}

/* a: n x 3, b: one vector -> dot(a[i], b) */
void tex_dot3(const float *a, const float *b, float *out, size_t n) {
	for (size_t i = 0; i < n; i++) out[i] = dm_dot3(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[0], b[1], b[2]);
}

/* x[i] to the power e, 1 <= e <= 32 */
void tex_powi(const float *x, int e, float *out, size_t n) {
	for (size_t i = 0; i < n; i++) out[i] = dm_powi(x[i], e);
}
