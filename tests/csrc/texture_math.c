/* Host build of csrc/detmath.h for tests/texture_ref.py: the two detmath routines the texture sampler uses, over arrays. */
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
