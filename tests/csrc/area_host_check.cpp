// area_host_check.cpp -- csrc/area_host.h (the area block's check, the clip, the lasso rule, the mask) as a stand-alone program
// for tests/test_area_host.py. May be built with -fsanitize=address,undefined and run directly: the mask is written into a heap
// array of exactly w * h bytes, the vertices are read from a heap array of exactly 2 n words, so a step outside either is a report.
// argv[1]: a text file, one case per line: w h x0 y0 x1 y1 n vx0 vy0 vx1 vy1 ...; per case one line of w * h characters 0 / 1
// goes to stdout ("refused" when area_mask refuses it), then the checks of area_check's edges, then "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "area_host.h"

static int failures = 0;
#define EXPECT(c)                                                 \
	do {                                                          \
		if (!(c)) {                                               \
			fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
			failures++;                                           \
		}                                                         \
	} while (0)

static srt_area rect(int x0, int y0, int x1, int y1, unsigned n) {
	srt_area a;
	memset(&a, 0, sizeof a);
	a.x0 = x0, a.y0 = y0, a.x1 = x1, a.y1 = y1, a.n_vertices = n;
	return a;
}

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "r");
	if (!f) return 2;
	int w, h, x0, y0, x1, y1, n;
	while (fscanf(f, "%d %d %d %d %d %d %d", &w, &h, &x0, &y0, &x1, &y1, &n) == 7) {
		int32_t *v = n > 0 ? (int32_t *)malloc(sizeof(int32_t) * 2 * (size_t)n) : nullptr;
		for (int i = 0; i < 2 * n; i++)
			if (fscanf(f, "%d", &v[i]) != 1) return 2;
		const srt_area a = rect(x0, y0, x1, y1, (unsigned)n);
		const size_t px = (size_t)w * (size_t)h;
		uint8_t *mask = (uint8_t *)malloc(px);
		if (area_mask(&a, v, w, h, mask, px) != SRT_OK) {
			puts("refused");
		} else {
			std::vector<char> line(px + 1, 0);
			for (size_t i = 0; i < px; i++) line[i] = mask[i] ? '1' : '0';
			puts(line.data());
			EXPECT(area_mask(&a, v, w, h, mask, px - 1) == SRT_ERR_INVALID); // one byte short
		}
		free(mask);
		free(v);
	}
	fclose(f);
	// ---- area_check at its edges ----
	const int32_t M = SRT_AREA_COORD_MAX;
	std::vector<int32_t> big(2 * SRT_AREA_MAX_VERTICES + 2, 1);
	const int32_t tri[6] = {0, 0, M, -M, -M, M};
	srt_area a = rect(0, 0, 0, 0, 0);
	EXPECT(area_check(&a, nullptr) == SRT_OK);
	EXPECT(area_check(nullptr, nullptr) == SRT_ERR_INVALID);
	a = rect(5, 5, 4, 9, 0);
	EXPECT(area_check(&a, nullptr) == SRT_ERR_INVALID);
	a = rect(5, 5, 9, 4, 0);
	EXPECT(area_check(&a, nullptr) == SRT_ERR_INVALID);
	for (unsigned n_bad : {1u, 2u, SRT_AREA_MAX_VERTICES + 1u, 0xffffffffu}) {
		a = rect(0, 0, 4, 4, n_bad);
		EXPECT(area_check(&a, big.data()) == SRT_ERR_INVALID);
	}
	for (unsigned n_ok : {3u, SRT_AREA_MAX_VERTICES}) {
		a = rect(0, 0, 4, 4, n_ok);
		EXPECT(area_check(&a, big.data()) == SRT_OK);
		EXPECT(area_check(&a, nullptr) == SRT_ERR_INVALID);
	}
	a = rect(-M - 5, 0, M + 5, 4, 3); // (the rectangle has no range of its own)
	EXPECT(area_check(&a, tri) == SRT_OK);
	for (int k = 0; k < 6; k++)
		for (int32_t bad : {M + 1, -M - 1}) {
			int32_t v[6];
			memcpy(v, tri, sizeof v);
			v[k] = bad;
			EXPECT(area_check(&a, v) == SRT_ERR_INVALID);
		}
	a = rect(0, 0, 4, 4, 0);
	a.flags = 1;
	EXPECT(area_check(&a, nullptr) == SRT_ERR_INVALID);
	for (int k = 0; k < 2; k++) {
		a = rect(0, 0, 4, 4, 0);
		a.reserved[k] = 1;
		EXPECT(area_check(&a, nullptr) == SRT_ERR_INVALID);
	}
	// ---- the clip ----
	int32_t c[4];
	area_clip(rect(-M, -M, M, M, 0), 70, 37, c);
	EXPECT(c[0] == 0 && c[1] == 0 && c[2] == 70 && c[3] == 37);
	area_clip(rect(80, 40, 90, 50, 0), 70, 37, c);
	EXPECT(c[0] == c[2] && c[1] == c[3]);
	area_clip(rect(-2147483647 - 1, -5, 2147483647, 3, 0), 70, 37, c);
	EXPECT(c[0] == 0 && c[1] == 0 && c[2] == 70 && c[3] == 3);
	uint8_t one = 7;
	a = rect(0, 0, 1, 1, 0);
	EXPECT(area_mask(&a, nullptr, 0, 1, &one, 1) == SRT_ERR_INVALID && area_mask(&a, nullptr, 1, 1, nullptr, 1) == SRT_ERR_INVALID && one == 7);
	EXPECT(area_mask(&a, nullptr, 1 << 16, 1 << 15, &one, 1) == SRT_ERR_INVALID); // 2^31 pixels
	if (failures) return 1;
	puts("ok");
	return 0;
}
