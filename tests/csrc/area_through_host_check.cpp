// area_through_host_check.cpp -- csrc/area_through_host.h (the frame check and the launch grid of X-ray area selection) as a
// stand-alone program for tests/test_area_through_host.py. May be built with -fsanitize=address,undefined and run directly.
// For every case the grid is checked against a walk of its own workgroups: every pixel of the clipped rectangle belongs to
// exactly one (workgroup, wave, lane), marked in a heap array of exactly w * h bytes, so a lane that maps outside the frame is a
// report. argv[1]: a text file, one case per line: w h x0 y0 x1 y1; per case one line "x0 y0 x1 y1 col_groups row_groups blocks"
// goes to stdout, then "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "area_through_host.h"

static int failures = 0;
#define EXPECT(c)                                                 \
	do {                                                          \
		if (!(c)) {                                               \
			fprintf(stderr, "line %d: %s\n", __LINE__, #c);       \
			failures++;                                           \
		}                                                         \
	} while (0)

static srt_area rect(int x0, int y0, int x1, int y1) {
	srt_area a;
	memset(&a, 0, sizeof a);
	a.x0 = x0, a.y0 = y0, a.x1 = x1, a.y1 = y1;
	return a;
}

// the kernels' mapping: workgroup b takes column group b % col_groups of row group b / col_groups, wave k row 4 * row group + k
static void walk(const AreaThroughGrid &g, int w, int h) {
	std::vector<unsigned char> seen((size_t)w * (size_t)h, 0);
	for (uint32_t b = 0; b < g.blocks; b++)
		for (uint32_t wave = 0; wave < 4; wave++)
			for (uint32_t lane = 0; lane < 64; lane++) {
				const int32_t y = g.c[1] + (int32_t)((b / g.col_groups) * 4u + wave), x = g.c[0] + (int32_t)((b % g.col_groups) * 64u + lane);
				if (y < g.c[3] && x < g.c[2]) seen[(size_t)y * (size_t)w + (size_t)x] += 1;
			}
	for (int y = 0; y < h; y++)
		for (int x = 0; x < w; x++) EXPECT(seen[(size_t)y * (size_t)w + (size_t)x] == ((x >= g.c[0] && x < g.c[2] && y >= g.c[1] && y < g.c[3]) ? 1 : 0));
}

int main(int argc, char **argv) {
	if (argc < 2) return 2;
	FILE *f = fopen(argv[1], "r");
	if (!f) return 2;
	int w, h, x0, y0, x1, y1;
	while (fscanf(f, "%d %d %d %d %d %d", &w, &h, &x0, &y0, &x1, &y1) == 6) {
		EXPECT(area_through_frame_check(w, h) == SRT_OK);
		const srt_area a = rect(x0, y0, x1, y1);
		EXPECT(area_check(&a, nullptr) == SRT_OK);
		AreaThroughGrid g;
		area_through_grid(a, w, h, &g);
		EXPECT(g.blocks == g.col_groups * g.row_groups);
		EXPECT((g.blocks == 0) == (g.c[0] >= g.c[2] || g.c[1] >= g.c[3]));
		walk(g, w, h);
		printf("%d %d %d %d %u %u %u\n", g.c[0], g.c[1], g.c[2], g.c[3], g.col_groups, g.row_groups, g.blocks);
	}
	fclose(f);
	// the frame check's edges
	EXPECT(area_through_frame_check(0, 5) == SRT_ERR_INVALID && area_through_frame_check(5, 0) == SRT_ERR_INVALID);
	EXPECT(area_through_frame_check(-1, 5) == SRT_ERR_INVALID && area_through_frame_check(5, -7) == SRT_ERR_INVALID);
	EXPECT(area_through_frame_check(1 << 16, 1 << 15) == SRT_ERR_INVALID); // 2^31 pixels
	EXPECT(area_through_frame_check((1 << 16) - 1, 1 << 15) == SRT_OK);
	EXPECT(area_through_frame_check(0x7fffffff, 1) == SRT_OK && area_through_frame_check(0x7fffffff, 2) == SRT_ERR_INVALID);
	// the largest frames' grids stay below 2^31 workgroups without walking them
	AreaThroughGrid g;
	area_through_grid(rect(-(1 << 30), -(1 << 30), 0x7fffffff, 0x7fffffff), 0x7fffffff, 1, &g);
	EXPECT(g.col_groups == (0x7fffffffu + 63u) / 64u && g.row_groups == 1u && g.blocks == g.col_groups);
	area_through_grid(rect(0, 0, 1, 0x7fffffff), 1, 0x7fffffff, &g);
	EXPECT(g.col_groups == 1u && g.row_groups == (0x7fffffffu + 3u) / 4u && g.blocks == g.row_groups);
	if (failures) return 1;
	puts("ok");
	return 0;
}
