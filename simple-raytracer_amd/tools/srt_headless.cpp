// srt_headless — drives the mirrored C++ host API (host/tracer.hpp) the way the
// reference's src/main.cpp drives its Tracer, without SDL/ImGui: build a scene with
// Shape/Material/Box/Model, optionally load OBJ/STL models, render N progressive
// frames, write a PPM (save_ppm) and, for tests, raw dumps of inputs and canvas.
//
//   srt_headless [--scene spheres|meshes|empty] [--obj f.obj]... [--stl f.stl]...
//                [--width W --height H --spp S --bounces B --frames N --time T]
//                [--obj-materials] [--out frame.ppm] [--dump prefix] [--parse-only] [--bvh] [--bvh-build device[:MIN]] [--bvh-order morton|median] [--gpus N] [--pipelined] [--skybox sky.ppm] [--denoise K] [--demodulate] [--spatial-variance N] [--temporal] [--history-illumination] [--history-clamp G] [--history-feedback] [--move DX]
// --denoise K: the frames go through the edge-aware denoiser with K a-trous passes (Tracer::set_denoise; with --gpus N the
//                members gather the filter's inputs with the frame and device 0 filters: the same bytes as on one device)
// --demodulate: with --denoise, the passes filter colour / first-hit albedo (Tracer::set_denoise_demodulation); an error without it
// --spatial-variance N: with --denoise, pixels with fewer than N samples take their variance from their 7x7 neighbourhood
//                (Tracer::set_denoise_spatial_variance); an error without it
// --temporal: with --denoise, the denoiser's temporal reprojection (Tracer::set_denoise_temporal)
// --history-illumination: with --temporal, the history is reprojected as illumination (Tracer::set_denoise_history_illumination); an error without it
// --history-clamp G: with --temporal, the reprojected history colour is clamped into mean +- G sigma of the frame's 7x7 neighbourhood
//                (Tracer::set_denoise_history_clamp; 0 < G <= 64, 1 is the library's advice); an error without --temporal
// --history-feedback: with --temporal, the first a-trous pass's output is what enters the history (Tracer::set_denoise_history_feedback);
//                an error without --temporal
// --exposure auto[:EVBIAS] | EV: the bytes go through the exposed resolve (Tracer::set_exposure): metered on the device from every
//                frame's luminance histogram, with an optional bias in stops, or a fixed 2^EV; the exposure is printed at the end
// --bloom [THRESHOLD[:INTENSITY[:LEVELS]]]: the bright part of every frame glows (Tracer::set_bloom): what of the exposed colour
//                lies above THRESHOLD is blurred over LEVELS pyramid levels and added with weight INTENSITY before the tone map;
//                what is left out is the library's default. Works with and without --exposure
// --until-noise THRESHOLD[:MAXDISPATCHES[:PERMILLE]]: instead of --frames N, dispatches of --spp samples accumulate until PERMILLE
//                (default 950) of the pixels have a relative standard error of at most THRESHOLD, or MAXDISPATCHES (default 1024)
//                are done (Tracer::render_until; the time advances by 7919 per dispatch, as in the frame loop). Turns the denoiser on
//                with K = 0 when --denoise is not given: the moments it accumulates are what is metered. Prints T, P and the level.
//                One device only.
// --noise-view f.ppm: the heat map of the final accumulation's noise (Tracer::resolve_noise_view): green four octaves below the
//                threshold, red four above, magenta where the estimate is not finite. Turns the denoiser on like --until-noise.
// --pick-through X,Y[:K] (may be given several times): the first K (default 8, 1 .. 8) hits under the image point in order
//                (Tracer::pick_through): one line per record in --pick's format, then the count. Click-through selection.
// --pick X,Y (may be given several times): after the scene is loaded, the hit under the image point (X, Y) -- continuous pixel
//                coordinates, a pixel's centre is (px + 0.5, py + 0.5) -- through the first frame's camera (Tracer::pick); one line
//                per pick: shape, triangle, material (-1: none), t, position, normal. Then the frames render as before.
// --nearest X,Y,Z[:RADIUS[:SKIP]] (may be given several times): the closest surface to the world point within RADIUS (default:
//                any distance), shape SKIP left out (Tracer::nearest); one line each: shape, triangle, material, distance, the
//                closest point, the feature it lies on (face, vertexN, edgeNM) and the side (front / back).
// --line-of-sight X0,Y0,Z0:X1,Y1,Z1[:GAP] (may be given several times): after the scene is loaded, is the point GAP (default 0)
//                short of (X1, Y1, Z1) visible from (X0, Y0, Z0) (Tracer::occluded); one line per question: `visible`, `occluded`
//                or `invalid`. Then the frames render as before.
// --select I[,J...][:WIDTH[:RRGGBBAA]]: shapes I, J, ... are outlined in every frame (Tracer::set_selection): WIDTH pixels (1..8,
//                default: the library's 2) in the colour RRGGBBAA (hex; default ffa000ff), over the finished bytes; whether the
//                overlay ran is printed at the end
// --ao S[:RADIUS[:BIAS]]: after the frames, the ambient-occlusion pass through the last frame's camera (Tracer::render_ao): S rays per
//                pixel (1, 2, 4, ... 64) within RADIUS (default: no limit) from BIAS (default: the library's 0.001) above the
//                surface; prints `ao: pixels P surfaces H mean M`, M the mean of occluded / S over the pixels with a surface
// --ao-view f.ppm: the pass as a grey picture (Tracer::resolve_ao_view); needs --ao
// --move DX: the camera moves by DX along x every frame and every frame clears the canvas, as the front-end does while moving
// --move-shape I DX: with --temporal, shape I (a sphere, a plane or a model instance) moves by DX along x every frame and every
//                frame clears the canvas, as the front-end does while a gizmo is dragged; turns object motion on
//                (Tracer::set_denoise_object_motion)
//
// --skybox sky.ppm: an 8-bit binary PPM (P6) as the sky, prepared the way the reference prepares assets/skybox.png
//                   (host/skybox.hpp: four channels, rows flipped, pow(byte / 255, 2.2)); default: the synthetic sky.
//
// --texture img.ppm --texture-material N [--texture-scale S] [--texture-nearest]: an 8-bit binary PPM as the albedo texture of
//                   material N, its texels prepared like the sky's (host/skybox.hpp); OBJ models hand their `vt` out as UVs
// --obj-materials: OBJ models keep their `usemtl` groups: the `mtllib` files are read relative to the OBJ (host/parser.hpp
//                   load_mtl), their materials appended to the scene's, and every triangle gets the material of its group
//                   (Tracer::set_triangle_materials); a group whose name no MTL file defines, and everything that is not an
//                   OBJ, keeps the shape's material. A `map_Kd` that names a binary PPM becomes that material's texture
//                   (as --texture); any other kind of file is reported and skipped. --parse-only prints the table's summary.
// --dump prefix writes prefix.{shapes,tris,mats,rd,sd,canvas,argb}.bin (raw records).
// --parse-only skips everything that needs a GPU (loaders + scene construction only).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../host/parser.hpp"
#include "../host/skybox.hpp"
#include "../host/tracer.hpp"

// binary PPM (P6, maxval 255; comments allowed in the header) -> RGB bytes, first row = top of the picture
static bool load_ppm(const std::string &path, std::vector<uint8_t> &rgb, int &w, int &h) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	std::string magic;
	f >> magic;
	if (magic != "P6") return false;
	int vals[3], got = 0;
	while (got < 3 && f) {
		f >> std::ws;
		if (f.peek() == '#') {
			std::string line;
			std::getline(f, line);
			continue;
		}
		f >> vals[got++];
	}
	if (got < 3 || vals[0] <= 0 || vals[1] <= 0 || vals[2] != 255) return false;
	f.get(); // the single whitespace byte behind maxval
	w = vals[0], h = vals[1];
	rgb.resize((size_t)w * h * 3);
	f.read(reinterpret_cast<char *>(rgb.data()), (std::streamsize)rgb.size());
	return (size_t)f.gcount() == rgb.size();
}

// same integer formula as simple-raytracer_amd/scenes.py synthetic_sky()
static std::vector<float> synthetic_sky(int w, int h) {
	std::vector<float> out((size_t)w * h * 4);
	const long horizon = h / 2;
	auto clampi = [](long v) { return v < 0 ? 0L : (v > 255 ? 255L : v); };
	for (long y = 0; y < h; y++)
		for (long x = 0; x < w; x++) {
			long up = y - horizon > 0 ? y - horizon : 0;
			long cloud = (((x * 5 + y * 3) >> 5) ^ ((x * 3 - y * 7) >> 6)) & 31;
			long base = y < horizon ? 70 + (y * 40) / (horizon > 1 ? horizon : 1) : 230 - (up * 120) / ((h - horizon) > 1 ? (h - horizon) : 1);
			long r = clampi(base - 40 + cloud), g = clampi(base - 10 + cloud);
			long b = y < horizon ? clampi(base - 20 + cloud) : clampi(base + 20 + cloud / 2);
			float *t = &out[((size_t)y * w + x) * 4];
			t[0] = (float)(r * r) / 65025.0f;
			t[1] = (float)(g * g) / 65025.0f;
			t[2] = (float)(b * b) / 65025.0f;
			t[3] = 1.0f;
		}
	return out;
}

// The front-end's camera convention: camera_to_world carries the eye position in
// column 3 and the yaw-then-pitch rotation in the upper 3x3.
static glm::mat4 eye_matrix(const glm::vec3 &eye, float yaw, float pitch) {
	return glm::translate(eye) * glm::eulerAngleYXZ(yaw, pitch, 0.0f);
}

// the scene's material table; the names only matter to a GUI, so the tool keeps none
struct MaterialTable {
	std::vector<Material> list;
	int add(const Material &m) {
		list.push_back(m);
		return (int)list.size() - 1;
	}
	int size() const { return (int)list.size(); }
};

template <class T>
static void dump(const std::string &path, const T *data, size_t count) {
	std::ofstream f(path, std::ios::binary);
	f.write(reinterpret_cast<const char *>(data), (std::streamsize)(count * sizeof(T)));
}

int main(int argc, char **argv) {
	std::string scene = "spheres", out, dump_prefix, skybox_path, texture_path;
	int texture_material = -1;
	float texture_scale = 1.0f;
	bool texture_nearest = false;
	std::vector<std::string> objs, stls;
	int width = 256, height = 256, spp = 16, bounces = 10, frames = 1;
	unsigned time_seed = 12345;
	bool parse_only = false, bvh = false, pipelined = false, obj_materials = false;
	int gpus = 1, denoise = -1, spatial_variance = 0;
	bool temporal = false, demodulate = false, history_illumination = false, history_feedback = false;
	float history_clamp = 0.0f;
	bool clamp_given = false;
	bool exposure = false, exposure_auto = false;
	float exposure_ev = 0.0f;
	bool bloom = false;
	std::vector<uint32_t> selected; // --select
	srt_area area{};                // --select-area, --lasso
	bool select_area = false;
	bool area_through = false;      // --through: the X-ray counts (srt_area_coverage_through)
	int area_mode = SRT_SELECT_REPLACE;
	unsigned area_min_pixels = 1;
	std::vector<int32_t> lasso;
	float select_width = 0.0f;      // (0: the library's default)
	uint32_t select_colour = 0xffa000ffu;
	float bloom_threshold = -1.0f, bloom_intensity = -1.0f; // (negative: the library's default)
	int bloom_levels = 0;
	bool until_noise = false;
	float noise_threshold = 0.0f; // (0: the library's default)
	long noise_max = 1024;
	int noise_permille = 0;
	std::string noise_view;
	int ao_samples = 0; // --ao
	float ao_radius = 0.0f, ao_bias = -1.0f;
	std::string ao_view;
	float move = 0.0f, shape_move = 0.0f;
	int move_shape = -1;
	bool moving = false;
	bool bvh_build_device = false;
	uint32_t bvh_build_min = 0;
	int bvh_order = SRT_BUILD_ORDER_MORTON;
	std::vector<float> picks; // --pick X,Y: x0, y0, x1, y1, ...
	std::vector<float> through;      // --pick-through X,Y[:K]: x0, y0, x1, y1, ...
	std::vector<unsigned> through_k; // ... its K
	std::vector<srt_point_query> nearests; // --nearest X,Y,Z[:RADIUS[:SKIP]]
	std::vector<uint32_t> nearest_skips;   // ... its SKIP (SRT_HIT_NONE: none)
	std::vector<srt_segment> sights; // --line-of-sight
	for (int i = 1; i < argc; i++) {
		std::string a = argv[i];
		auto next = [&]() -> const char * {
			if (i + 1 >= argc) {
				std::cerr << "missing value for " << a << "\n";
				std::exit(2);
			}
			return argv[++i];
		};
		if (a == "--scene") scene = next();
		else if (a == "--obj") objs.push_back(next());
		else if (a == "--stl") stls.push_back(next());
		else if (a == "--width") width = std::atoi(next());
		else if (a == "--height") height = std::atoi(next());
		else if (a == "--spp") spp = std::atoi(next());
		else if (a == "--bounces") bounces = std::atoi(next());
		else if (a == "--frames") frames = std::atoi(next());
		else if (a == "--time") time_seed = (unsigned)std::strtoul(next(), nullptr, 10);
		else if (a == "--out") out = next();
		else if (a == "--dump") dump_prefix = next();
		else if (a == "--parse-only") parse_only = true;
		else if (a == "--bvh") bvh = true;
		else if (a == "--bvh-build") { // device[:MIN] | host
			const std::string v = next();
			if (v == "host") bvh_build_device = false;
			else if (v.rfind("device", 0) == 0 && (v.size() == 6 || v[6] == ':')) {
				bvh_build_device = true;
				bvh_build_min = v.size() > 7 ? (uint32_t)std::strtoul(v.c_str() + 7, nullptr, 10) : 0u;
			} else {
				std::cerr << "--bvh-build takes host or device[:MIN]\n";
				return 2;
			}
		}
		else if (a == "--bvh-order") { // morton | median
			const std::string v = next();
			if (v == "morton") bvh_order = SRT_BUILD_ORDER_MORTON;
			else if (v == "median") bvh_order = SRT_BUILD_ORDER_MEDIAN;
			else {
				std::cerr << "--bvh-order takes morton or median\n";
				return 2;
			}
		}
		else if (a == "--obj-materials") obj_materials = true;
		else if (a == "--gpus") gpus = std::atoi(next());
		else if (a == "--pipelined") pipelined = true;
		else if (a == "--skybox") skybox_path = next();
		else if (a == "--texture") texture_path = next();
		else if (a == "--texture-material") texture_material = std::atoi(next());
		else if (a == "--texture-scale") texture_scale = std::strtof(next(), nullptr);
		else if (a == "--texture-nearest") texture_nearest = true;
		else if (a == "--denoise") denoise = std::atoi(next());
		else if (a == "--demodulate") demodulate = true;
		else if (a == "--spatial-variance") spatial_variance = std::atoi(next());
		else if (a == "--temporal") temporal = true;
		else if (a == "--history-illumination") history_illumination = true;
		else if (a == "--history-clamp") history_clamp = std::strtof(next(), nullptr), clamp_given = true;
		else if (a == "--history-feedback") history_feedback = true;
		else if (a == "--exposure") { // auto[:EVBIAS] | EV
			const std::string v = next();
			char *end = nullptr;
			exposure = true;
			exposure_auto = v.rfind("auto", 0) == 0;
			const char *num = exposure_auto ? (v.size() > 4 && v[4] == ':' ? v.c_str() + 5 : "") : v.c_str();
			exposure_ev = *num ? std::strtof(num, &end) : 0.0f;
			if ((exposure_auto && v.size() > 4 && v[4] != ':') || (!exposure_auto && !*num) || (*num && (!end || *end)) || !(exposure_ev >= -32.0f && exposure_ev <= 32.0f)) {
				std::cerr << "--exposure takes auto, auto:EVBIAS or EV, |EV| <= 32\n";
				return 2;
			}
		}
		else if (a == "--bloom") { // [THRESHOLD[:INTENSITY[:LEVELS]]]: the value is optional, the library's defaults fill the rest
			bloom = true;
			if (i + 1 < argc && std::strncmp(argv[i + 1], "--", 2) != 0) {
				const std::string v = argv[++i];
				char *end = nullptr;
				bloom_threshold = std::strtof(v.c_str(), &end);
				if (end && *end == ':') bloom_intensity = std::strtof(end + 1, &end);
				if (end && *end == ':') bloom_levels = (int)std::strtol(end + 1, &end, 10);
				if (!end || *end || end == v.c_str()) {
					std::cerr << "--bloom takes nothing, THRESHOLD, THRESHOLD:INTENSITY or THRESHOLD:INTENSITY:LEVELS\n";
					return 2;
				}
			}
		}
		else if (a == "--until-noise") { // THRESHOLD[:MAXDISPATCHES[:PERMILLE]]
			const std::string v = next();
			char *end = nullptr;
			until_noise = true;
			noise_threshold = std::strtof(v.c_str(), &end);
			if (end && *end == ':') noise_max = std::strtol(end + 1, &end, 10);
			if (end && *end == ':') noise_permille = (int)std::strtol(end + 1, &end, 10);
			if (!end || *end || end == v.c_str() || !(noise_threshold > 0.0f) || noise_max < 1 || noise_permille < 0) {
				std::cerr << "--until-noise takes THRESHOLD, THRESHOLD:MAXDISPATCHES or THRESHOLD:MAXDISPATCHES:PERMILLE\n";
				return 2;
			}
		}
		else if (a == "--noise-view") noise_view = next();
		else if (a == "--ao") { // S[:RADIUS[:BIAS]]
			const std::string v = next();
			char *end = nullptr;
			ao_samples = (int)std::strtol(v.c_str(), &end, 10);
			bool ok = end != v.c_str() && ao_samples >= 1 && ao_samples <= 64 && (ao_samples & (ao_samples - 1)) == 0;
			if (ok && *end == ':') {
				ao_radius = std::strtof(end + 1, &end);
				ok = ao_radius > 0.0f;
				if (ok && *end == ':') {
					ao_bias = std::strtof(end + 1, &end);
					ok = ao_bias >= 0.0f && std::isfinite(ao_bias);
				}
			}
			if (!ok || *end) {
				std::cerr << "--ao takes S, S:RADIUS or S:RADIUS:BIAS; S one of 1, 2, 4, 8, 16, 32, 64, RADIUS > 0, BIAS >= 0\n";
				return 2;
			}
		}
		else if (a == "--ao-view") ao_view = next();
		else if (a == "--select") { // I[,J...][:WIDTH[:RRGGBBAA]]
			const std::string v = next();
			const char *c = v.c_str();
			char *end = nullptr;
			bool ok = true;
			for (;;) {
				const unsigned long i = std::strtoul(c, &end, 10);
				ok = ok && end != c && i <= 0xfffffffeul;
				if (!ok) break;
				selected.push_back((uint32_t)i);
				if (*end != ',') break;
				c = end + 1;
			}
			if (ok && *end == ':') {
				c = end + 1;
				select_width = std::strtof(c, &end);
				ok = end != c && select_width >= 1.0f && select_width <= 8.0f;
				if (ok && *end == ':') {
					c = end + 1;
					select_colour = (uint32_t)std::strtoul(c, &end, 16);
					ok = end - c == 8;
				}
			}
			if (!ok || *end) {
				std::cerr << "--select takes I[,J...], I[,J...]:WIDTH or I[,J...]:WIDTH:RRGGBBAA, 1 <= WIDTH <= 8\n";
				return 2;
			}
		}
		else if (a == "--select-area") { // X0,Y0:X1,Y1[:MODE[:MINPIXELS]]
			char mode[16] = "replace";
			const int got = std::sscanf(next(), "%d,%d:%d,%d:%15[a-z]:%u", &area.x0, &area.y0, &area.x1, &area.y1, mode, &area_min_pixels);
			const std::string m = mode;
			area_mode = m == "replace" ? SRT_SELECT_REPLACE : m == "add" ? SRT_SELECT_ADD : m == "subtract" ? SRT_SELECT_SUBTRACT : m == "toggle" ? SRT_SELECT_TOGGLE : -1;
			if (got < 4 || area_mode < 0 || area.x1 < area.x0 || area.y1 < area.y0) {
				std::cerr << "--select-area takes X0,Y0:X1,Y1[:MODE[:MINPIXELS]], X0 <= X1, Y0 <= Y1, MODE replace, add, subtract or toggle\n";
				return 2;
			}
			select_area = true;
		}
		else if (a == "--through") area_through = true;
		else if (a == "--lasso") { // X,Y;X,Y;...
			const std::string v = next();
			const char *c = v.c_str();
			int x = 0, y = 0, used = 0;
			while (std::sscanf(c, "%d,%d%n", &x, &y, &used) == 2) {
				lasso.push_back(x), lasso.push_back(y);
				c += used;
				if (*c != ';') break;
				c++;
			}
			if (*c || lasso.size() < 6 || lasso.size() > 2 * SRT_AREA_MAX_VERTICES) {
				std::cerr << "--lasso takes X,Y;X,Y;... with 3 to 256 pixel-corner vertices\n";
				return 2;
			}
		}
		else if (a == "--pick") { // X,Y
			float x = 0.f, y = 0.f;
			if (std::sscanf(next(), "%f,%f", &x, &y) != 2) {
				std::cerr << "--pick takes X,Y\n";
				return 2;
			}
			picks.push_back(x), picks.push_back(y);
		}
		else if (a == "--pick-through") { // X,Y[:K]
			float x = 0.f, y = 0.f;
			unsigned k = SRT_MULTI_HIT_MAX;
			if (std::sscanf(next(), "%f,%f:%u", &x, &y, &k) < 2 || k < 1u || k > SRT_MULTI_HIT_MAX) {
				std::cerr << "--pick-through takes X,Y[:K] with K in 1 .. 8\n";
				return 2;
			}
			through.push_back(x), through.push_back(y), through_k.push_back(k);
		}
		else if (a == "--nearest") { // X,Y,Z[:RADIUS[:SKIP]]
			srt_point_query pq{{0.f, 0.f, 0.f}, INFINITY};
			unsigned skip = SRT_HIT_NONE;
			if (std::sscanf(next(), "%f,%f,%f:%f:%u", &pq.point[0], &pq.point[1], &pq.point[2], &pq.max_distance, &skip) < 3) {
				std::cerr << "--nearest takes X,Y,Z[:RADIUS[:SKIP]]\n";
				return 2;
			}
			nearests.push_back(pq), nearest_skips.push_back(skip);
		}
		else if (a == "--line-of-sight") { // X0,Y0,Z0:X1,Y1,Z1[:GAP]
			srt_segment sg{};
			if (std::sscanf(next(), "%f,%f,%f:%f,%f,%f:%f", &sg.from[0], &sg.from[1], &sg.from[2], &sg.to[0], &sg.to[1], &sg.to[2], &sg.end_gap) < 6) {
				std::cerr << "--line-of-sight takes X0,Y0,Z0:X1,Y1,Z1[:GAP]\n";
				return 2;
			}
			sights.push_back(sg);
		}
		else if (a == "--move") move = std::strtof(next(), nullptr), moving = true;
		else if (a == "--move-shape") move_shape = std::atoi(next()), shape_move = std::strtof(next(), nullptr);
		else {
			std::cerr << "usage: srt_headless [--scene spheres|meshes|empty] [--obj f]... [--stl f]... [--width W --height H --spp S "
			             "--bounces B --frames N --time T] [--out f.ppm] [--dump prefix] [--parse-only] [--bvh] [--bvh-build device[:MIN]] [--bvh-order morton|median] [--gpus N] [--pipelined] [--skybox sky.ppm] "
			             "[--denoise K] [--demodulate] [--spatial-variance N] [--temporal] [--history-illumination] [--history-clamp G] [--history-feedback] [--exposure auto[:EVBIAS]|EV] [--bloom [THRESHOLD[:INTENSITY[:LEVELS]]]] [--until-noise THRESHOLD[:MAXDISPATCHES[:PERMILLE]]] [--noise-view f.ppm] [--ao S[:RADIUS[:BIAS]]] [--ao-view f.ppm] [--select I[,J...][:WIDTH[:RRGGBBAA]]] [--select-area X0,Y0:X1,Y1[:MODE[:MINPIXELS]] [--lasso X,Y;X,Y;...] [--through]] [--pick X,Y]... [--pick-through X,Y[:K]]... [--nearest X,Y,Z[:RADIUS[:SKIP]]]... [--line-of-sight X0,Y0,Z0:X1,Y1,Z1[:GAP]]... [--move DX] [--move-shape I DX] [--texture img.ppm --texture-material N [--texture-scale S] [--texture-nearest]] [--obj-materials]\n";
			return 2;
		}
	}

	if (demodulate && denoise < 0) {
		std::cerr << "--demodulate needs --denoise K\n";
		return 2;
	}
	if (spatial_variance != 0 && (denoise < 0 || spatial_variance < 0)) {
		std::cerr << "--spatial-variance N needs --denoise K and N >= 0\n";
		return 2;
	}
	if (history_illumination && (!temporal || denoise < 0)) {
		std::cerr << "--history-illumination needs --denoise K --temporal\n";
		return 2;
	}
	if (clamp_given && (!temporal || denoise < 0 || !(history_clamp > 0.0f && history_clamp <= 64.0f))) {
		std::cerr << "--history-clamp G needs --denoise K --temporal and 0 < G <= 64\n";
		return 2;
	}
	if (history_feedback && (!temporal || denoise < 0)) {
		std::cerr << "--history-feedback needs --denoise K --temporal\n";
		return 2;
	}
	if (temporal && denoise < 0) {
		std::cerr << "--temporal needs --denoise K\n";
		return 2;
	}
	if (!ao_view.empty() && ao_samples == 0) {
		std::cerr << "--ao-view needs --ao S\n";
		return 2;
	}
	if ((until_noise || !noise_view.empty()) && gpus > 1) {
		std::cerr << "--until-noise and --noise-view run on one device (--gpus 1): a group has no render-until call\n";
		return 2;
	}
	if (until_noise && (pipelined || moving || move_shape >= 0)) {
		std::cerr << "--until-noise accumulates one still frame: not with --pipelined, --move or --move-shape\n";
		return 2;
	}
	if ((until_noise || !noise_view.empty()) && denoise < 0) denoise = 0; // the moments are the denoiser's; K = 0 keeps the plain resolve's bytes

	// ---- scene construction, as src/main.cpp:95-126 does it ----
	std::vector<Shape> shapes;
	std::vector<Triangle> triangles;
	MaterialTable materials;
	Box::create_triangle(triangles);

	if (scene == "spheres") {
		materials.add(Material(Color(0.8f, 0.8f, 0.9f)));
		materials.add(Material(Color(0.9f, 0.3f, 0.3f)));
		materials.add(Material(Color(0.3f, 0.9f, 0.4f)));
		materials.add(Material(Color(0.9f, 0.95f, 1.0f)));
		materials.add(Material(color::white, 1.0f, 0.0f, 0.0f, 1.0f, 1.5f));
		materials.add(Material(Color(0.2f, 0.3f, 0.9f), 1.0f, 1.0f));
		materials.add(Material(color::white, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, Color(1.0f, 0.2f, 0.2f), 5.0f));
		shapes.push_back(Shape(0, Plane({0, -1, 0}, {0, 1, 0})));
		shapes.push_back(Shape(1, Plane({-4, 0, 0}, {1, 0, 0})));
		shapes.push_back(Shape(2, Plane({0, 0, -6}, {0, 0, 1})));
		shapes.push_back(Shape(3, Sphere({-2, 0, -1}, 1.5f)));
		shapes.push_back(Shape(4, Sphere({0.5f, 0.8f, -3}, 1.0f)));
		shapes.push_back(Shape(5, Sphere({2.5f, 0.5f, -1.5f}, 1.0f)));
		shapes.push_back(Shape(6, Sphere({0.6f, -1, 0}, 0.6f)));
	} else if (scene == "meshes") {
		materials.add(Material(Color(0.8f, 0.8f, 0.8f)));
		materials.add(Material(Color(0.4f, 0.9f, 0.5f), 1.0f, 0.0f, 0.0f, 1.0f, 1.3f));
		materials.add(Material(Color(0.9f, 0.7f, 0.3f), 0.7f, 0.6f));
		shapes.push_back(Shape(0, Plane({0, -1.2f, 0}, {0, 1, 0})));
		shapes.push_back(Shape(2, Box::model({2.5f, -0.2f, -3.0f}, {2, 2, 2})));
	} else {
		materials.add(Material()); // the app's start-up state (main.cpp:100)
	}

	std::vector<std::pair<std::string, int>> mtl_index; // --obj-materials: (MTL material name, its index in `materials`)
	int slot = 0;
	auto add_model = [&](const std::optional<ModelPair> &pair, const std::string &path) {
		if (!pair) {
			std::cerr << "Inexistant file: " << path << "\n";
			std::exit(3);
		}
		Model m(triangles, pair->first, pair->second);
		// place successive models side by side, like dragging them apart in the GUI
		m.transform = glm::translate(glm::vec3(-1.3f + 2.7f * (float)slot, 0.1f, -1.0f - 0.6f * (float)slot)) *
		              glm::eulerAngleYXZ(0.6f - 1.5f * (float)slot, 0.2f, 0.0f);
		m.compute_bounding_box(triangles);
		shapes.push_back(Shape(materials.size() > 1 ? 1 + slot % (materials.size() - 1) : 0, m));
		slot++;
		std::cout << path << ": " << pair->second << " triangles at " << pair->first << "\n";
	};
	std::vector<float> uvs(triangles.size() * 6, 0.0f); // parallel to `triangles`: the box's and STL triangles have none
	// --obj-materials: the `usemtl` name of every triangle (an index into usemtl_names, -1: none), the OBJs' MTL materials
	// appended to the scene's, and the table Tracer::set_triangle_materials takes
	std::vector<int32_t> face_names(triangles.size(), -1), triangle_materials;
	std::vector<std::string> usemtl_names;
	std::vector<std::pair<int, std::string>> material_maps; // (material, its map_Kd file)
	for (auto &p : objs) {
		if (!obj_materials) {
			add_model(load_obj_model(p, triangles, &uvs), p);
			continue;
		}
		std::vector<std::string> mtllibs;
		add_model(load_obj_model(p, triangles, &uvs, &face_names, &usemtl_names, &mtllibs), p);
		for (auto &lib : mtllibs) {
			std::vector<std::string> maps;
			const fs::path lib_path = fs::path(p).parent_path() / lib;
			const auto loaded = load_mtl(lib_path, &maps);
			if (loaded.empty()) std::cerr << lib_path.string() << ": no materials read\n";
			for (size_t i = 0; i < loaded.size(); i++) {
				const int index = materials.add(loaded[i].second);
				mtl_index.emplace_back(loaded[i].first, index);
				if (!maps[i].empty()) material_maps.emplace_back(index, (lib_path.parent_path() / maps[i]).string());
			}
		}
	}
	for (auto &p : stls) add_model(load_stl_model(p, triangles), p);
	uvs.resize(triangles.size() * 6, 0.0f);
	if (obj_materials) {
		face_names.resize(triangles.size(), -1);
		std::vector<int32_t> of_name(usemtl_names.size(), -1); // a name no MTL file defines keeps the shape's material
		for (size_t n = 0; n < usemtl_names.size(); n++)
			for (auto &entry : mtl_index)
				if (entry.first == usemtl_names[n]) {
					of_name[n] = entry.second; // (the first definition of a name counts)
					break;
				}
		size_t with = 0;
		for (int32_t f : face_names) {
			triangle_materials.push_back(f < 0 ? -1 : of_name[(size_t)f]);
			with += triangle_materials.back() >= 0;
		}
		std::cout << "per-triangle materials: " << triangle_materials.size() << " triangles, " << with << " with a material of their own, " << usemtl_names.size()
		          << " usemtl names:";
		for (size_t n = 0; n < usemtl_names.size(); n++) std::cout << ' ' << usemtl_names[n] << '=' << of_name[n];
		std::cout << "\n";
	}

	const glm::mat4 camera_to_world = eye_matrix(glm::vec3(0.0f, 0.5f, 5.0f), 0.0f, 0.0f);

	if (!dump_prefix.empty()) {
		dump(dump_prefix + ".shapes.bin", shapes.data(), shapes.size());
		dump(dump_prefix + ".tris.bin", triangles.data(), triangles.size());
		dump(dump_prefix + ".mats.bin", materials.list.data(), materials.list.size());
		if (obj_materials) dump(dump_prefix + ".tm.bin", triangle_materials.data(), triangle_materials.size());
	}
	if (parse_only) return 0;

	// ---- tracer set-up, as src/main.cpp:114-126 ----
	Tracer tracer(width, height, 0, gpus); // --gpus N: one Tracer over N devices (rows split, one RCCL gather per frame)
	if (bvh) tracer.set_acceleration(SRT_ACCEL_BVH);
	tracer.set_acceleration_build_order(bvh_order); // (of --bvh-build device; else no effect)
	if (bvh_build_device) tracer.set_acceleration_build(SRT_BUILD_DEVICE, bvh_build_min); // (models of at least MIN triangles; without --bvh: no effect)
	if (exposure) tracer.set_exposure(exposure_auto, exposure_ev);
	if (bloom) tracer.set_bloom(bloom_threshold, bloom_intensity, bloom_levels);
	if (!selected.empty()) tracer.set_selection(selected, select_width, select_colour);
	if (denoise >= 0) tracer.set_denoise(denoise);
	if (demodulate) tracer.set_denoise_demodulation();
	if (spatial_variance > 0) tracer.set_denoise_spatial_variance((uint32_t)spatial_variance);
	if (temporal) tracer.set_denoise_temporal();
	if (history_illumination) tracer.set_denoise_history_illumination();
	if (clamp_given) tracer.set_denoise_history_clamp(history_clamp);
	if (history_feedback) tracer.set_denoise_history_feedback();
	if (until_noise || !noise_view.empty()) tracer.set_noise_meter(noise_threshold, noise_permille);
	if (move_shape >= 0) {
		if (!temporal || (size_t)move_shape >= shapes.size()) {
			std::cerr << "--move-shape needs --temporal and a shape index below " << shapes.size() << "\n";
			return 2;
		}
		tracer.set_denoise_object_motion();
	}
	tracer.options.num_samples = spp;
	tracer.options.num_bounces = bounces;
	tracer.options.show_normals = false;
	tracer.scene_data.horizon_color = color::from_hex(0x374F62);
	tracer.scene_data.zenith_color = color::from_hex(0x11334A);
	tracer.scene_data.ground_color = color::from_hex(0x777777);
	tracer.scene_data.sun_focus = 25.0f;
	tracer.scene_data.sun_color = color::from_hex(0xffffd3);
	tracer.scene_data.sun_intensity = 1.0f;
	tracer.scene_data.sun_direction = VEC3TOCL(glm::normalize(glm::vec3(1.0f, -1.0f, 0.0f)));
	int sky_w = 2048, sky_h = 1024;
	std::vector<float> sky;
	if (!skybox_path.empty()) {
		std::vector<uint8_t> rgb;
		if (!load_ppm(skybox_path, rgb, sky_w, sky_h)) {
			std::cerr << "cannot read " << skybox_path << " (binary PPM, P6, maxval 255)\n";
			return 3;
		}
		sky.resize((size_t)sky_w * sky_h * 4);
		srt_skybox_from_rgb8(rgb.data(), sky_w, sky_h, 3, sky.data()); // as stbi_loadf + flip (src/tracer.cpp:42-46)
	} else {
		sky = synthetic_sky(sky_w, sky_h);
	}
	tracer.set_skybox(sky.data(), sky_w, sky_h);
	std::vector<Tracer::Texture> textures;
	std::vector<Tracer::MaterialTexture> bindings(materials.list.size(), Tracer::MaterialTexture{-1, SRT_FILTER_LINEAR, 1.0f, 1.0f});
	auto load_texture = [&](const std::string &path, Tracer::Texture &tex) {
		std::vector<uint8_t> rgb;
		if (!load_ppm(path, rgb, tex.width, tex.height)) return false;
		tex.rgba.resize((size_t)tex.width * tex.height * 4);
		srt_skybox_from_rgb8(rgb.data(), tex.width, tex.height, 3, tex.rgba.data());
		return true;
	};
	if (!texture_path.empty()) {
		Tracer::Texture tex;
		if (!load_texture(texture_path, tex)) {
			std::cerr << "cannot read " << texture_path << " (binary PPM, P6, maxval 255)\n";
			return 3;
		}
		if (texture_material < 0 || (size_t)texture_material >= materials.list.size()) {
			std::cerr << "--texture needs --texture-material N with N below " << materials.list.size() << "\n";
			return 2;
		}
		bindings[(size_t)texture_material] = Tracer::MaterialTexture{0, texture_nearest ? SRT_FILTER_NEAREST : SRT_FILTER_LINEAR, texture_scale, texture_scale};
		textures.push_back(tex);
	}
	for (auto &map : material_maps) { // --obj-materials: the MTL files' map_Kd, where the tool reads that kind of file
		Tracer::Texture tex;
		if (textures.size() >= SRT_MAX_TEXTURES || !load_texture(map.second, tex)) {
			std::cerr << "map_Kd " << map.second << " of material " << map.first << ": not a binary PPM the tool reads (or too many images), skipped\n";
			continue;
		}
		bindings[(size_t)map.first] = Tracer::MaterialTexture{(int32_t)textures.size(), SRT_FILTER_LINEAR, 1.0f, 1.0f};
		textures.push_back(tex);
	}
	if (!textures.empty()) {
		tracer.set_textures(textures);
		tracer.set_material_textures(bindings);
		if (!objs.empty()) tracer.set_triangle_uvs(uvs);
		if (!dump_prefix.empty()) {
			dump(dump_prefix + ".texture.bin", textures[0].rgba.data(), textures[0].rgba.size());
			dump(dump_prefix + ".uvs.bin", uvs.data(), uvs.size());
		}
	}
	if (obj_materials) tracer.set_triangle_materials(triangle_materials);
	if (!dump_prefix.empty()) dump(dump_prefix + ".sky.bin", sky.data(), sky.size());

	std::vector<uint8_t> pixels((size_t)width * height * 4);

	if ((!lasso.empty() || area_through) && !select_area) {
		std::cerr << "--lasso and --through need --select-area\n";
		return 2;
	}
	if (select_area) { // --select-area: the shapes visible inside the area through the first frame's camera, combined with --select's
		tracer.update_scene(shapes, triangles, materials.list);
		auto &options = tracer.options;
		options.aspect_ratio = (float)width / (float)height;
		options.fov_scale = 1.0f;
		options.camera_to_world = moving ? eye_matrix(glm::vec3(0.0f, 0.5f, 5.0f), 0.0f, 0.0f) : camera_to_world;
		srt_area_summary sum;
		const std::vector<uint32_t> counts = tracer.area_coverage(area, lasso, &sum, area_through);
		std::printf("area: %u pixel(s), %u on shapes, %u miss, %u shape(s)\n", sum.area_pixels, sum.hit_pixels, sum.miss_pixels, sum.distinct);
		for (size_t i = 0; i < counts.size(); i++)
			if (counts[i]) std::printf("shape %zu count %u\n", i, counts[i]);
		const size_t n = tracer.select_area(area, lasso, area_mode, area_min_pixels, area_through);
		selected = tracer.read_selection();
		std::printf("area selection: %zu shape(s)\n", n);
	}

	if (!picks.empty() || !through.empty()) { // --pick, --pick-through: what is under these image points, through the first frame's camera
		tracer.update_scene(shapes, triangles, materials.list);
		auto &options = tracer.options;
		options.aspect_ratio = (float)width / (float)height;
		options.fov_scale = 1.0f;
		options.camera_to_world = moving ? eye_matrix(glm::vec3(0.0f, 0.5f, 5.0f), 0.0f, 0.0f) : camera_to_world;
		// the picked point's ray once more on the host, for the printed position (the library's own is made on the device)
		auto ray_of = [&](float x, float y) {
			const float sx = (2.0f * (x / (float)width) - 1.0f) * options.aspect_ratio * options.fov_scale;
			const float sy = (1.0f - 2.0f * (y / (float)height)) * options.fov_scale;
			const glm::vec4 v = options.camera_to_world * glm::vec4(sx, sy, -1.0f, 0.0f);
			const glm::vec3 d = glm::normalize(glm::vec3(v.x, v.y, v.z));
			const glm::vec4 o = options.camera_to_world[3];
			srt_ray r{{o.x, o.y, o.z}, INFINITY, {d.x, d.y, d.z}, 0u};
			return r;
		};
		auto print_hit = [&](const char *what, float x, float y, const srt_ray_hit &h) {
			const srt_ray r = ray_of(x, y);
			std::printf("%s %g,%g: shape %u triangle %d material %d t %.9g position %.9g %.9g %.9g normal %.9g %.9g %.9g\n", what, x, y, h.shape,
			            h.triangle == SRT_HIT_NONE ? -1 : (int)h.triangle, h.material, h.t, r.origin[0] + r.direction[0] * h.t,
			            r.origin[1] + r.direction[1] * h.t, r.origin[2] + r.direction[2] * h.t, h.normal[0], h.normal[1], h.normal[2]);
		};
		const std::vector<srt_ray_hit> hits = picks.empty() ? std::vector<srt_ray_hit>() : tracer.pick(picks);
		for (size_t k = 0; k < hits.size(); k++) {
			if (!(hits[k].flags & SRT_HIT_HIT)) {
				std::printf("pick %g,%g: miss\n", picks[2 * k], picks[2 * k + 1]);
				continue;
			}
			print_hit("pick", picks[2 * k], picks[2 * k + 1], hits[k]);
		}
		for (size_t q = 0; q < through_k.size(); q++) { // one record per line, nearest first, then how many there were
			const float x = through[2 * q], y = through[2 * q + 1];
			std::vector<uint32_t> counts;
			const std::vector<srt_ray_hit> recs = tracer.pick_through(std::vector<float>{x, y}, through_k[q], &counts);
			for (uint32_t j = 0; j < counts[0]; j++) print_hit("pick-through", x, y, recs[j]);
			std::printf("pick-through %g,%g: %u hit(s)\n", x, y, counts[0]);
		}
	}

	if (!nearests.empty()) { // --nearest: the closest surface to these points, answered without rendering
		tracer.update_scene(shapes, triangles, materials.list);
		static const char *const features[7] = {"face", "vertex0", "vertex1", "vertex2", "edge01", "edge02", "edge12"};
		for (size_t k = 0; k < nearests.size(); k++) {
			const srt_point_query &pq = nearests[k];
			const srt_nearest r = tracer.nearest(std::vector<srt_point_query>{pq}, nearest_skips[k])[0];
			if (!(r.flags & SRT_NEAREST_FOUND)) {
				std::printf("nearest %g,%g,%g: %s\n", pq.point[0], pq.point[1], pq.point[2], (r.flags & SRT_NEAREST_INVALID) ? "invalid" : "nothing");
				continue;
			}
			std::printf("nearest %g,%g,%g: shape %u triangle %d material %d distance %.9g point %.9g %.9g %.9g %s %s\n", pq.point[0], pq.point[1], pq.point[2],
			            r.shape, r.triangle == SRT_HIT_NONE ? -1 : (int)r.triangle, r.material, r.distance, r.point[0], r.point[1], r.point[2],
			            features[(r.flags & SRT_NEAREST_FEATURE_MASK) >> SRT_NEAREST_FEATURE_SHIFT], (r.flags & SRT_NEAREST_BACK) ? "back" : "front");
		}
	}

	if (!sights.empty()) { // --line-of-sight: a yes/no question each, answered without rendering
		tracer.update_scene(shapes, triangles, materials.list);
		std::vector<bool> invalid;
		const std::vector<bool> occluded = tracer.occluded(sights, &invalid);
		for (size_t k = 0; k < sights.size(); k++) {
			const srt_segment &sg = sights[k];
			std::printf("line of sight %g,%g,%g:%g,%g,%g:%g: %s\n", sg.from[0], sg.from[1], sg.from[2], sg.to[0], sg.to[1], sg.to[2], sg.end_gap,
			            invalid[k] ? "invalid" : occluded[k] ? "occluded" : "visible");
		}
	}

	// ---- frame loop, as src/main.cpp:277-290,337 ----
	unsigned time_not_moved = 1;
	auto t0 = std::chrono::steady_clock::now();
	srt_noise_result noise{};
	uint32_t noise_dispatches = 0;
	if (until_noise) { // one still frame, accumulated until the meter says so
		frames = 0;
		tracer.clear_canvas();
		tracer.update_scene(shapes, triangles, materials.list);
		auto &options = tracer.options;
		options.aspect_ratio = (float)width / (float)height;
		options.fov_scale = 1.0f;
		options.camera_to_world = camera_to_world;
		options.time = time_seed;
		options.tick = 0;
		noise_dispatches = tracer.render_until((uint32_t)noise_max, pixels, noise, 7919u);
	}
	for (int frame = 0; frame < frames; frame++) {
		if (time_not_moved == 1) {
			tracer.clear_canvas();
			if (move_shape >= 0 && frame > 0) { // the dragged shape, as the front-end's gizmo edits the record
				Shape &s = shapes[(size_t)move_shape];
				if (s.type == SHAPE_SPHERE) s.shape.sphere.position.x += shape_move;
				else if (s.type == SHAPE_PLANE) s.shape.plane.position.x += shape_move;
				else {
					s.shape.model.transform[3].x += shape_move;
					s.shape.model.compute_bounding_box(triangles);
				}
			}
			tracer.update_scene(shapes, triangles, materials.list);
		}
		auto &options = tracer.options;
		options.aspect_ratio = (float)width / (float)height;
		options.fov_scale = 1.0f; // tan(90deg / 2)
		options.camera_to_world = moving ? eye_matrix(glm::vec3(move * (float)frame, 0.5f, 5.0f), 0.0f, 0.0f) : camera_to_world;
		options.time = time_seed + 7919u * (unsigned)frame;
		options.tick = (unsigned)frame;
		if (pipelined) tracer.render_pipelined(time_not_moved, pixels); // delivers the previous frame
		else tracer.render(time_not_moved, pixels);
		time_not_moved = (moving || move_shape >= 0) ? 1 : time_not_moved + 1; // a moving camera clears every frame (src/main.cpp:270-290)
	}
	if (pipelined) tracer.finish(pixels);
	double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	srt_counters c = tracer.counters();
	std::printf("%d frame(s) %dx%d x %d spp: %.3f s, %.1f Mray/s, %llu NaN pixels\n", frames, width, height, spp, secs,
	            (double)c.rays / secs / 1e6, (unsigned long long)c.nan_pixels);
	if (exposure) {
		float log2_exposure = 0.0f;
		const float e = tracer.read_exposure(&log2_exposure);
		std::printf("exposure %s: %.6g (2^%.4f)%s\n", exposure_auto ? "auto" : "manual", e, log2_exposure, tracer.last_resolve_exposed() ? "" : " -- NOT applied");
	}
	if (bloom) {
		int w0 = 0, h0 = 0;
		const bool ran = tracer.last_resolve_bloomed();
		if (ran) tracer.read_bloom(0, nullptr, &w0, &h0);
		std::printf("bloom: level 0 is %dx%d%s\n", w0, h0, ran ? "" : " -- NOT applied");
	}
	if (!selected.empty()) std::printf("selection: %zu shape(s)%s\n", selected.size(), tracer.last_resolve_selected() ? "" : " -- NOT applied");

	if (until_noise)
		std::printf("until-noise: %s after %u dispatches; deciding check at T = %u, P = %u: level %.6g (bin %d), %u of %u pixels below, %u left out\n",
		            noise.converged ? "converged" : "NOT converged", noise_dispatches, noise.dispatches, noise.samples, (double)noise.level, noise.level_bin, noise.below,
		            noise.metered, noise.left_out);

	if (!out.empty()) save_ppm(out, pixels, width, height);
	if (!noise_view.empty()) { // (after the picture: the heat map overwrites the handle's image)
		std::vector<uint8_t> heat;
		tracer.resolve_noise_view(heat);
		save_ppm(noise_view, heat, width, height);
		const srt_noise_result r = tracer.read_noise();
		std::printf("noise-view: T = %u, P = %u: level %.6g (bin %d), %u of %u pixels below, %u left out\n", r.dispatches, r.samples, (double)r.level, r.level_bin, r.below,
		            r.metered, r.left_out);
	}
	if (ao_samples > 0) { // (after the picture, as the noise view: the grey picture overwrites the handle's image)
		tracer.render_ao(ao_samples, ao_radius, ao_bias);
		std::vector<uint32_t> occluded;
		const int s = tracer.read_ao(occluded);
		size_t surfaces = 0;
		double sum = 0.0;
		for (uint32_t c : occluded)
			if (c != SRT_HIT_NONE) surfaces++, sum += (double)c / (double)s;
		std::printf("ao: pixels %zu surfaces %zu mean %.6f\n", occluded.size(), surfaces, surfaces ? sum / (double)surfaces : 0.0);
		if (!ao_view.empty()) {
			std::vector<uint8_t> grey;
			tracer.resolve_ao_view(grey);
			save_ppm(ao_view, grey, width, height);
		}
	}
	if (!dump_prefix.empty()) {
		std::vector<float> canvas;
		tracer.read_canvas(canvas);
		dump(dump_prefix + ".canvas.bin", canvas.data(), canvas.size());
		dump(dump_prefix + ".argb.bin", pixels.data(), pixels.size());
		dump(dump_prefix + ".rd.bin", &tracer.options, 1);
		dump(dump_prefix + ".sd.bin", &tracer.scene_data, 1);
	}
	return 0;
}
