// tracer.hpp — `class Tracer` with the reference's public interface
// (/root/reference/include/tracer.hpp:26-88), implemented over the C ABI of
// libsrt_hip.so instead of boost.compute/OpenCL. The front-end's call sequence
// (src/main.cpp:114-126, 277-290) works unchanged:
//
//     Tracer tracer(w, h);  tracer.options.num_samples = 2; tracer.scene_data.sun_focus = ...
//     tracer.clear_canvas(); tracer.update_scene(shapes, triangles, materials.materials);
//     tracer.options.camera_to_world = camera_mat; ...; tracer.render(ticks, pixels);
//
// Differences a maintainer must know: no run-time files are read
// (render.cl is gone; the skybox is handed over decoded via set_skybox), and failures
// throw std::runtime_error carrying srt_last_error() where boost.compute threw.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/srt_abi.h"
#include "color.hpp"
#include "material.hpp"
#include "shape.hpp"

#define VEC3TOCL(v) (cl_float3({{(v).x, (v).y, (v).z}}))
#define VEC4TOCL(v) (cl_float4({{(v).x, (v).y, (v).z, (v).w}}))

class Tracer {
  private:
	srt_tracer *handle = nullptr; // one device ...
	srt_group *group = nullptr;   // ... or a group of devices (n_devices > 1): rows dealt in interleaved blocks, one RCCL gather per frame

	void check(int rc) const {
		if (rc != SRT_OK) throw std::runtime_error(std::string("srt: ") + (group ? srt_group_last_error(group) : srt_last_error(handle)));
	}

  public:
	struct RenderData {
		cl_int width, height;
		cl_int num_samples;
		cl_int num_bounces;
		cl_float aspect_ratio;
		cl_float fov_scale;
		bool show_normals;

		alignas(cl_float4) glm::mat4 camera_to_world;

		cl_uint time;
		cl_uint tick;

		RenderData(int width, int height)
			: width(width), height(height), num_samples(4), num_bounces(10), aspect_ratio(float(width) / float(height)),
			  fov_scale(1.0f), show_normals(false), camera_to_world(1.0f), time(1), tick(0) {}
	} options;

	struct SceneData {
		cl_int num_shapes;
		cl_float sun_focus;
		cl_float sun_intensity;

		alignas(cl_float3) Color horizon_color;
		alignas(cl_float3) Color zenith_color;
		alignas(cl_float3) Color ground_color;
		alignas(cl_float3) Color sun_color;

		cl_float3 sun_direction;
	} scene_data;

	/// n_devices == 1: the reference's single-device Tracer on HIP device `device`. n_devices > 1 (new): the same
	/// interface over devices 0 .. n_devices-1 of this node; every call below fans out, render() collects the
	/// frame with ONE ncclGather on device 0 and returns the same bytes a single device would.
	Tracer(const int width, const int height, const int device = 0, const int n_devices = 1) : options(width, height), scene_data() {
		int rc = n_devices > 1 ? srt_group_create(width, height, n_devices, nullptr, 8, &group) : srt_create(width, height, device, &handle);
		if (rc != SRT_OK) throw std::runtime_error(std::string("srt_create: ") + srt_last_error(nullptr));
	}
	~Tracer() {
		srt_group_destroy(group);
		srt_destroy(handle);
	}
	Tracer(const Tracer &) = delete;
	Tracer &operator=(const Tracer &) = delete;

	/// replaces the stbi_loadf + enqueue_write_image of the reference's constructor:
	/// `rgba` = width*height RGBA32F texels, row 0 = bottom of the picture
	void set_skybox(const float *rgba, int width, int height) {
		check(group ? srt_group_set_skybox(group, rgba, width, height) : srt_set_skybox(handle, rgba, width, height));
	}

	void update_scene(
		const std::vector<Shape> &shapes, const std::vector<Triangle> &triangles, const std::vector<Material> &materials
	) {
		static_assert(sizeof(SceneData) == sizeof(srt_scene_data), "SceneData layout");
		const srt_shape *sh = reinterpret_cast<const srt_shape *>(shapes.data());
		const srt_triangle *tr = reinterpret_cast<const srt_triangle *>(triangles.data());
		const srt_material *ma = reinterpret_cast<const srt_material *>(materials.data());
		const srt_scene_data *sd = reinterpret_cast<const srt_scene_data *>(&scene_data);
		check(group ? srt_group_update_scene(group, sh, shapes.size(), tr, triangles.size(), ma, materials.size(), sd)
		            : srt_update_scene(handle, sh, shapes.size(), tr, triangles.size(), ma, materials.size(), sd));
		scene_data.num_shapes = (cl_int)shapes.size();
	}

	void clear_canvas() { check(group ? srt_group_clear_canvas(group) : srt_clear_canvas(handle)); }

	/// trace + resolve + blocking read-back of width*height*4 bytes (A,R,G,B)
	void render(cl_uint ticks_stopped, std::vector<uint8_t> &output) {
		static_assert(sizeof(RenderData) == sizeof(srt_render_data), "RenderData layout");
		if (output.size() < size_t(options.width) * size_t(options.height) * 4)
			throw std::runtime_error("Tracer::render: output must hold width*height*4 bytes");
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		check(group ? srt_group_render(group, rd, ticks_stopped, output.data()) : srt_render(handle, rd, ticks_stopped, output.data()));
	}

	/// render() for a loop that can show a frame one call late (src/main.cpp:277-337 blits `output` right after the
	/// call): enqueues this frame and fills `output` with the PREVIOUS one, so frame N's read-back runs under frame
	/// N+1's trace. Returns the index of the frame delivered, -1 on the first call (output untouched); finish()
	/// hands out the last one. Same bytes as render(), one call later. Single device only.
	long long render_pipelined(cl_uint ticks_stopped, std::vector<uint8_t> &output) {
		if (group) throw std::runtime_error("Tracer::render_pipelined: single-device tracers only");
		if (output.size() < size_t(options.width) * size_t(options.height) * 4)
			throw std::runtime_error("Tracer::render_pipelined: output must hold width*height*4 bytes");
		long long delivered = -1;
		check(srt_render_pipelined(handle, reinterpret_cast<const srt_render_data *>(&options), ticks_stopped, output.data(), &delivered));
		return delivered;
	}
	long long finish(std::vector<uint8_t> &output) {
		long long delivered = -1;
		if (!group) check(srt_pipeline_flush(handle, output.data(), &delivered));
		return delivered;
	}

	// -- extras beyond the reference's interface --
	/// Albedo textures (include/srt_abi.h "albedo textures"; the reference's "texture support" plan). A texture is
	/// width * height RGBA32F texels, row 0 = bottom (host/skybox.hpp prepares 8-bit images); `bindings` holds one
	/// MaterialTexture per material, in the order of MaterialHelper::materials; `uvs` 6 floats per triangle as
	/// load_obj_model hands them out. None of the three clears the canvas.
	struct Texture {
		std::vector<float> rgba;
		int width = 0, height = 0;
	};
	using MaterialTexture = srt_material_texture; // {texture (-1: none), filter (SRT_FILTER_*), scale_u, scale_v}
	void set_textures(const std::vector<Texture> &textures) {
		std::vector<srt_texture_desc> d(textures.size());
		for (size_t i = 0; i < textures.size(); i++) d[i] = srt_texture_desc{textures[i].rgba.data(), textures[i].width, textures[i].height};
		check(group ? srt_group_set_textures(group, d.data(), d.size()) : srt_set_textures(handle, d.data(), d.size()));
	}
	void set_material_textures(const std::vector<MaterialTexture> &bindings) {
		check(group ? srt_group_set_material_textures(group, bindings.data(), bindings.size())
		            : srt_set_material_textures(handle, bindings.data(), bindings.size()));
	}
	void set_triangle_uvs(const std::vector<float> &uvs) {
		const float *p = uvs.empty() ? nullptr : uvs.data();
		check(group ? srt_group_set_triangle_uvs(group, p, uvs.size() / 6) : srt_set_triangle_uvs(handle, p, uvs.size() / 6));
	}

	/// Per-triangle materials (include/srt_abi.h "per-triangle materials"): one index into the material array per triangle,
	/// parallel to `triangles` as load_obj_model hands them out for an OBJ's `usemtl` groups; -1 keeps the shape's material.
	/// An empty vector removes the table. Does not clear the canvas.
	void set_triangle_materials(const std::vector<int32_t> &materials) {
		const int32_t *p = materials.empty() ? nullptr : materials.data();
		check(group ? srt_group_set_triangle_materials(group, p, materials.size()) : srt_set_triangle_materials(handle, p, materials.size()));
	}

	/// SRT_ACCEL_BVH: models get a bounding-volume hierarchy at the next update_scene (the
	/// reference's README.md:41 "future plan"); SRT_ACCEL_NONE (default) keeps the array-order scan
	void set_acceleration(int mode) { check(group ? srt_group_set_acceleration(group, mode) : srt_set_acceleration(handle, mode)); }
	// SRT_REFIT_HOST / SRT_REFIT_DEVICE: who refits the hierarchy of a model that only moved (the next update_scene on)
	void set_acceleration_refit(int mode) { check(group ? srt_group_set_acceleration_refit(group, mode) : srt_set_acceleration_refit(handle, mode)); }
	// SRT_DEFORM_REBUILD / SRT_DEFORM_REFIT: a model whose vertices changed is built anew / keeps its tree with new boxes, until
	// its cost ratio passes rebuild_ratio (0 = never; the next update_scene on)
	void set_acceleration_deform(int mode, float rebuild_ratio = 0.0f) {
		check(group ? srt_group_set_acceleration_deform(group, mode, rebuild_ratio) : srt_set_acceleration_deform(handle, mode, rebuild_ratio));
	}
	// SRT_BUILD_HOST / SRT_BUILD_DEVICE: a model of at least min_triangles triangles without a hierarchy to keep is built by the
	// host's SAH / gets the balanced topology over its Morton order, sorted on the device
	void set_acceleration_build(int mode, uint32_t min_triangles = 0) {
		check(group ? srt_group_set_acceleration_build(group, mode, min_triangles) : srt_set_acceleration_build(handle, mode, min_triangles));
	}
	// SRT_BUILD_ORDER_MORTON / SRT_BUILD_ORDER_MEDIAN: the order SRT_BUILD_DEVICE lays the balanced topology over (the next
	// update_scene on; without effect under SRT_BUILD_HOST)
	void set_acceleration_build_order(int order) {
		check(group ? srt_group_set_acceleration_build_order(group, order) : srt_set_acceleration_build_order(handle, order));
	}
	// {models built on the device by the last update, records sorted, build launches, 0} (a group: its first member's)
	void acceleration_build_info(uint64_t out[4]) { check(srt_acceleration_build_info(group ? srt_group_tracer(group, 0) : handle, out)); }
	/// The edge-aware denoiser (srt_set_denoise): iterations < 0 turns it off, else it is on with srt_denoise_defaults()
	/// overridden by the arguments; render() / render_pipelined() then hand out the filtered image. On a Tracer over several
	/// devices the members gather the filter's inputs with the frame and device 0 filters (srt_group_set_denoise): the same bytes.
	void set_denoise(int iterations = 5, int feature_samples = 1, float sigma_luminance = 4.0f, float sigma_normal = 128.0f,
	                 float sigma_depth = 1.0f, float sigma_albedo = 0.1f) {
		if (iterations < 0) {
			check(group ? srt_group_set_denoise(group, nullptr) : srt_set_denoise(handle, nullptr));
			return;
		}
		srt_denoise_params d;
		check(srt_denoise_defaults(&d));
		d.iterations = iterations;
		d.feature_samples = feature_samples;
		d.sigma_luminance = sigma_luminance;
		d.sigma_normal = sigma_normal;
		d.sigma_depth = sigma_depth;
		d.sigma_albedo = sigma_albedo;
		check(group ? srt_group_set_denoise(group, &d) : srt_set_denoise(handle, &d));
	}
	/// The denoiser's temporal reprojection (srt_set_denoise_temporal): the frame before each clear_canvas is reprojected
	/// into the next camera and blended in. Needs set_denoise first; enable = false turns it off. Several devices: the history lives on device 0.
	void set_denoise_temporal(bool enable = true, int history_limit = 32, float normal_threshold = 0.9f, float depth_threshold = 0.05f) {
		if (!enable) {
			check(group ? srt_group_set_denoise_temporal(group, nullptr) : srt_set_denoise_temporal(handle, nullptr));
			return;
		}
		srt_temporal_params p;
		check(srt_temporal_defaults(&p));
		p.history_limit = history_limit;
		p.normal_threshold = normal_threshold;
		p.depth_threshold = depth_threshold;
		check(group ? srt_group_set_denoise_temporal(group, &p) : srt_set_denoise_temporal(handle, &p));
	}
	/// Albedo demodulation (srt_set_denoise_demodulation): the a-trous passes filter colour / first-hit albedo and the last one
	/// multiplies the albedo back, which keeps fine textures and still averages their noise. Needs set_denoise first; one
	/// device or a device group (the group's filter runs on device 0).
	void set_denoise_demodulation(bool enable = true) {
		check(group ? srt_group_set_denoise_demodulation(group, enable ? 1 : 0) : srt_set_denoise_demodulation(handle, enable ? 1 : 0));
	}
	/// The history reprojected as illumination (srt_set_denoise_history_illumination): a history tap is rescaled from its own
	/// first-hit albedo to the pixel's, so a moving camera no longer blurs a texture through the history. Needs
	/// set_denoise_temporal first; one device or a device group (the group's set-up runs on device 0).
	void set_denoise_history_illumination(bool enable = true) {
		check(group ? srt_group_set_denoise_history_illumination(group, enable ? 1 : 0) : srt_set_denoise_history_illumination(handle, enable ? 1 : 0));
	}
	/// Whether the last temporal set-up (a filter's or a clear's) launched an illumination kernel
	bool last_setup_history_illumination() {
		return (group ? srt_group_last_setup_history_illumination(group) : srt_last_setup_history_illumination(handle)) != 0;
	}
	/// The history clamp (srt_set_denoise_history_clamp): the reprojected history colour of a pixel is pulled into mean +- gamma
	/// sigma of the current frame's 7x7 neighbourhood before it is blended in, so lighting a moved shape left behind (its shadow,
	/// its reflection) is corrected within a frame or two. 0 turns it off. Needs set_denoise_temporal first; one device or a
	/// device group (the group's set-up runs on device 0).
	void set_denoise_history_clamp(float gamma = 1.0f) {
		check(group ? srt_group_set_denoise_history_clamp(group, gamma) : srt_set_denoise_history_clamp(handle, gamma));
	}
	/// Whether the last temporal set-up (a filter's or a clear's) ran the bounds launch and a clamping set-up
	bool last_setup_history_clamp() {
		return (group ? srt_group_last_setup_history_clamp(group) : srt_last_setup_history_clamp(handle)) != 0;
	}
	/// The history feedback (srt_set_denoise_history_feedback): with iterations >= 1 the colour that enters the temporal history
	/// is the first a-trous pass's output instead of the integrated samples, SVGF's feedback. Needs set_denoise_temporal first;
	/// one device or a device group (the group's filter and commit run on device 0).
	void set_denoise_history_feedback(bool enable = true) {
		check(group ? srt_group_set_denoise_history_feedback(group, enable ? 1 : 0) : srt_set_denoise_history_feedback(handle, enable ? 1 : 0));
	}
	/// Whether the last pass 1 (a filter's or a clear's) was a feedback instantiation
	bool last_filter_history_feedback() {
		return (group ? srt_group_last_filter_history_feedback(group) : srt_last_filter_history_feedback(handle)) != 0;
	}
	/// Spatial variance estimate (srt_set_denoise_spatial_variance): a pixel with fewer than min_samples samples (the first
	/// frames after a clear, disocclusions under temporal reprojection) takes its variance from the moments of its 7x7
	/// neighbourhood instead of its own two or three samples. 0 turns it off. Needs set_denoise first; one device or a group.
	void set_denoise_spatial_variance(uint32_t min_samples = 8) {
		check(group ? srt_group_set_denoise_spatial_variance(group, min_samples) : srt_set_denoise_spatial_variance(handle, min_samples));
	}
	/// Whether the last filter enqueued that estimate (the switch on and iterations >= 1)
	bool last_filter_spatial_variance() {
		int ran = 0;
		check(group ? srt_group_last_filter_spatial_variance(group, &ran) : srt_last_filter_spatial_variance(handle, &ran));
		return ran != 0;
	}
	/// Exposure for the resolve (srt_set_exposure): every frame's bytes are tonemap(colour * exposure). automatic: the exposure is
	/// metered on the device from the frame's luminance histogram and ev is a bias on it; else it is 2^ev. adapt in (0, 1]: how
	/// much of the way to a new metered value one frame goes, in log2 (1: at once). One device or a group (the group's state
	/// lives on device 0). Never waits for the device.
	void set_exposure(bool automatic = true, float ev = 0.0f, float adapt = 1.0f) {
		srt_exposure_params p;
		check(srt_exposure_defaults(&p));
		p.mode = automatic ? SRT_EXPOSURE_AUTO : SRT_EXPOSURE_MANUAL;
		p.ev = ev;
		p.adapt = adapt;
		check(group ? srt_group_set_exposure(group, &p) : srt_set_exposure(handle, &p));
	}
	/// ... off: the plain resolve alone, and the adaptation starts anew when it is turned on again
	void clear_exposure() { check(group ? srt_group_set_exposure(group, nullptr) : srt_set_exposure(handle, nullptr)); }
	/// Forget the adaptation state: the next metered frame adopts its target (a cut to another scene)
	void reset_exposure() { check(group ? srt_group_reset_exposure(group) : srt_reset_exposure(handle)); }
	/// The exposure of the last exposed frame and its log2 (waits for the device; for a readout, not for the frame loop)
	float read_exposure(float *log2_exposure = nullptr) {
		float e = 1.0f;
		check(group ? srt_group_read_exposure(group, log2_exposure, &e, nullptr, nullptr) : srt_read_exposure(handle, log2_exposure, &e, nullptr, nullptr));
		return e;
	}
	/// Whether the last frame's bytes went through the exposed resolve
	bool last_resolve_exposed() {
		int exposed = 0;
		check(group ? srt_group_last_resolve_exposed(group, &exposed) : srt_last_resolve_exposed(handle, &exposed));
		return exposed != 0;
	}
	/// Bloom for the resolve (srt_set_bloom): what of the exposed colour lies above `threshold` is blurred over `levels` pyramid
	/// levels on the device and added with weight `intensity` before the tone map. A negative threshold or intensity, or
	/// levels 0, keeps the library's default (1, 0.1, 6). With or without set_exposure; one device or a group (the group's
	/// state lives on device 0). Never waits for the device.
	void set_bloom(float threshold = -1.0f, float intensity = -1.0f, int levels = 0) {
		srt_bloom_params p;
		check(srt_bloom_defaults(&p));
		if (threshold >= 0.0f) {
			p.threshold = threshold;
			if (p.knee > threshold) p.knee = threshold; // (0 <= knee <= threshold)
		}
		if (intensity >= 0.0f) p.intensity = intensity;
		if (levels > 0) p.levels = levels;
		check(group ? srt_group_set_bloom(group, &p) : srt_set_bloom(handle, &p));
	}
	/// ... off: the sites resolve as they do without it
	void clear_bloom() { check(group ? srt_group_set_bloom(group, nullptr) : srt_set_bloom(handle, nullptr)); }
	/// Level `level` of the last bloomed frame's pyramid, 4 floats per texel, into `rgba` (resized; nullptr: the size only).
	/// Waits for the device; for a readout, not for the frame loop
	void read_bloom(int level, std::vector<float> *rgba, int *w, int *h) {
		int lw = 0, lh = 0;
		check(group ? srt_group_read_bloom(group, level, nullptr, 0, &lw, &lh) : srt_read_bloom(handle, level, nullptr, 0, &lw, &lh));
		if (rgba) {
			rgba->resize((size_t)lw * (size_t)lh * 4);
			const size_t n = (size_t)lw * (size_t)lh;
			check(group ? srt_group_read_bloom(group, level, rgba->data(), n, &lw, &lh) : srt_read_bloom(handle, level, rgba->data(), n, &lw, &lh));
		}
		if (w) *w = lw;
		if (h) *h = lh;
	}
	/// Whether the last frame's bytes went through the bloom composite
	bool last_resolve_bloomed() {
		int bloomed = 0;
		check(group ? srt_group_last_resolve_bloomed(group, &bloomed) : srt_last_resolve_bloomed(handle, &bloomed));
		return bloomed != 0;
	}
	/// Selection overlay (srt_set_selection): the visible pixels of `shapes` (indices into update_scene's array) are tinted and
	/// outlined in every picture render() / render_pipelined() deliver, as the last step on the bytes. width: pixels, 1..8, a
	/// non-positive one keeps the library's default (2); outline_rrggbbaa / fill_rrggbbaa: 0xRRGGBBAA, fill alpha 0 = no tint. No
	/// shapes: off. The ID pass behind it runs only when the camera or the scene has changed. One device or a group.
	void set_selection(const std::vector<uint32_t> &shapes, float width = 0.0f, uint32_t outline_rrggbbaa = 0xffa000ffu, uint32_t fill_rrggbbaa = 0xffa00000u) {
		srt_selection_params p;
		check(srt_selection_defaults(&p));
		if (width > 0.0f) p.outline_width = width;
		auto argb = [](uint32_t c, uint8_t out[4]) { out[0] = uint8_t(c), out[1] = uint8_t(c >> 24), out[2] = uint8_t(c >> 16), out[3] = uint8_t(c >> 8); };
		argb(outline_rrggbbaa, p.outline_argb), argb(fill_rrggbbaa, p.fill_argb);
		check(group ? srt_group_set_selection(group, &p, shapes.data(), shapes.size()) : srt_set_selection(handle, &p, shapes.data(), shapes.size()));
	}
	/// Area selection (srt_area_coverage): the visible pixels of every shape inside the half-open pixel rectangle of `area`,
	/// optionally cut by a lasso (pixel-corner vertices x0, y0, x1, y1, ...; even-odd rule), counted on the device from the ID
	/// planes of the camera of `options` -- what a rubber band asks. summary (optional): the area's totals. Blocking.
	/// through = true (srt_area_coverage_through): X-ray coverage -- the pixels whose ray meets the shape at all, hidden or not.
	std::vector<uint32_t> area_coverage(srt_area area, const std::vector<int32_t> &lasso = {}, srt_area_summary *summary = nullptr, bool through = false) {
		std::vector<uint32_t> counts((size_t)scene_data.num_shapes);
		srt_area_summary s;
		area.n_vertices = uint32_t(lasso.size() / 2);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		if (through)
			check(group ? srt_group_area_coverage_through(group, rd, &area, lasso.data(), counts.data(), counts.size(), &s)
			            : srt_area_coverage_through(handle, rd, &area, lasso.data(), counts.data(), counts.size(), &s));
		else
			check(group ? srt_group_area_coverage(group, rd, &area, lasso.data(), counts.data(), counts.size(), &s)
			            : srt_area_coverage(handle, rd, &area, lasso.data(), counts.data(), counts.size(), &s));
		if (summary) *summary = s;
		return counts;
	}
	/// The pixels per triangle of model `shape` inside the area (srt_area_triangle_coverage; through = true:
	/// srt_area_triangle_coverage_through, back-facing and hidden faces included). n_triangles: the model's triangle count. Blocking.
	std::vector<uint32_t> area_triangle_coverage(uint32_t shape, size_t n_triangles, srt_area area, const std::vector<int32_t> &lasso = {},
	                                             srt_area_summary *summary = nullptr, bool through = false) {
		std::vector<uint32_t> counts(n_triangles);
		srt_area_summary s;
		area.n_vertices = uint32_t(lasso.size() / 2);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		if (through)
			check(group ? srt_group_area_triangle_coverage_through(group, rd, &area, lasso.data(), shape, counts.data(), counts.size(), &s)
			            : srt_area_triangle_coverage_through(handle, rd, &area, lasso.data(), shape, counts.data(), counts.size(), &s));
		else
			check(group ? srt_group_area_triangle_coverage(group, rd, &area, lasso.data(), shape, counts.data(), counts.size(), &s)
			            : srt_area_triangle_coverage(handle, rd, &area, lasso.data(), shape, counts.data(), counts.size(), &s));
		if (summary) *summary = s;
		return counts;
	}
	/// ... and the shapes with at least min_pixels visible pixels combined with the current selection (mode: SRT_SELECT_REPLACE,
	/// ADD, SUBTRACT, TOGGLE) and overlaid as set_selection overlays a list, with the parameters it was last given. Returns the
	/// new list's length. One call per mouse-move of a drag: under an unchanged camera and scene no ID pass runs. Blocking.
	/// through = true (srt_select_area_through): by the through counts; an infinite plane the frame faces is met by most pixels --
	/// filter it with min_pixels or by type.
	size_t select_area(srt_area area, const std::vector<int32_t> &lasso = {}, int mode = SRT_SELECT_REPLACE, uint32_t min_pixels = 1, bool through = false) {
		size_t n = 0;
		area.n_vertices = uint32_t(lasso.size() / 2);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		if (through)
			check(group ? srt_group_select_area_through(group, rd, &area, lasso.data(), mode, min_pixels, &n)
			            : srt_select_area_through(handle, rd, &area, lasso.data(), mode, min_pixels, &n));
		else check(group ? srt_group_select_area(group, rd, &area, lasso.data(), mode, min_pixels, &n) : srt_select_area(handle, rd, &area, lasso.data(), mode, min_pixels, &n));
		return n;
	}
	/// The current selection, ascending and unique; empty while the overlay is off
	std::vector<uint32_t> read_selection() {
		size_t n = 0;
		check(group ? srt_group_read_selection(group, nullptr, 0, &n) : srt_read_selection(handle, nullptr, 0, &n));
		std::vector<uint32_t> list(n);
		check(group ? srt_group_read_selection(group, list.data(), list.size(), &n) : srt_read_selection(handle, list.data(), list.size(), &n));
		return list;
	}
	/// ... off: the sites resolve as they do without it
	void clear_selection() { check(group ? srt_group_set_selection(group, nullptr, nullptr, 0) : srt_set_selection(handle, nullptr, nullptr, 0)); }
	/// The ID pass alone for the camera of `options` (srt_render_ids): shape, triangle and material per pixel, for read_id_pass.
	/// Asynchronous; single-device tracers only.
	void render_ids() {
		if (group) throw std::runtime_error("Tracer::render_ids: single-device tracers only");
		check(srt_render_ids(handle, reinterpret_cast<const srt_render_data *>(&options)));
	}
	/// The planes of the last ID pass (render_ids, or the overlay's) into the vectors that are not nullptr (resized). Waits for
	/// the device.
	void read_id_pass(std::vector<uint32_t> *shape, std::vector<uint32_t> *triangle, std::vector<int32_t> *material, int *w = nullptr, int *h = nullptr) {
		int pw = 0, ph = 0;
		check(group ? srt_group_read_id_pass(group, nullptr, nullptr, nullptr, 0, &pw, &ph) : srt_read_id_pass(handle, nullptr, nullptr, nullptr, 0, &pw, &ph));
		const size_t n = (size_t)pw * (size_t)ph;
		if (shape) shape->resize(n);
		if (triangle) triangle->resize(n);
		if (material) material->resize(n);
		uint32_t *s = shape ? shape->data() : nullptr, *t = triangle ? triangle->data() : nullptr;
		int32_t *m = material ? material->data() : nullptr;
		check(group ? srt_group_read_id_pass(group, s, t, m, n, &pw, &ph) : srt_read_id_pass(handle, s, t, m, n, &pw, &ph));
		if (w) *w = pw;
		if (h) *h = ph;
	}
	/// Whether the last frame's bytes went through the overlay
	bool last_resolve_selected() {
		int applied = 0;
		check(group ? srt_group_last_resolve_selected(group, &applied, nullptr) : srt_last_resolve_selected(handle, &applied, nullptr));
		return applied != 0;
	}
	/// Noise metering (srt_set_noise_meter): a per-pixel relative standard error from the denoiser's moments, its histogram and
	/// the stopping rule "permille of the pixels below threshold". A non-positive threshold, permille or check_every keeps the
	/// library's default (0.05, 950, 4). Needs set_denoise first (iterations 0 is enough); one device or a group. With it on,
	/// render() and render_pipelined() meter every check_every-th frame on their own and a front-end only polls.
	void set_noise_meter(float threshold = 0.0f, int permille = 0, int check_every = 0) {
		srt_noise_params p;
		check(srt_noise_defaults(&p));
		if (threshold > 0.0f) p.threshold = threshold;
		if (permille > 0) p.permille = permille;
		if (check_every > 0) p.check_every = check_every;
		check(group ? srt_group_set_noise_meter(group, &p) : srt_set_noise_meter(handle, &p));
	}
	/// ... off: every call enqueues what it does without it
	void clear_noise_meter() { check(group ? srt_group_set_noise_meter(group, nullptr) : srt_set_noise_meter(handle, nullptr)); }
	/// Enqueue one metering of the current accumulation. Never waits for the device.
	void meter_noise() { check(group ? srt_group_meter_noise(group) : srt_meter_noise(handle)); }
	/// The newest metering's result; false while its copy is in flight (`result` untouched). Never waits for the device.
	bool poll_noise(srt_noise_result &result) {
		int ready = 0;
		check(group ? srt_group_poll_noise(group, &result, nullptr, &ready) : srt_poll_noise(handle, &result, nullptr, &ready));
		return ready != 0;
	}
	/// ... waiting for that copy only, not for the device's queue
	srt_noise_result read_noise() {
		srt_noise_result r;
		check(group ? srt_group_read_noise(group, &r, nullptr) : srt_read_noise(handle, &r, nullptr));
		return r;
	}
	/// Meter and read back the heat map (green: four octaves below the threshold, red: four above, magenta: left out) into
	/// `output`, width*height*4 bytes. Waits for the device.
	void resolve_noise_view(std::vector<uint8_t> &output) {
		output.resize(size_t(options.width) * size_t(options.height) * 4);
		check(group ? srt_group_resolve_noise_view(group) : srt_resolve_noise_view(handle));
		check(group ? srt_group_read_noise_view(group, output.data()) : srt_read_argb(handle, output.data()));
	}
	/// The ambient-occlusion pass for the camera and frame of `options` (srt_render_ao): per pixel, how many of `samples` hemisphere
	/// rays from the visible surface meet anything within `radius`. A non-positive samples, radius or a negative bias keeps the
	/// library's default (16, +inf, 0.001). Asynchronous; then read_ao() or resolve_ao_view().
	void render_ao(int samples = 0, float radius = 0.0f, float bias = -1.0f, uint32_t seed = 0) {
		srt_ao_params p;
		check(srt_ao_defaults(&p));
		if (samples > 0) p.samples = (uint32_t)samples;
		if (radius > 0.0f) p.radius = radius;
		if (bias >= 0.0f) p.bias = bias;
		p.seed = seed;
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		check(group ? srt_group_render_ao(group, rd, &p) : srt_render_ao(handle, rd, &p));
	}
	/// The last pass's plane (resized): occluded rays per pixel, SRT_HIT_NONE where the pixel has no surface. Returns the pass's
	/// sample count. Waits for the device.
	int read_ao(std::vector<uint32_t> &occluded, int *w = nullptr, int *h = nullptr) {
		int pw = 0, ph = 0, s = 0;
		check(group ? srt_group_read_ao(group, nullptr, 0, &pw, &ph, &s) : srt_read_ao(handle, nullptr, 0, &pw, &ph, &s));
		occluded.resize((size_t)pw * (size_t)ph);
		check(group ? srt_group_read_ao(group, occluded.data(), occluded.size(), &pw, &ph, &s) : srt_read_ao(handle, occluded.data(), occluded.size(), &pw, &ph, &s));
		if (w) *w = pw;
		if (h) *h = ph;
		return s;
	}
	/// The last pass as a grey picture into `output`, width*height*4 bytes (overwrites the handle's image). Waits for the device.
	void resolve_ao_view(std::vector<uint8_t> &output) {
		output.resize(size_t(options.width) * size_t(options.height) * 4);
		check(group ? srt_group_resolve_ao_view(group) : srt_resolve_ao_view(handle));
		check(group ? srt_group_read_ao_view(group, output.data()) : srt_read_argb(handle, output.data()));
	}
	/// Render until converged (srt_render_until): dispatches `options` with time + i * time_stride until a check converges or
	/// max_dispatches are done, then resolves into `output`. Returns the dispatches done; `result` is the deciding check's.
	/// Single-device tracers only.
	uint32_t render_until(uint32_t max_dispatches, std::vector<uint8_t> &output, srt_noise_result &result, uint32_t time_stride = 7919) {
		if (group) throw std::runtime_error("Tracer::render_until: single-device tracers only");
		if (output.size() < size_t(options.width) * size_t(options.height) * 4)
			throw std::runtime_error("Tracer::render_until: output must hold width*height*4 bytes");
		uint32_t done = 0;
		check(srt_render_until(handle, reinterpret_cast<const srt_render_data *>(&options), time_stride, max_dispatches, output.data(), &result, &done));
		return done;
	}
	/// Object motion for the temporal stage (srt_set_denoise_object_motion): the history survives an update_scene that only
	/// moves spheres, planes or model instances. Needs set_denoise_temporal first; the clear_canvas / update_scene / render
	/// order of the frame loop stays as it is. Single-device tracers only (a group gathers no shape indices).
	void set_denoise_object_motion(bool enable = true) {
		if (group) throw std::runtime_error("Tracer::set_denoise_object_motion: single-device tracers only");
		check(srt_set_denoise_object_motion(handle, enable ? 1 : 0));
	}
	/// Per-triangle motion (srt_set_denoise_vertex_motion): the history also survives an update_scene that changes a model's
	/// vertices and keeps its topology (skinning, cloth, morph targets). Needs set_denoise_object_motion first.
	/// Single-device tracers only.
	void set_denoise_vertex_motion(bool enable = true) {
		if (group) throw std::runtime_error("Tracer::set_denoise_vertex_motion: single-device tracers only");
		check(srt_set_denoise_vertex_motion(handle, enable ? 1 : 0));
	}
	/// render() / render_pipelined() record the kernel timers' events too (off by default: they cost 10-17 us of a 150 us
	/// frame); single-device tracers only
	void set_kernel_timers(bool enable) {
		if (!group) check(srt_set_kernel_timers(handle, enable ? 1 : 0));
	}
	void read_canvas(std::vector<float> &rgba) {
		rgba.resize(size_t(options.width) * size_t(options.height) * 4);
		check(group ? srt_group_read_canvas(group, rgba.data()) : srt_read_canvas(handle, rgba.data()));
	}
	srt_counters counters() {
		srt_counters c;
		check(group ? srt_group_get_counters(group, &c) : srt_get_counters(handle, &c));
		return c;
	}
	/// Ray queries (srt_cast_rays): the closest hit of each ray in the scene of the last update_scene, without rendering.
	/// unit_directions: the directions are unit length already and are used bit for bit. Blocking.
	std::vector<srt_ray_hit> cast_rays(const std::vector<srt_ray> &rays, bool unit_directions = false) {
		std::vector<srt_ray_hit> hits(rays.size());
		const uint32_t flags = unit_directions ? SRT_RAYS_UNIT_DIRECTIONS : 0u;
		check(group ? srt_group_cast_rays(group, rays.data(), rays.size(), flags, hits.data()) : srt_cast_rays(handle, rays.data(), rays.size(), flags, hits.data()));
		return hits;
	}
	/// Picking (srt_pick): the hits under image points, xy = {x0, y0, x1, y1, ...} in continuous pixel coordinates of the
	/// frame `options` describes (a pixel's centre is (px + 0.5, py + 0.5)) -- what a mouse handler asks. Blocking.
	std::vector<srt_ray_hit> pick(const std::vector<float> &xy) {
		std::vector<srt_ray_hit> hits(xy.size() / 2);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		check(group ? srt_group_pick(group, rd, xy.data(), hits.size(), hits.data()) : srt_pick(handle, rd, xy.data(), hits.size(), hits.data()));
		return hits;
	}
	srt_ray_hit pick(float x, float y) { return pick(std::vector<float>{x, y})[0]; }
	/// Multi-hit ray queries (srt_cast_rays_multi): the first k hits along each ray in order, hits[q * k + j] the j-th of ray q,
	/// the slots past a ray's last hit holding the miss record; counts (may be null) gets the records written per ray, or with
	/// count_all the size of the ray's whole candidate set. k in 1 .. SRT_MULTI_HIT_MAX. Blocking.
	std::vector<srt_ray_hit> cast_multi(const std::vector<srt_ray> &rays, uint32_t k, std::vector<uint32_t> *counts = nullptr, bool unit_directions = false,
	                                    bool count_all = false) {
		std::vector<srt_ray_hit> hits(rays.size() * k);
		if (counts) counts->assign(rays.size(), 0u);
		const uint32_t flags = (unit_directions ? SRT_RAYS_UNIT_DIRECTIONS : 0u) | (count_all ? SRT_RAYS_COUNT_ALL : 0u);
		uint32_t *c = counts ? counts->data() : nullptr;
		check(group ? srt_group_cast_rays_multi(group, rays.data(), rays.size(), k, flags, hits.data(), c)
		            : srt_cast_rays_multi(handle, rays.data(), rays.size(), k, flags, hits.data(), c));
		return hits;
	}
	/// Click-through picking (srt_pick_through): the first k hits under image points, xy as pick takes it. Blocking.
	std::vector<srt_ray_hit> pick_through(const std::vector<float> &xy, uint32_t k, std::vector<uint32_t> *counts = nullptr) {
		const size_t n = xy.size() / 2;
		std::vector<srt_ray_hit> hits(n * k);
		if (counts) counts->assign(n, 0u);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		uint32_t *c = counts ? counts->data() : nullptr;
		check(group ? srt_group_pick_through(group, rd, xy.data(), n, k, hits.data(), c) : srt_pick_through(handle, rd, xy.data(), n, k, hits.data(), c));
		return hits;
	}
	/// Nearest-surface queries (srt_nearest_points): the closest scene point to each query point, closer than its max_distance
	/// -- what snapping and clearance checks ask. skip_shape: a shape left out (the one being dragged). Blocking.
	std::vector<srt_nearest> nearest(const std::vector<srt_point_query> &queries, uint32_t skip_shape = SRT_HIT_NONE) {
		std::vector<srt_nearest> out(queries.size());
		check(group ? srt_group_nearest_points(group, queries.data(), queries.size(), skip_shape, out.data())
		            : srt_nearest_points(handle, queries.data(), queries.size(), skip_shape, out.data()));
		return out;
	}
	srt_nearest nearest(float x, float y, float z, float max_distance = INFINITY, uint32_t skip_shape = SRT_HIT_NONE) {
		return nearest(std::vector<srt_point_query>{srt_point_query{{x, y, z}, max_distance}}, skip_shape)[0];
	}
	/// Occlusion queries (srt_occluded_rays): is anything closer than tmax along each ray -- true exactly where cast_rays would
	/// report a hit, without looking for the closest one. invalid (optional): the rays the device refused. Blocking.
	std::vector<bool> occluded(const std::vector<srt_ray> &rays, bool unit_directions = false, std::vector<bool> *invalid = nullptr) {
		std::vector<uint64_t> occ((rays.size() + 63) / 64), inv(invalid ? occ.size() : 0);
		const uint32_t flags = unit_directions ? SRT_RAYS_UNIT_DIRECTIONS : 0u;
		check(group ? srt_group_occluded_rays(group, rays.data(), rays.size(), flags, occ.data(), invalid ? inv.data() : nullptr)
		            : srt_occluded_rays(handle, rays.data(), rays.size(), flags, occ.data(), invalid ? inv.data() : nullptr));
		if (invalid) *invalid = mask_bits(inv, rays.size());
		return mask_bits(occ, rays.size());
	}
	/// The rays pick would cast for image points (srt_pick_rays), xy as pick takes it: unit directions, tmax = +inf. Blocking.
	std::vector<srt_ray> pick_rays(const std::vector<float> &xy) {
		const size_t n = xy.size() / 2;
		std::vector<srt_ray> rays(n);
		const srt_render_data *rd = reinterpret_cast<const srt_render_data *>(&options);
		check(group ? srt_group_pick_rays(group, rd, xy.data(), n, rays.data()) : srt_pick_rays(handle, rd, xy.data(), n, rays.data()));
		return rays;
	}
	/// ... between `from` and the point end_gap short of `to` of each segment (srt_occluded_segments): a line of sight.
	std::vector<bool> occluded(const std::vector<srt_segment> &segments, std::vector<bool> *invalid = nullptr) {
		std::vector<uint64_t> occ((segments.size() + 63) / 64), inv(invalid ? occ.size() : 0);
		check(group ? srt_group_occluded_segments(group, segments.data(), segments.size(), occ.data(), invalid ? inv.data() : nullptr)
		            : srt_occluded_segments(handle, segments.data(), segments.size(), occ.data(), invalid ? inv.data() : nullptr));
		if (invalid) *invalid = mask_bits(inv, segments.size());
		return mask_bits(occ, segments.size());
	}
	/// the first n bits of a mask: ray q is bit q & 63 of word q >> 6
	static std::vector<bool> mask_bits(const std::vector<uint64_t> &words, size_t n) {
		std::vector<bool> bits(n);
		for (size_t q = 0; q < n; q++) bits[q] = (words[q >> 6] >> (q & 63)) & 1u;
		return bits;
	}
	srt_tracer *native_handle() { return group ? srt_group_tracer(group, 0) : handle; }
};

static_assert(offsetof(Tracer::RenderData, camera_to_world) == offsetof(srt_render_data, camera_to_world), "RenderData.camera_to_world");
static_assert(offsetof(Tracer::RenderData, time) == offsetof(srt_render_data, time), "RenderData.time");
static_assert(offsetof(Tracer::RenderData, show_normals) == offsetof(srt_render_data, show_normals), "RenderData.show_normals");
static_assert(offsetof(Tracer::SceneData, sun_color) == offsetof(srt_scene_data, sun_color), "SceneData.sun_color");
static_assert(offsetof(Tracer::SceneData, sun_direction) == offsetof(srt_scene_data, sun_direction), "SceneData.sun_direction");
static_assert(offsetof(Tracer::SceneData, horizon_color) == offsetof(srt_scene_data, horizon_color), "SceneData.horizon_color");
