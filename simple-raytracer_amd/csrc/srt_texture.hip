// srt_texture.hip -- albedo textures and per-triangle materials, host side: what srt_set_textures / srt_set_material_textures /
// srt_set_triangle_uvs / srt_set_triangle_materials store, the checks, the plane frames, the device tables of the textured
// kernels (kernels_tex.hip) and the choice between those and the untextured ones (tex_active). include/srt_abi.h "albedo
// textures" and "per-triangle materials" state the contracts; DESIGN.md §13 and §16.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srt_abi.h"
#include "device_types.h"
#include "srt_internal.h"

namespace {
const int32_t MAX_TEXTURE_SIDE = 16384;

// The frame of a plane, in double, rounded to float once at the end: a = the world axis on which |n| is smallest (ties: x,
// then y, then z), T = normalise(a x n), B = n x T. No frame for a normal that is zero or not finite.
bool plane_frame(const float nf[3], float T[3], float B[3]) {
	for (int k = 0; k < 3; k++) T[k] = B[k] = 0.0f;
	if (!std::isfinite(nf[0]) || !std::isfinite(nf[1]) || !std::isfinite(nf[2])) return false;
	const double n[3] = {nf[0], nf[1], nf[2]};
	if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return false;
	int axis = 0;
	for (int k = 1; k < 3; k++)
		if (std::fabs(n[k]) < std::fabs(n[axis])) axis = k;
	double a[3] = {0.0, 0.0, 0.0};
	a[axis] = 1.0;
	double t[3] = {a[1] * n[2] - a[2] * n[1], a[2] * n[0] - a[0] * n[2], a[0] * n[1] - a[1] * n[0]};
	const double len = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
	if (!(len > 0.0) || !std::isfinite(len)) return false; // (cannot happen for a finite non-zero float normal: the smallest component is dropped)
	for (int k = 0; k < 3; k++) t[k] /= len;
	const double b[3] = {n[1] * t[2] - n[2] * t[1], n[2] * t[0] - n[0] * t[2], n[0] * t[1] - n[1] * t[0]};
	for (int k = 0; k < 3; k++) T[k] = (float)t[k], B[k] = (float)b[k];
	return true;
}

// empty = fine, else what is wrong
std::string check_images(const srt_texture_desc *descs, size_t n) {
	if (n > SRT_MAX_TEXTURES) return "more than SRT_MAX_TEXTURES images";
	if (n && !descs) return "NULL array with non-zero count";
	for (size_t i = 0; i < n; i++) {
		if (!descs[i].rgba) return "image " + std::to_string(i) + " has no texels";
		if (descs[i].width < 1 || descs[i].height < 1 || descs[i].width > MAX_TEXTURE_SIDE || descs[i].height > MAX_TEXTURE_SIDE)
			return "image " + std::to_string(i) + ": width and height must be in 1..16384";
	}
	return "";
}

std::string check_bindings(const srt_material_texture *b, size_t n, size_t n_textures) {
	if (n && !b) return "NULL array with non-zero count";
	for (size_t i = 0; i < n; i++) {
		if (b[i].texture < -1 || (b[i].texture >= 0 && (size_t)b[i].texture >= n_textures))
			return "material " + std::to_string(i) + " binds texture " + std::to_string(b[i].texture) + " but " + std::to_string(n_textures) + " exist";
		if (b[i].filter != SRT_FILTER_LINEAR && b[i].filter != SRT_FILTER_NEAREST) return "material " + std::to_string(i) + ": unknown filter";
		if (!std::isfinite(b[i].scale_u) || !std::isfinite(b[i].scale_v)) return "material " + std::to_string(i) + ": scale is not finite";
	}
	return "";
}

std::string check_uvs(bool has_uvs, size_t uv_triangles, size_t scene_triangles) {
	if (has_uvs && uv_triangles != scene_triangles)
		return "UVs for " + std::to_string(uv_triangles) + " triangles, the scene has " + std::to_string(scene_triangles);
	return "";
}

// per-triangle materials meeting a scene: one entry per triangle, each -1 or a material of the scene
std::string check_tri_materials(bool has, const int32_t *tm, size_t n, size_t scene_triangles, size_t n_materials) {
	if (!has) return "";
	if (n != scene_triangles) return "materials for " + std::to_string(n) + " triangles, the scene has " + std::to_string(scene_triangles);
	for (size_t k = 0; k < n; k++)
		if (tm[k] < -1 || (tm[k] >= 0 && (size_t)tm[k] >= n_materials))
			return "triangle " + std::to_string(k) + " has material " + std::to_string(tm[k]) + " but " + std::to_string(n_materials) + " exist";
	return "";
}

// nothing was given to any setter: nothing to check, nothing to upload
bool nothing_set(const srt_tracer *t) { return t->tex_bindings.empty() && !t->tex_has_uvs && !t->tex_has_tm; }

// after a setter: later dispatches see the new data, the denoiser's history saw the old
void changed(srt_tracer *t) {
	t->tex_dirty = true;
	srt_temporal_drop(t);
}
} // namespace

void srt_texture_scene(srt_tracer *t, const srt_shape *shapes, size_t n_shapes, size_t n_triangles) {
	t->tex_frames_host.assign(n_shapes ? n_shapes : 1, PlaneFrame());
	for (size_t i = 0; i < n_shapes; i++) {
		PlaneFrame &f = t->tex_frames_host[i];
		memset(&f, 0, sizeof f);
		if (shapes[i].type != SRT_SHAPE_PLANE) continue;
		const srt_plane &pl = shapes[i].shape.plane;
		const float n[3] = {pl.normal.x, pl.normal.y, pl.normal.z};
		float T[3], B[3];
		const bool ok = plane_frame(n, T, B);
		f.px = pl.position.x, f.py = pl.position.y, f.pz = pl.position.z, f.valid = ok ? 1.0f : 0.0f;
		f.tx = T[0], f.ty = T[1], f.tz = T[2];
		f.bx = B[0], f.by = B[1], f.bz = B[2];
	}
	t->tex_scene_triangles = n_triangles;
	t->tex_dirty = true;
}

int srt_texture_check_scene(srt_tracer *t, size_t n_triangles, size_t n_materials) {
	if (nothing_set(t)) return SRT_OK;
	std::string bad = check_bindings(t->tex_bindings.data(), t->tex_bindings.size(), t->tex_images.size());
	if (bad.empty()) bad = check_uvs(t->tex_has_uvs, t->tex_uv_host.size() / 6, n_triangles);
	if (bad.empty()) bad = check_tri_materials(t->tex_has_tm, t->tex_tm_host.data(), t->tex_tm_host.size(), n_triangles, n_materials);
	if (!bad.empty()) return fail(t, SRT_ERR_INVALID, "srt_update_scene: textures: " + bad);
	return SRT_OK;
}

int srt_texture_sync(srt_tracer *t) {
	t->tex_active = t->tex_tm_active = false;
	if (nothing_set(t)) return SRT_OK;
	std::string bad = check_bindings(t->tex_bindings.data(), t->tex_bindings.size(), t->tex_images.size());
	if (bad.empty() && t->scene_set) bad = check_uvs(t->tex_has_uvs, t->tex_uv_host.size() / 6, t->tex_scene_triangles);
	if (bad.empty() && t->scene_set)
		bad = check_tri_materials(t->tex_has_tm, t->tex_tm_host.data(), t->tex_tm_host.size(), t->tex_scene_triangles, t->num_materials);
	if (!bad.empty()) return fail(t, SRT_ERR_INVALID, "textures: " + bad);
	if (!t->scene_set) return SRT_OK;
	const size_t n_mat = t->num_materials;
	bool any = false;
	for (size_t i = 0; i < n_mat && i < t->tex_bindings.size(); i++) any = any || t->tex_bindings[i].texture >= 0;
	// per-triangle materials are read by the textured kernels alone: a table that replaces something (an entry >= 0; a checked
	// table is as long as the scene's triangle array, so a scene without triangles has none) launches them with no texture
	// bound too -- every binding of the table below is then -1 and texture_albedo returns the material's colour
	bool any_tm = false;
	for (size_t k = 0; k < t->tex_tm_host.size() && !any_tm; k++) any_tm = t->tex_tm_host[k] >= 0;
	if (!any && !any_tm) return SRT_OK;
	if (t->tex_dirty) {
		std::vector<srt_material_texture> table(n_mat ? n_mat : 1, srt_material_texture{-1, SRT_FILTER_LINEAR, 1.0f, 1.0f});
		for (size_t i = 0; i < n_mat && i < t->tex_bindings.size(); i++) table[i] = t->tex_bindings[i];
		SRT_HIP(t, hipSetDevice(t->device));
		SRT_HIP(t, hipStreamSynchronize(t->stream)); // kernels may still read the old tables
		SRT_HIP(t, t->tex_bind_dev.reserve(table.size()));
		SRT_HIP(t, t->tex_frames.reserve(t->tex_frames_host.size()));
		SRT_HIP(t, hipMemcpy(t->tex_bind_dev.ptr, table.data(), table.size() * sizeof(srt_material_texture), hipMemcpyHostToDevice));
		if (!t->tex_frames_host.empty())
			SRT_HIP(t, hipMemcpy(t->tex_frames.ptr, t->tex_frames_host.data(), t->tex_frames_host.size() * sizeof(PlaneFrame), hipMemcpyHostToDevice));
		if (t->tex_has_uvs && !t->tex_uv_host.empty()) {
			SRT_HIP(t, t->tex_uvs.reserve(t->tex_uv_host.size()));
			SRT_HIP(t, hipMemcpy(t->tex_uvs.ptr, t->tex_uv_host.data(), t->tex_uv_host.size() * sizeof(float), hipMemcpyHostToDevice));
		}
		if (any_tm) {
			SRT_HIP(t, t->tex_tm.reserve(t->tex_tm_host.size()));
			SRT_HIP(t, hipMemcpy(t->tex_tm.ptr, t->tex_tm_host.data(), t->tex_tm_host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		}
		t->tex_dirty = false;
	}
	t->tex_tm_active = any_tm;
	t->tex_active = true;
	return SRT_OK;
}

TexParams srt_texture_params(const srt_tracer *t) {
	TexParams x;
	x.texels = t->tex_texels.ptr;
	x.descs = t->tex_descs.ptr;
	x.bindings = t->tex_bind_dev.ptr;
	x.frames = t->tex_frames.ptr;
	x.tri_uvs = (t->tex_has_uvs && !t->tex_uv_host.empty()) ? t->tex_uvs.ptr : nullptr;
	x.tri_materials = t->tex_tm_active ? t->tex_tm.ptr : nullptr;
	return x;
}

void srt_texture_release(srt_tracer *t) {
	t->tex_texels.release();
	t->tex_uvs.release();
	t->tex_tm.release();
	t->tex_descs.release();
	t->tex_bind_dev.release();
	t->tex_frames.release();
}

extern "C" {

int srt_set_textures(srt_tracer *t, const srt_texture_desc *descs, size_t n) {
	if (!t) return SRT_ERR_INVALID;
	try {
		const std::string bad = check_images(descs, n);
		if (!bad.empty()) return fail(t, SRT_ERR_INVALID, "srt_set_textures: " + bad);
		std::vector<TexDesc> images(n);
		size_t texels = 0;
		for (size_t i = 0; i < n; i++) {
			TexDesc &d = images[i];
			memset(&d, 0, sizeof d);
			d.offset = (uint32_t)texels;
			d.w = descs[i].width, d.h = descs[i].height;
			d.fw = (float)d.w, d.fh = (float)d.h;
			texels += (size_t)d.w * (size_t)d.h; // <= 64 * 2^28: fits 32 bits only just, so
			if (texels > 0x7fffffffu) return fail(t, SRT_ERR_INVALID, "srt_set_textures: more than 2^31 texels");
		}
		SRT_HIP(t, hipSetDevice(t->device));
		SRT_HIP(t, hipStreamSynchronize(t->stream)); // kernels may still read the old images
		// the new set goes into buffers of its own and replaces the old one, host list and device buffers together, only once
		// every copy has succeeded: a failure leaves the handle with the images it had
		DevBuf<float> new_texels;
		DevBuf<TexDesc> new_descs;
		hipError_t e = hipSuccess;
		if (n) {
			e = new_texels.reserve(texels * 4);
			if (e == hipSuccess) e = new_descs.reserve(n);
			for (size_t i = 0; i < n && e == hipSuccess; i++)
				e = hipMemcpy(new_texels.ptr + (size_t)images[i].offset * 4, descs[i].rgba, (size_t)images[i].w * images[i].h * 16, hipMemcpyHostToDevice);
			if (e == hipSuccess) e = hipMemcpy(new_descs.ptr, images.data(), n * sizeof(TexDesc), hipMemcpyHostToDevice);
		}
		if (e != hipSuccess) {
			new_texels.release();
			new_descs.release();
			return fail(t, SRT_ERR_HIP, std::string("srt_set_textures: ") + hipGetErrorString(e));
		}
		t->tex_texels.release(); // (n == 0: nothing is kept)
		t->tex_descs.release();
		t->tex_texels = new_texels;
		t->tex_descs = new_descs;
		t->tex_images.swap(images);
		changed(t);
		return SRT_OK;
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_set_material_textures(srt_tracer *t, const srt_material_texture *bindings, size_t n_materials) {
	if (!t) return SRT_ERR_INVALID;
	try {
		if (!bindings) n_materials = 0;
		t->tex_bindings.assign(bindings, bindings + n_materials);
		changed(t);
		return SRT_OK;
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_set_triangle_uvs(srt_tracer *t, const float *uv, size_t n_triangles) {
	if (!t) return SRT_ERR_INVALID;
	try {
		t->tex_has_uvs = uv != nullptr;
		if (!uv) n_triangles = 0;
		t->tex_uv_host.assign(uv, uv + n_triangles * 6);
		changed(t);
		return SRT_OK;
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_set_triangle_materials(srt_tracer *t, const int32_t *materials, size_t n_triangles) {
	if (!t) return SRT_ERR_INVALID;
	try {
		if (!materials) n_triangles = 0;
		t->tex_has_tm = materials != nullptr && n_triangles != 0;
		t->tex_tm_host.assign(materials, materials + n_triangles);
		changed(t);
		return SRT_OK;
	} catch (...) {
		return fail(t, SRT_ERR_INVALID, "out of host memory");
	}
}

int srt_triangle_materials_check_host(const int32_t *materials, size_t n, size_t scene_triangles, size_t n_materials) {
	try {
		if (!materials && n) return SRT_ERR_INVALID;
		return check_tri_materials(materials != nullptr && n != 0, materials, n, scene_triangles, n_materials).empty() ? SRT_OK : SRT_ERR_INVALID;
	} catch (...) {
		return SRT_ERR_INVALID;
	}
}

int srt_last_trace_textured(const srt_tracer *t, int *textured) {
	if (!t || !textured) return SRT_ERR_INVALID;
	*textured = t->last_trace_textured ? 1 : 0;
	return SRT_OK;
}

int srt_plane_frame_host(const float normal[3], float T[3], float B[3]) {
	if (!normal || !T || !B) return 0;
	return plane_frame(normal, T, B) ? 1 : 0;
}

int srt_texture_check_host(const srt_texture_desc *descs, size_t n_textures, const srt_material_texture *bindings, size_t n_bindings,
                           long long uv_triangles, size_t scene_triangles) {
	try {
		if (n_textures > SRT_MAX_TEXTURES) return SRT_ERR_INVALID;
		if (descs && !check_images(descs, n_textures).empty()) return SRT_ERR_INVALID;
		if (!check_bindings(bindings, n_bindings, n_textures).empty()) return SRT_ERR_INVALID;
		if (!check_uvs(uv_triangles >= 0, uv_triangles >= 0 ? (size_t)uv_triangles : 0, scene_triangles).empty()) return SRT_ERR_INVALID;
		return SRT_OK;
	} catch (...) {
		return SRT_ERR_INVALID;
	}
}

} // extern "C"
