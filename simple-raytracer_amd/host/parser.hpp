// parser.hpp — same interface as the reference's include/parser.hpp / src/parser.cpp:
// the on-disk formats either side of the hot path.
//
//   save_ppm        ARGB8 frame -> binary PPM ("P6 W H 255\n", alpha dropped)
//   load_stl_model  binary STL  -> flat-shaded Triangles (facet normal on all 3 corners)
//   load_obj_model  Wavefront OBJ (v / vn / vt / f, triangulated; optionally usemtl / mtllib) -> smooth-shaded Triangles
//   load_mtl        Wavefront MTL -> named Materials (the mapping is at the function)
//
// Both loaders APPEND to `triangles` and return {first index, count}, or nullopt when
// the file cannot be opened — as the reference does. Deliberate differences (the
// reference's behaviour there is undefined, not a format rule):
//   * OBJ negative indices follow the OBJ spec (-1 = last element so far at the time
//     the whole file is read); the reference computes `len - index + 1` (out of range).
//   * A face without `vn` indices gets the geometric face normal on its three corners;
//     the reference leaves those normals uninitialised.
//   * A truncated STL stops at the last complete record instead of pushing garbage.
//   * Index values outside the vertex / normal lists make the loader return nullopt.
#pragma once

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <optional>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "material.hpp"
#include "shape.hpp"

namespace fs = std::filesystem;

using ModelPair = std::pair<unsigned int, unsigned int>;

inline void save_ppm(const fs::path &filename, const std::vector<uint8_t> &pixels, int width, int height) {
	std::ofstream file(filename, std::ios::binary | std::ios::out);
	file << "P6 " << width << ' ' << height << " 255\n";
	std::vector<char> rgb;
	rgb.reserve(pixels.size() / 4 * 3);
	for (size_t i = 0; i + 3 < pixels.size(); i += 4) { // bytes are A,R,G,B
		rgb.push_back((char)pixels[i + 1]);
		rgb.push_back((char)pixels[i + 2]);
		rgb.push_back((char)pixels[i + 3]);
	}
	file.write(rgb.data(), (std::streamsize)rgb.size());
}

inline std::optional<ModelPair> load_stl_model(const fs::path &filename, std::vector<Triangle> &triangles) {
	std::ifstream file(filename, std::ios::binary | std::ios::in);
	if (file.fail()) return std::nullopt;

	unsigned char header[84]; // 80 bytes of text + little-endian u32 facet count
	file.read(reinterpret_cast<char *>(header), sizeof header);
	if (file.gcount() != (std::streamsize)sizeof header) return ModelPair{(unsigned)triangles.size(), 0u};
	uint32_t count;
	std::memcpy(&count, header + 80, 4);

	const unsigned first = (unsigned)triangles.size();
	unsigned loaded = 0;
	for (uint32_t i = 0; i < count; i++) {
		unsigned char rec[50]; // 12 floats (normal, v1, v2, v3) + u16 attribute
		file.read(reinterpret_cast<char *>(rec), sizeof rec);
		if (file.gcount() != (std::streamsize)sizeof rec) break;
		float f[12];
		std::memcpy(f, rec, sizeof f);
		triangles.push_back(Triangle(glm::vec3(f[0], f[1], f[2]), glm::vec3(f[3], f[4], f[5]), glm::vec3(f[6], f[7], f[8]),
		                             glm::vec3(f[9], f[10], f[11])));
		loaded++;
	}
	return ModelPair{first, loaded};
}

/// `uvs` (optional): receives 6 floats per loaded triangle (u, v of its three corners, from the corners' `vt`; a corner
/// without one, or with an index that does not exist, gets (0, 0)), appended so that the vector stays parallel to
/// `triangles` when it was before: what Tracer::set_triangle_uvs takes.
/// `face_materials` and `material_names` (optional, given together): `usemtl NAME` sets the current name; every loaded triangle
/// appends the index of its name in `material_names` (a name is appended there on first use, so several files can share one
/// list), -1 for a face before any `usemtl`. The caller maps names to indices of its material array (load_mtl) to make what
/// Tracer::set_triangle_materials takes. `mtllibs` (optional): the file names of the `mtllib` lines, as written.
inline std::optional<ModelPair> load_obj_model(const fs::path filename, std::vector<Triangle> &triangles, std::vector<float> *uvs = nullptr,
                                               std::vector<int32_t> *face_materials = nullptr, std::vector<std::string> *material_names = nullptr,
                                               std::vector<std::string> *mtllibs = nullptr) {
	std::ifstream file(filename, std::ios::in);
	if (file.fail()) return std::nullopt;

	struct Corner {
		long v = 0, n = 0; // 1-based / negative as written; n == 0: no normal given
		long t = 0;        // the same for the texture coordinate
	};
	std::vector<glm::vec3> positions, normals;
	std::vector<float> texcoords; // u, v per `vt`
	std::vector<Corner> corners; // 3 per face
	const bool want_materials = face_materials && material_names;
	std::vector<int32_t> corner_face_material; // one per face, parallel to corners / 3
	int32_t current_material = -1;

	std::string line;
	while (std::getline(file, line)) {
		std::istringstream in(line);
		std::string tag;
		in >> tag;
		if (tag == "v") {
			float x = 0, y = 0, z = 0;
			in >> x >> y >> z;
			positions.push_back(glm::vec3(x, y, z));
		} else if (tag == "vn") {
			float x = 0, y = 0, z = 0;
			in >> x >> y >> z;
			normals.push_back(glm::normalize(glm::vec3(x, y, z)));
		} else if (tag == "vt") {
			float u = 0, v = 0;
			in >> u >> v;
			texcoords.push_back(u);
			texcoords.push_back(v);
		} else if (tag == "f") {
			std::string tok;
			int got = 0;
			Corner c[3];
			while (got < 3 && (in >> tok)) {
				// forms: v | v/vt | v//vn | v/vt/vn
				long v = 0, vt = 0, vn = 0;
				if (std::sscanf(tok.c_str(), "%ld/%ld/%ld", &v, &vt, &vn) == 3) {
				} else if (std::sscanf(tok.c_str(), "%ld//%ld", &v, &vn) == 2) {
					vt = 0;
				} else if (std::sscanf(tok.c_str(), "%ld/%ld", &v, &vt) == 2) {
					vn = 0;
				} else if (std::sscanf(tok.c_str(), "%ld", &v) == 1) {
					vn = 0;
					vt = 0;
				} else {
					break;
				}
				c[got].v = v;
				c[got].n = vn;
				c[got].t = vt;
				got++;
			}
			if (got == 3) {
				for (auto &k : c) corners.push_back(k);
				if (want_materials) corner_face_material.push_back(current_material);
			}
		} else if (tag == "usemtl" && want_materials) {
			std::string name;
			in >> name;
			const auto at = std::find(material_names->begin(), material_names->end(), name);
			current_material = (int32_t)(at - material_names->begin());
			if (at == material_names->end()) material_names->push_back(name);
		} else if (tag == "mtllib" && mtllibs) {
			std::string name;
			while (in >> name) mtllibs->push_back(name);
		}
		// '#', 's', 'o', 'g', ... are ignored
	}

	auto resolve = [](long index, size_t len) -> long { // -> 0-based, or -1 when invalid
		if (index > 0) return index <= (long)len ? index - 1 : -1;
		if (index < 0) return (long)len + index >= 0 ? (long)len + index : -1;
		return -1;
	};

	const unsigned first = (unsigned)triangles.size();
	const size_t first_uv = uvs ? uvs->size() : 0;
	const size_t first_fm = want_materials ? face_materials->size() : 0;
	for (size_t f = 0; f + 2 < corners.size(); f += 3) {
		Triangle t;
		bool have_normals = true;
		for (int i = 0; i < 3; i++) {
			long vi = resolve(corners[f + i].v, positions.size());
			if (vi < 0) {
				triangles.resize(first);
				if (uvs) uvs->resize(first_uv);
				if (want_materials) face_materials->resize(first_fm);
				return std::nullopt;
			}
			t.vertices[i].pos = positions[(size_t)vi];
			if (corners[f + i].n == 0) {
				have_normals = false;
			} else {
				long ni = resolve(corners[f + i].n, normals.size());
				if (ni < 0) {
					triangles.resize(first);
					if (uvs) uvs->resize(first_uv);
					if (want_materials) face_materials->resize(first_fm);
					return std::nullopt;
				}
				t.vertices[i].normal = normals[(size_t)ni];
			}
		}
		if (!have_normals) {
			glm::vec3 n = glm::cross(t.vertices[1].pos - t.vertices[0].pos, t.vertices[2].pos - t.vertices[0].pos);
			float len2 = glm::dot(n, n);
			n = len2 > 0.0f ? glm::normalize(n) : glm::vec3(0.0f);
			for (auto &v : t.vertices) v.normal = n;
		}
		triangles.push_back(t);
		if (want_materials) face_materials->push_back(corner_face_material[f / 3]);
		if (uvs)
			for (int i = 0; i < 3; i++) {
				const long ti = corners[f + i].t == 0 ? -1 : resolve(corners[f + i].t, texcoords.size() / 2);
				uvs->push_back(ti < 0 ? 0.0f : texcoords[2 * (size_t)ti]);
				uvs->push_back(ti < 0 ? 0.0f : texcoords[2 * (size_t)ti + 1]);
			}
	}
	return ModelPair{first, (unsigned)(triangles.size() - first)};
}

/// Wavefront MTL -> the file's materials in file order, as (name, Material) pairs; `maps` (optional) receives one `map_Kd` file
/// name per material (empty: none). The mapping is fixed:
///   Kd r g b   color
///   Ke r g b   emission; emission_strength = 1 when any component > 0
///   Ni x       refraction_index
///   d x        transmittance = 1 - x
///   Tr x       transmittance = x
///   Pm x       metallic
///   Pr x       smoothness = 1 - x
///   Ns x       smoothness = clamp(x / 1000, 0, 1), only in a material without Pr
///   map_Kd f   reported through `maps`
/// Everything else starts from Material()'s defaults; unknown keys are ignored; a file that cannot be opened gives an empty list.
inline std::vector<std::pair<std::string, Material>> load_mtl(const fs::path &filename, std::vector<std::string> *maps = nullptr) {
	std::vector<std::pair<std::string, Material>> out;
	std::ifstream file(filename, std::ios::in);
	if (file.fail()) return out;
	bool have_pr = false;
	std::string line;
	while (std::getline(file, line)) {
		std::istringstream in(line);
		std::string tag;
		in >> tag;
		if (tag == "newmtl") {
			std::string name;
			in >> name;
			out.emplace_back(name, Material());
			if (maps) maps->push_back("");
			have_pr = false;
			continue;
		}
		if (out.empty()) continue; // a key before the first newmtl belongs to nothing
		Material &m = out.back().second;
		float x = 0, y = 0, z = 0;
		if (tag == "Kd") {
			in >> x >> y >> z;
			m.color = Color(x, y, z);
		} else if (tag == "Ke") {
			in >> x >> y >> z;
			m.emission = Color(x, y, z);
			m.emission_strength = (x > 0.0f || y > 0.0f || z > 0.0f) ? 1.0f : 0.0f;
		} else if (tag == "Ni") {
			in >> x;
			m.refraction_index = x;
		} else if (tag == "d") {
			in >> x;
			m.transmittance = 1.0f - x;
		} else if (tag == "Tr") {
			in >> x;
			m.transmittance = x;
		} else if (tag == "Pm") {
			in >> x;
			m.metallic = x;
		} else if (tag == "Pr") {
			in >> x;
			m.smoothness = 1.0f - x;
			have_pr = true;
		} else if (tag == "Ns") {
			in >> x;
			if (!have_pr) m.smoothness = std::min(std::max(x / 1000.0f, 0.0f), 1.0f);
		} else if (tag == "map_Kd" && maps) {
			std::string name, last;
			while (in >> name) last = name; // options (-s, -o, ...) come before the file name
			maps->back() = last;
		}
	}
	return out;
}
