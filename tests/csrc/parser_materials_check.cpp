// parser_materials_check -- a stand-alone driver of host/parser.hpp's material side for tests/test_triangle_materials_host.py:
// load_obj_model with and without the usemtl arguments, and load_mtl. Built by the test with the host compiler (and
// -fsanitize=address,undefined), no GPU and no library needed. Every argument is a file: *.obj or *.mtl; the results are
// printed as lines the test parses.
//   obj FILE ok|none          ok: the loader returned a range
//   range FIRST COUNT
//   names N...                the usemtl names in order of first use
//   faces I...                one index per loaded triangle
//   mtllibs F...
//   plain same|different      the loader without the new arguments, on vectors of its own: triangles and UVs byte for byte
//   mtl FILE COUNT
//   material NAME smoothness metallic specular emission_strength transmittance refraction_index r g b er eg eb MAP|-
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../simple-raytracer_amd/host/parser.hpp"

static bool ends_with(const std::string &s, const char *tail) {
	const size_t n = std::strlen(tail);
	return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

int main(int argc, char **argv) {
	for (int i = 1; i < argc; i++) {
		const std::string path = argv[i];
		if (ends_with(path, ".mtl")) {
			std::vector<std::string> maps;
			const auto mats = load_mtl(path, &maps);
			std::printf("mtl %s %zu\n", path.c_str(), mats.size());
			if (maps.size() != mats.size()) return 4;
			for (size_t k = 0; k < mats.size(); k++) {
				const Material &m = mats[k].second;
				std::printf("material %s %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %s\n", mats[k].first.c_str(), m.smoothness, m.metallic,
				            m.specular, m.emission_strength, m.transmittance, m.refraction_index, m.color.x, m.color.y, m.color.z, m.emission.x, m.emission.y,
				            m.emission.z, maps[k].empty() ? "-" : maps[k].c_str());
			}
			if (load_mtl(path).size() != mats.size()) return 4; // (without the optional vector)
			continue;
		}
		// two triangles and their UVs and indices are there already: the loader appends and keeps the vectors parallel
		std::vector<Triangle> tris(2), plain_tris(2);
		std::vector<float> uvs(12, 0.5f), plain_uvs(12, 0.5f);
		std::vector<int32_t> faces(2, -1);
		std::vector<std::string> names, mtllibs;
		const auto got = load_obj_model(path, tris, &uvs, &faces, &names, &mtllibs);
		const auto plain = load_obj_model(path, plain_tris, &plain_uvs);
		std::printf("obj %s %s\n", path.c_str(), got ? "ok" : "none");
		if (got.has_value() != plain.has_value()) return 5;
		if (faces.size() != tris.size() || uvs.size() != tris.size() * 6) return 6; // parallel, after a failure too
		if (got) std::printf("range %u %u\n", got->first, got->second);
		std::printf("names");
		for (auto &n : names) std::printf(" %s", n.c_str());
		std::printf("\nfaces");
		for (size_t k = 2; k < faces.size(); k++) std::printf(" %d", faces[k]);
		std::printf("\nmtllibs");
		for (auto &n : mtllibs) std::printf(" %s", n.c_str());
		bool same = tris.size() == plain_tris.size() && uvs == plain_uvs && (!got || *got == *plain);
		for (size_t k = 0; same && k < tris.size(); k++)
			for (int c = 0; c < 3; c++) // (field by field: the padding of a Triangle holds nothing)
				same = same && std::memcmp(&tris[k].vertices[c].pos, &plain_tris[k].vertices[c].pos, sizeof(glm::vec3)) == 0 &&
				       std::memcmp(&tris[k].vertices[c].normal, &plain_tris[k].vertices[c].normal, sizeof(glm::vec3)) == 0;
		std::printf("\nplain %s\n", same ? "same" : "different");
		// one list of names shared by two loads: the second load finds the names of the first
		std::vector<int32_t> faces2(tris.size(), -1);
		const size_t n_names = names.size();
		if (load_obj_model(path, tris, nullptr, &faces2, &names, nullptr) && names.size() != n_names) return 7;
	}
	return 0;
}
