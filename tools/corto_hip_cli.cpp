// corto_hip — the `corto` command line tool (upstream src/main.cpp:48-388) on this repo's encoder and GPU decoder.
//
//   corto_hip [OPTIONS] <FILE.ply>
//   corto_hip [OPTIONS] <FILE.ply> <FILE.ply> ...    every file to <stem>.crt in one crthip_encode_batch on device 0
//
// Same options, same defaults and the same flow as upstream: load the model, encode it to <output>.crt, and - with
// -P <file.ply> - decode the blob again (here: on the MI355X through the crt::Decoder facade) and save the decoded mesh
// as a binary PLY laid out like upstream's MeshLoader::savePly (src/meshloader.cpp:294-329), so both files can be compared
// byte for byte with upstream's (tests/test_cli_*.py).  Differences: upstream always runs the round-trip decode to print
// its speed, this tool only when -P asks for the result (the decode needs a GPU; there is no CPU fallback); .obj input,
// per-wedge texture coordinates and `texnumber` groups (upstream's tinyply/objload loaders) are not read.
//
// Build: g++ -O2 -std=c++17 -I include tools/corto_hip_cli.cpp -L corto_amd/lib -lcorto_hip   (python -m corto_amd.build)
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "corto/decoder.h"
#include "corto_hip.h"

namespace {

struct Model {                                  // what upstream's MeshLoader holds after loadPly (src/meshloader.h:45-57)
	uint32_t nvert = 0, nface = 0, ncolor = 0;
	std::vector<float> coords, norms, uvs, radiuses;
	std::vector<uint8_t> colors;
	std::vector<uint32_t> index;
};

// ---- PLY in: ascii / binary_little_endian, scalar properties of any PLY type, one list property per face ----------------
struct Prop { std::string name; int type = 0, list_count_type = -1; };      // type: index into kTypes
const char *const kTypes[][2] = {{"char", "int8"}, {"uchar", "uint8"}, {"short", "int16"}, {"ushort", "uint16"},
                                 {"int", "int32"}, {"uint", "uint32"}, {"float", "float32"}, {"double", "float64"}};
const int kSize[] = {1, 1, 2, 2, 4, 4, 4, 8};

int type_of(const std::string &t) {
	for(int i = 0; i < 8; i++) if(t == kTypes[i][0] || t == kTypes[i][1]) return i;
	return -1;
}

struct Reader {
	std::istream &in;
	bool ascii;
	double scalar(int type) {
		if(ascii) { double v = 0; in >> v; return v; }
		unsigned char b[8] = {0};
		in.read((char *)b, kSize[type]);
		switch(type) {
		case 0: return (double)(int8_t)b[0];
		case 1: return (double)b[0];
		case 2: { int16_t v; memcpy(&v, b, 2); return v; }
		case 3: { uint16_t v; memcpy(&v, b, 2); return v; }
		case 4: { int32_t v; memcpy(&v, b, 4); return v; }
		case 5: { uint32_t v; memcpy(&v, b, 4); return v; }
		case 6: { float v; memcpy(&v, b, 4); return v; }
		default: { double v; memcpy(&v, b, 8); return v; }
		}
	}
};

bool load_ply(const std::string &path, Model &m, std::string &err) {
	std::ifstream in(path, std::ios::binary);
	if(!in.is_open()) { err = "cannot open " + path; return false; }
	std::string line;
	std::getline(in, line);
	if(line.substr(0, 3) != "ply") { err = "not a PLY file"; return false; }
	struct Element { std::string name; size_t count = 0; std::vector<Prop> props; };
	std::vector<Element> elements;
	bool ascii = false, have_format = false;
	while(std::getline(in, line)) {
		if(!line.empty() && line.back() == '\r') line.pop_back();
		std::istringstream ls(line);
		std::string tok;
		ls >> tok;
		if(tok == "end_header") break;
		if(tok == "format") {
			std::string f; ls >> f;
			if(f == "ascii") ascii = true;
			else if(f != "binary_little_endian") { err = "unsupported PLY format " + f; return false; }
			have_format = true;
		} else if(tok == "element") {
			Element e; ls >> e.name >> e.count; elements.push_back(e);
		} else if(tok == "property" && !elements.empty()) {
			Prop p; std::string t; ls >> t;
			if(t == "list") { std::string ct, it; ls >> ct >> it >> p.name; p.list_count_type = type_of(ct); p.type = type_of(it); }
			else { p.type = type_of(t); ls >> p.name; }
			if(p.type < 0) { err = "unknown PLY property type in: " + line; return false; }
			elements.back().props.push_back(p);
		}
	}
	if(!have_format) { err = "PLY header without format"; return false; }
	Reader R{in, ascii};
	for(const Element &e : elements) {
		if(e.name == "vertex") {
			// columns upstream asks tinyply for (src/meshloader.cpp:52-64): the first uv naming that is present wins
			std::map<std::string, int> col;
			for(size_t k = 0; k < e.props.size(); k++) col[e.props[k].name] = (int)k;
			auto has = [&](std::initializer_list<const char *> names) { for(auto n : names) if(!col.count(n)) return false; return true; };
			const bool P = has({"x", "y", "z"}), N = has({"nx", "ny", "nz"}), C3 = has({"red", "green", "blue"}), C4 = C3 && col.count("alpha");
			const char *un = nullptr, *vn = nullptr;
			if(has({"texture_u", "texture_v"})) { un = "texture_u"; vn = "texture_v"; }
			else if(has({"s", "t"})) { un = "s"; vn = "t"; }
			else if(has({"u", "v"})) { un = "u"; vn = "v"; }
			const bool Rd = col.count("radius") != 0;
			if(!P) { err = "PLY vertex element without x, y, z"; return false; }
			m.nvert = (uint32_t)e.count;
			m.coords.resize(e.count*3);
			if(N) m.norms.resize(e.count*3);
			m.ncolor = C4 ? 4 : 0;                 // upstream requests red, green, blue, alpha together (4 components or none)
			if(C4) m.colors.resize(e.count*4);
			if(un) m.uvs.resize(e.count*2);
			if(Rd) m.radiuses.resize(e.count);
			std::vector<double> row(e.props.size());
			for(size_t i = 0; i < e.count; i++) {
				for(size_t k = 0; k < e.props.size(); k++) {
					if(e.props[k].list_count_type >= 0) { const size_t n = (size_t)R.scalar(e.props[k].list_count_type); for(size_t j = 0; j < n; j++) R.scalar(e.props[k].type); row[k] = 0; }
					else row[k] = R.scalar(e.props[k].type);
				}
				m.coords[i*3] = (float)row[col["x"]]; m.coords[i*3 + 1] = (float)row[col["y"]]; m.coords[i*3 + 2] = (float)row[col["z"]];
				if(N) { m.norms[i*3] = (float)row[col["nx"]]; m.norms[i*3 + 1] = (float)row[col["ny"]]; m.norms[i*3 + 2] = (float)row[col["nz"]]; }
				if(C4) { m.colors[i*4] = (uint8_t)row[col["red"]]; m.colors[i*4 + 1] = (uint8_t)row[col["green"]]; m.colors[i*4 + 2] = (uint8_t)row[col["blue"]]; m.colors[i*4 + 3] = (uint8_t)row[col["alpha"]]; }
				if(un) { m.uvs[i*2] = (float)row[col[un]]; m.uvs[i*2 + 1] = (float)row[col[vn]]; }
				if(Rd) m.radiuses[i] = (float)row[col["radius"]];
			}
		} else {
			const bool face = e.name == "face";
			if(face) m.index.reserve(e.count*3);
			for(size_t i = 0; i < e.count; i++)
				for(const Prop &p : e.props) {
					if(p.list_count_type < 0) { R.scalar(p.type); continue; }
					const size_t n = (size_t)R.scalar(p.list_count_type);
					const bool idx = face && (p.name == "vertex_index" || p.name == "vertex_indices");
					if(idx && n != 3) { err = "only triangles are supported"; return false; }
					for(size_t j = 0; j < n; j++) { const double v = R.scalar(p.type); if(idx) m.index.push_back((uint32_t)v); }
				}
		}
		if(!in && !in.eof()) { err = "PLY file ends early"; return false; }
	}
	m.nface = (uint32_t)(m.index.size()/3);
	for(uint32_t v : m.index) if(v >= m.nvert) { err = "face index out of range"; return false; }
	return true;
}

// ---- PLY out: the layout of upstream's savePly through tinyply's binary writer ------------------------------------------
bool save_ply(const std::string &path, const Model &m) {
	FILE *f = fopen(path.c_str(), "wb");
	if(!f) return false;
	std::string h = "ply\nformat binary_little_endian 1.0\n";
	h += "element vertex " + std::to_string(m.nvert) + "\nproperty float x\nproperty float y\nproperty float z\n";
	if(!m.norms.empty()) h += "property float nx\nproperty float ny\nproperty float nz\n";
	if(!m.colors.empty()) { h += "property uchar red\nproperty uchar green\nproperty uchar blue\n"; if(m.ncolor == 4) h += "property uchar alpha\n"; }
	if(!m.uvs.empty()) h += "property float texture_u\nproperty float texture_v\n";
	if(!m.radiuses.empty()) h += "property float radius\n";
	if(m.nface) h += "element face " + std::to_string(m.nface) + "\nproperty list uchar uint vertex_indices\n";
	h += "end_header\n";
	fwrite(h.data(), 1, h.size(), f);
	for(uint32_t i = 0; i < m.nvert; i++) {
		fwrite(&m.coords[(size_t)i*3], 4, 3, f);
		if(!m.norms.empty()) fwrite(&m.norms[(size_t)i*3], 4, 3, f);
		if(!m.colors.empty()) fwrite(&m.colors[(size_t)i*m.ncolor], 1, m.ncolor, f);
		if(!m.uvs.empty()) fwrite(&m.uvs[(size_t)i*2], 4, 2, f);
		if(!m.radiuses.empty()) fwrite(&m.radiuses[i], 4, 1, f);
	}
	for(uint32_t i = 0; i < m.nface; i++) { const uint8_t three = 3; fwrite(&three, 1, 1, f); fwrite(&m.index[(size_t)i*3], 4, 3, f); }
	return fclose(f) == 0;
}

void usage() {
	std::cerr <<
R"use(Usage: corto_hip [OPTIONS] <FILE> [<FILE> ...]

FILE is the path to a .ply 3D model.  With several files, all are encoded in one batch on the GPU,
each to <stem>.crt (-o and -P take one file).
  -o <output>: filename of the .crt compressed file.
               if not specified the extension of the input file will be replaced.
  -e <key=value>: add an exif property, or more than one.
  -p : treat the input as a point cloud.
  -v <bits>: vertex bits quantization. If not specified an euristic is used
  -n <bits>: normal bits quantization. Default 10.
  -c <bits>: color bits quantization. Default 6.
  -u <bits>: texture coordinate bits. Default 12.
  -q <step>: quantization step unit (float) instead of bits for vertex coordinates
  -N <prediction>: normal prediction can be: delta, estimated, border (default)
  -P <file.ply>: decompress on the GPU and save as .ply
)use";
}

bool ends_with(const std::string &s, const std::string &x) { return s.size() >= x.size() && !s.compare(s.size() - x.size(), x.size(), x); }

struct Options {
	bool pointcloud = false;
	float vertex_q = 0.0f;
	int vertex_bits = 0, norm_bits = 10, r_bits = 6, g_bits = 7, b_bits = 6, a_bits = 5, uv_bits = 12;     // src/main.cpp:81-88
	int prediction = 2;                                                   // BORDER, src/main.cpp:163
};

// the crthip_mesh upstream's main builds for a loaded model (src/main.cpp:180-222); points into `in`, `group_end` and `ex`
void describe(Model &in, const Options &o, uint32_t &group_end, const std::string &ex, uint32_t nexif, crthip_mesh &M) {
	group_end = (uint32_t)(in.index.size()/3);                            // loadPly: one group holding every face (src/meshloader.cpp:121), kept under -p
	if(o.pointcloud) in.nface = 0;
	const bool pointcloud = in.nface == 0;
	memset(&M, 0, sizeof(M));
	M.nvert = in.nvert; M.nface = in.nface;
	M.position = in.coords.data();
	M.index = pointcloud ? nullptr : in.index.data();
	M.position_bits = o.vertex_bits; M.position_q = o.vertex_q;         // both 0: upstream's heuristic step
	if(!in.norms.empty() && o.norm_bits > 0) { M.normal = in.norms.data(); M.normal_bits = o.norm_bits; M.normal_prediction = o.prediction; }
	if(!in.colors.empty() && o.r_bits > 0) {
		M.color = in.colors.data(); M.color_components = (int32_t)in.ncolor;
		M.color_bits[0] = o.r_bits; M.color_bits[1] = o.g_bits; M.color_bits[2] = o.b_bits; M.color_bits[3] = o.a_bits;
	}
	if(!in.uvs.empty() && o.uv_bits > 0) { M.uv = in.uvs.data(); M.uv_q = (float)pow(2, -o.uv_bits); }
	if(!in.radiuses.empty()) { M.radius = in.radiuses.data(); M.radius_q = 1.0f; }
	M.group_end = &group_end; M.ngroups = 1;
	M.entropy = CRTHIP_ENTROPY_TUNSTALL;
	M.exif = ex.data(); M.nexif = nexif;
}

bool write_file(const std::string &path, const uint8_t *p, size_t n) {
	FILE *file = fopen(path.c_str(), "wb");
	if(!file) { std::cerr << "Could not open file: " << path << std::endl; return false; }
	const size_t written = fwrite(p, 1, n, file);
	fclose(file);
	if(written != n) { std::cerr << "Failed saving file: " << path << std::endl; return false; }
	return true;
}

// several input files: one crthip_encode_batch on device 0, every file to <stem>.crt (the same bytes as one run per file)
int encode_many(const std::vector<std::string> &inputs, const Options &o, const std::string &ex, uint32_t nexif) {
	const size_t n = inputs.size();
	std::vector<Model> models(n);
	std::vector<uint32_t> group_end(n);
	std::vector<crthip_mesh> meshes(n);
	for(size_t i = 0; i < n; i++) {
		const std::string &input = inputs[i];
		if(!ends_with(input, ".ply") && !ends_with(input, ".PLY")) { std::cerr << "Failed loading model: " << input << " (only .ply input is supported)" << std::endl; return 1; }
		std::string err;
		if(!load_ply(input, models[i], err)) { std::cerr << "Failed loading model: " << input << " (" << err << ")" << std::endl; return 1; }
	}
	for(size_t i = 0; i < n; i++) describe(models[i], o, group_end[i], ex, nexif, meshes[i]);
	crthip_ctx *ctx = nullptr;
	if(crthip_ctx_create(0, &ctx) != CRTHIP_OK) { std::cerr << "Encoding failed: " << crthip_last_error() << std::endl; return 1; }
	std::vector<uint64_t> offs(n + 1);
	std::vector<uint32_t> nvert(n), nface(n);
	std::vector<int32_t> status(n);
	int64_t size = crthip_encode_batch(ctx, (uint32_t)n, meshes.data(), 0, nullptr, 0, offs.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
	std::vector<uint8_t> out(size > 0 ? (size_t)size : 1);
	if(size >= 0) size = crthip_encode_batch(ctx, (uint32_t)n, meshes.data(), 0, out.data(), out.size(), offs.data(), nvert.data(), nface.data(),
	                                         status.data(), nullptr, nullptr);
	if(size < 0) { std::cerr << "Encoding failed: " << crthip_last_error() << std::endl; crthip_ctx_destroy(ctx); return 1; }
	crthip_ctx_destroy(ctx);
	int rc = 0;
	for(size_t i = 0; i < n; i++) {
		if(status[i] != CRTHIP_OK) { std::cerr << "Encoding failed: " << inputs[i] << ": " << crthip_strerror(status[i]) << std::endl; rc = 1; continue; }
		const size_t bytes = (size_t)(offs[i + 1] - offs[i]);
		std::cout << inputs[i] << " Nvert: " << nvert[i] << " Nface: " << nface[i] << " Compressed to: " << bytes << std::endl;
		const std::string output = inputs[i].substr(0, inputs[i].find_last_of(".")) + ".crt";
		if(!write_file(output, out.data() + offs[i], bytes)) rc = 1;
	}
	return rc;
}

} // namespace

int main(int argc, char *argv[]) {
	std::string input, output, plyfile, normal_prediction;
	Options o;
	std::map<std::string, std::string> exif;
	int c;
	while((c = getopt(argc, argv, "pAo:v:n:c:u:q:N:e:P:G:")) != -1) {
		switch(c) {
		case 'o': output = optarg; break;
		case 'p': o.pointcloud = true; break;
		case 'v': o.vertex_bits = atoi(optarg); break;
		case 'n': o.norm_bits = atoi(optarg); break;
		case 'c': o.r_bits = o.g_bits = o.a_bits = o.b_bits = atoi(optarg); break;
		case 'u': o.uv_bits = atoi(optarg); break;
		case 'q': o.vertex_q = (float)atof(optarg); break;
		case 'N': normal_prediction = optarg; break;
		case 'P': plyfile = optarg; break;
		case 'A': std::cerr << "-A (add normals) is not supported" << std::endl; return 1;
		case 'G': std::cerr << "-G applies to .obj input, which is not supported" << std::endl; return 1;
		case 'e': {
			const std::string opt(optarg);
			const size_t pos = opt.find('=');
			if(pos == std::string::npos || pos == 0 || pos == opt.size() - 1) { std::cerr << "Expecting key=value or \"key=another value\" for exif arguments" << std::endl; return 1; }
			exif[opt.substr(0, pos)] = opt.substr(pos + 1);
			break;
		}
		case '?': usage(); return 0;
		default: usage(); return 1;
		}
	}
	if(optind == argc) { std::cerr << "Missing filename" << std::endl; usage(); return 1; }
	auto prediction_ok = [&]() -> bool {
		if(normal_prediction.empty()) return true;
		if(normal_prediction == "delta") o.prediction = 0;
		else if(normal_prediction == "border") o.prediction = 2;
		else if(normal_prediction == "estimated") o.prediction = 1;
		else { std::cerr << "Unknown normal prediction: " << normal_prediction << " expecting: delta, border or estimated" << std::endl; return false; }
		return true;
	};
	std::string ex;
	for(auto &kv : exif) { ex += kv.first; ex.push_back('\0'); ex += kv.second; ex.push_back('\0'); }
	if(optind != argc - 1) {
		if(!output.empty() || !plyfile.empty()) { std::cerr << "-o and -P take one input file; with several, each is written to <stem>.crt" << std::endl; usage(); return 1; }
		if(!prediction_ok()) return 1;
		return encode_many(std::vector<std::string>(argv + optind, argv + argc), o, ex, (uint32_t)exif.size());
	}
	input = argv[optind];
	if(!ends_with(input, ".ply") && !ends_with(input, ".PLY")) { std::cerr << "Failed loading model: " << input << " (only .ply input is supported)" << std::endl; return 1; }

	Model in;
	std::string err;
	if(!load_ply(input, in, err)) { std::cerr << "Failed loading model: " << input << " (" << err << ")" << std::endl; return 1; }
	if(!prediction_ok()) return 1;

	// ---- encode (src/main.cpp:180-222) ----
	crthip_mesh M;
	uint32_t group_end = 0;
	describe(in, o, group_end, ex, (uint32_t)exif.size(), M);
	uint32_t nvert = 0, nface = 0;
	const int64_t size = crthip_encode(&M, nullptr, 0, &nvert, &nface);
	if(size < 0) { std::cerr << "Encoding failed: " << crthip_last_error() << std::endl; return 1; }
	// the blob must sit on a 4-byte boundary for the decoder (src/decoder.cpp:43-44)
	std::vector<uint32_t> blob32(((size_t)size + 3)/4 + 1);
	uint8_t *blob = (uint8_t *)blob32.data();
	if(crthip_encode(&M, blob, (size_t)size, &nvert, &nface) != size) { std::cerr << "Encoding failed: " << crthip_last_error() << std::endl; return 1; }
	std::cout << "Nvert: " << nvert << " Nface: " << nface << std::endl;
	std::cout << "Compressed to: " << size << std::endl;
	std::cout << "Ratio: " << 100.0f*size/(nvert*12 + nface*12) << "%" << std::endl;
	std::cout << "Bpv: " << 8.0f*size/nvert << std::endl << std::endl;

	// ---- decode on the GPU and save, when asked to (src/main.cpp:266-300, 330-331) ----
	if(!plyfile.empty()) {
		Model out;
		try {
			crt::Decoder decoder((int)size, blob);
			if(decoder.nface != nface || decoder.nvert != nvert) { std::cerr << "Decoder disagrees with the encoder about the mesh size" << std::endl; return 1; }
			out.nvert = nvert; out.nface = nface;
			out.coords.resize((size_t)nvert*3);
			decoder.setPositions(out.coords.data());
			if(decoder.data.count("normal")) { out.norms.resize((size_t)nvert*3); decoder.setNormals(out.norms.data()); }
			if(decoder.data.count("color")) { out.ncolor = in.ncolor; out.colors.resize((size_t)nvert*in.ncolor); decoder.setColors(out.colors.data(), (int)in.ncolor); }
			if(decoder.data.count("uv")) { out.uvs.resize((size_t)nvert*2); decoder.setUvs(out.uvs.data()); }
			if(decoder.data.count("radius")) { out.radiuses.resize(nvert); decoder.setAttribute("radius", (char *)out.radiuses.data(), crt::VertexAttribute::FLOAT); }
			if(decoder.nface) { out.index.resize((size_t)nface*3); decoder.setIndex(out.index.data()); }
			decoder.decode();
		} catch(const char *e) { std::cerr << "Decoding failed: " << e << std::endl; return 1; }
		if(!save_ply(plyfile, out)) { std::cerr << "Failed saving file: " << plyfile << std::endl; return 1; }
	}

	if(output.empty()) output = input.substr(0, input.find_last_of("."));
	if(!ends_with(output, ".crt")) output += ".crt";
	return write_file(output, blob, (size_t)size) ? 0 : 1;
}
