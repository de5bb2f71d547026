// size_class_probe.cpp — the decode planner's size-class predicates, answered on the host with the library's own inline functions
// (batch_internal.h, kernels.h), for tests/test_size_classes_cpu.py and tests/test_size_classes_gpu.py.  One query a line on stdin,
// one answer a line on stdout:
//   delta NVERT N U8 WIDE              -> NEED IN_LDS          delta_lds_need (-1: not eligible) / delta_in_lds of one K-DELTA job alone
//   delta_last N U8 WIDE               -> NVERT                the largest nvert whose job is in LDS (0: none)
//   groups WIDE NVERT N:U8 [N:U8 ...]  -> T j.. | G j.. | ...  the jobs of one blob's attributes, in order: those of k_delta_tiles (T),
//                                                             then the k_delta_lds16 workgroups (G), by Planner::group's rule
//   fused NVERT NFACE                  -> FUSED NV_OK NF_OK LDS_OK LDS LDS_FN
//   fused_last_closed                  -> NVERT                the largest closed mesh (nface = 2*nvert - 4) that k_normal_blob takes
//   fn_last_closed FN_MAX              -> NVERT                ... whose face normals fit a launch of FN_MAX bytes (normal_blob_lds_fn)
//   fn FN_MAX NV NF [NV NF ...]        -> LDS_BYTES L..        one k_normal_blob launch of these blobs: its LDS request and where each
//                                                             blob keeps its face normals (lds / scratch / recompute; unfused: not in it)
//   const NAME                         -> VALUE                DELTA16_LDS_MAX, NORMAL_LDS_MAX, NORMAL_FN_LDS_MAX, DELTA16_NVERT_MAX
// Only the group rule and the layout choice are restated here (they live inside Planner methods and the kernel); each cites its lines.
#include "batch_internal.h"

#include <iostream>
#include <sstream>

static DeltaJob job(uint32_t nvert, uint32_t N, uint32_t u8) {
	DeltaJob d{};
	d.nvert = nvert; d.N = N; d.is_u8 = (uint8_t)u8;
	return d;
}

// plan_group.cpp:67-87: tiles first (stable), then consecutive in-LDS jobs of one prediction array and nvert, up to DELTA_GROUP_MAX, while
// their values + the graph (without `a` once a three-component int16 job is in the group) fit DELTA16_LDS_MAX
static std::string groups(bool wide, const std::vector<DeltaJob> &jobs) {
	std::string tiles = "T", out;
	std::vector<size_t> lds;
	for(size_t k = 0; k < jobs.size(); k++) {
		if(!delta_in_lds(jobs[k], wide)) tiles += " " + std::to_string(k);
		else lds.push_back(k);
	}
	size_t j = 0;
	while(j < lds.size()) {
		const DeltaJob &d0 = jobs[lds[j]];
		uint32_t count = 1;
		uint64_t vals = delta_vbytes(d0.nvert, d0.N, d0.is_u8 != 0, wide);
		bool hosted = delta_hosts_a(d0);
		while(j + count < lds.size() && count < DELTA_GROUP_MAX) {
			const DeltaJob &d = jobs[lds[j + count]];
			const uint64_t more = delta_vbytes(d.nvert, d.N, d.is_u8 != 0, wide);
			const bool h2 = hosted || delta_hosts_a(d);
			if(vals + more + delta16_graph_lds(d0.nvert, h2) > DELTA16_LDS_MAX) break;
			vals += more; hosted = h2; count++;
		}
		out += " | G";
		for(uint32_t c = 0; c < count; c++) out += " " + std::to_string(lds[j + c]);
		j += count;
	}
	return tiles + out;
}

// plan_jobs.cpp:262-269 (the launch's LDS request), plan_carve.cpp:96-98 (the scratch array), k_normal.hip:226-231 (the kernel's choice)
static std::string fn_layout(uint32_t fn_max, const std::vector<std::pair<uint32_t, uint32_t>> &blobs) {
	uint32_t lds_bytes = 0;
	for(auto &b : blobs)
		if(normal_fused(b.first, b.second))
			lds_bytes = std::max(lds_bytes, normal_blob_lds_fn(b.first, b.second) <= fn_max ? normal_blob_lds_fn(b.first, b.second) :
				normal_blob_lds(b.first, b.second));
	std::string out = std::to_string(lds_bytes);
	for(auto &b : blobs) {
		if(!normal_fused(b.first, b.second)) { out += " unfused"; continue; }
		const bool scratch = normal_blob_lds_fn(b.first, b.second) > fn_max;
		out += normal_blob_lds_fn(b.first, b.second) <= lds_bytes ? " lds" : scratch ? " scratch" : " recompute";
	}
	return out;
}

int main() {
	std::string line;
	while(std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string q;
		if(!(in >> q)) continue;
		if(q == "delta") {
			uint32_t nv, N, u8, wide; in >> nv >> N >> u8 >> wide;
			const uint64_t need = delta_lds_need(job(nv, N, u8), wide != 0);
			std::cout << (need == ~0ull ? -1ll : (long long)need) << " " << delta_in_lds(job(nv, N, u8), wide != 0) << "\n";
		} else if(q == "delta_last") {
			uint32_t N, u8, wide; in >> N >> u8 >> wide;
			uint32_t last = 0;
			for(uint32_t nv = 1; nv <= 65536; nv++) if(delta_in_lds(job(nv, N, u8), wide != 0)) last = nv;
			std::cout << last << "\n";
		} else if(q == "groups") {
			uint32_t wide, nv; in >> wide >> nv;
			std::vector<DeltaJob> jobs;
			std::string t;
			while(in >> t) {
				const uint32_t N = (uint32_t)std::stoul(t.substr(0, t.find(':'))), u8 = (uint32_t)std::stoul(t.substr(t.find(':') + 1));
				for(uint32_t f = 0; f < N; f += 4) jobs.push_back(job(nv, N, u8));   // plan_jobs.cpp:233: more than four components, a job a slice
			}
			std::cout << groups(wide != 0, jobs) << "\n";
		} else if(q == "fused") {
			uint32_t nv, nf; in >> nv >> nf;
			std::cout << normal_fused(nv, nf) << " " << (nv <= 32767) << " " << ((uint64_t)3*nf <= 65535) << " " << (normal_blob_lds(nv, nf) <= NORMAL_LDS_MAX)
			          << " " << normal_blob_lds(nv, nf) << " " << normal_blob_lds_fn(nv, nf) << "\n";
		} else if(q == "fused_last_closed" || q == "fn_last_closed") {
			uint32_t fn_max = 0;
			if(q == "fn_last_closed") in >> fn_max;
			uint32_t last = 0;
			for(uint32_t nv = 4; nv <= 65536; nv++) {
				const uint32_t nf = 2*nv - 4;
				if(q == "fused_last_closed" ? normal_fused(nv, nf) : normal_fused(nv, nf) && normal_blob_lds_fn(nv, nf) <= fn_max) last = nv;
			}
			std::cout << last << "\n";
		} else if(q == "fn") {
			uint32_t fn_max; in >> fn_max;
			std::vector<std::pair<uint32_t, uint32_t>> blobs;
			uint32_t nv, nf;
			while(in >> nv >> nf) blobs.push_back({nv, nf});
			std::cout << fn_layout(fn_max, blobs) << "\n";
		} else if(q == "const") {
			std::string n; in >> n;
			std::cout << (n == "DELTA16_LDS_MAX" ? DELTA16_LDS_MAX : n == "NORMAL_LDS_MAX" ? NORMAL_LDS_MAX : n == "NORMAL_FN_LDS_MAX" ? NORMAL_FN_LDS_MAX :
			              n == "DELTA16_NVERT_MAX" ? DELTA16_NVERT_MAX : 0u) << "\n";
		} else std::cout << "?\n";
		std::cout.flush();
	}
	return 0;
}

// (batch_internal.h declares these for the library; the probe never calls them)
int fail(int code, const std::string &) { return code; }
int fail(int code) { return code; }
