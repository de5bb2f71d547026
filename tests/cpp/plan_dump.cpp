// plan_dump.cpp — the decode planner without a GPU: a stand-alone program built from plan_carve.cpp, plan_jobs.cpp, plan_group.cpp, batch_bind.cpp,
// meshlet_host.cpp, crt_format.cpp and host_probe.cpp as plain C++ (no HIP runtime is linked: the stubs below stand in for harvest, drop_staged
// and the four allocation calls; the pinned blocks are mapped at fixed addresses and the scratch block has a fixed fake one, so a plan's bytes are
// the same from run to run).
// It walks a corpus of real blobs (tests/test_plan_jobs_cpu.py encodes them), fills crthip_batch::blobs as batch.cpp's fill does, binds through the
// C ABI with constant fake addresses - the planner never dereferences the arena, the scratch block or a caller's buffer - and runs carve(), jobs(),
// group() and upload() for every scenario.  Two things come of it:
//   - the invariants of the plan that no other CPU test sees (checked always; the exit code says whether they held), and
//   - with --dump FILE, every job array as raw bytes, the Plan's scalars, every scratch offset, the Planner's counters, each blob's host status,
//     the staged image and the status block as upload() leaves them, and the code and message of every bind call: what two builds of the planner
//     are compared by (profiles/plan_jobs.md, profiles/plan_launch.md).
// The program names no field that holds a derived binding: it builds against any tree that has these files.
#include "batch_internal.h"

#include <sys/mman.h>

// ---- what the planner's stages and the bind calls need of batch.cpp and of the HIP runtime ----
int harvest(crthip_ctx *) { return CRTHIP_OK; }
void drop_staged(crthip_batch *) {}
static const uintptr_t PIN_BASE = 0x600000000000ull, PIN_SLOT = 1ull << 30;
static size_t pin_bytes[8];
extern "C" hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) {
	for(int s = 0; s < 8; s++) {
		if(pin_bytes[s]) continue;
		void *p = mmap((void *)(PIN_BASE + s*PIN_SLOT), size, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED_NOREPLACE, -1, 0);
		if(p != (void *)(PIN_BASE + s*PIN_SLOT)) { fprintf(stderr, "plan_dump: the fixed mapping failed\n"); exit(2); }
		pin_bytes[s] = size; *ptr = p;
		return hipSuccess;
	}
	return hipErrorOutOfMemory;
}
extern "C" hipError_t hipHostFree(void *ptr) {
	const size_t s = ((uintptr_t)ptr - PIN_BASE)/PIN_SLOT;
	munmap(ptr, pin_bytes[s]); pin_bytes[s] = 0;
	return hipSuccess;
}
static const uintptr_t DEV_BASE = 0x300000000000ull, ARENA_BASE = 0x400000000000ull, CALLER_BASE = 0x500000000000ull;
extern "C" hipError_t hipMalloc(void **ptr, size_t) { *ptr = (void *)DEV_BASE; return hipSuccess; }   // the scratch block: upload() only adds to its address
extern "C" hipError_t hipFree(void *) { return hipSuccess; }

// ---- the corpus (tests/test_plan_jobs_cpu.py writes it in this order) ----
enum { B_EST, B_BORDER, B_DIFF, B_NONORMAL, B_CLOUD, B_TANBIG, B_UNFUSED, B_BEYOND16, B_SIXCOMP, B_COUNT };
struct Blob { std::vector<uint32_t> words; uint32_t len; };
static std::vector<Blob> corpus;
static FILE *dump = nullptr;
static int nscenes = 0, narrays = 0, nfailed = 0;
#define CHECK(cond, ...) do { if(!(cond)) { nfailed++; printf("FAILED [%s] %s: ", name.c_str(), #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

struct Options { int tun_share = -1; bool wide = false, single_stream = false; uint32_t qout_blob_max = 0; };
// what a scenario expects of its plan beyond the checks every plan gets (-1: not looked at)
struct Expect {
	int computed = -1, tangent = -1, meshlet = -1, bounds = -1, adjacency = -1, weld = -1;
	bool no_derived = false;
	bool no_pos_out = false;                // a position that is not FLOAT: no normal kernel finishes it
	std::vector<uint32_t> ints_kept;        // blobs with tangents or bounds: the position's integers last until k_dequant
	std::vector<uint32_t> pos_by_normal;    // blobs with one fused reader and neither: the normal kernel writes the float positions
};

static void hex(std::string &s, const void *p, size_t n) {
	static const char *d = "0123456789abcdef";
	for(size_t i = 0; i < n; i++) { s.push_back(d[((const uint8_t *)p)[i] >> 4]); s.push_back(d[((const uint8_t *)p)[i] & 15]); }
}
static void put(std::string &s, const char *key, uint64_t v) { char t[96]; snprintf(t, sizeof t, " %s=%llu", key, (unsigned long long)v); s += t; }

struct Scene {
	std::string name, log;
	crthip_ctx ctx; crthip_batch b;
	uintptr_t next = CALLER_BASE;
	std::vector<std::vector<crthip_attr_binding>> at;    // what bind() hands over for each blob
	std::vector<void *> index;

	Scene(const char *name_, std::vector<int> which, Options o = Options{}) : name(name_) {
		ctx.dbg = DebugConfig{}; ctx.dbg.tun_share = o.tun_share; ctx.dbg.qout_blob_max = o.qout_blob_max;
		ctx.delta.wide = o.wide;
		if(o.single_stream) { ctx.single_stream = 1; ctx.normal_fn_max = 0; }            // (crthip_ctx_set_single_stream)
		b.ctx = &ctx; b.d_arena = (const uint8_t *)ARENA_BASE;
		b.blobs.resize(which.size()); at.resize(which.size()); index.assign(which.size(), nullptr);
		uint64_t off = 0;
		for(size_t i = 0; i < which.size(); i++) {
			BlobPlan &P = b.blobs[i]; const Blob &src = corpus[which[i]];
			reset_layout(P.L);
			if(walk_blob((const uint8_t *)src.words.data(), src.len, P.L)) { fprintf(stderr, "plan_dump: corpus blob %d does not walk\n", which[i]); exit(2); }
			P.arena_off = off; P.len = src.len; P.bind.assign(P.L.h.attrs.size(), Binding{});
			off += ((uint64_t)src.len + 15) & ~15ull;
			// every attribute in its usual format, packed; the index as uint32
			for(const AttrHeader &a : P.L.h.attrs) {
				crthip_attr_binding d{};
				d.buffer = addr(); d.format = a.codec == CRTHIP_CODEC_COLOR ? CRTHIP_FMT_UINT8 : CRTHIP_FMT_FLOAT;
				at[i].push_back(d);
			}
			if(P.L.h.nface) index[i] = addr();
		}
		b.arena_bytes = off; b.status.assign(which.size(), 0);
		for(uint32_t i = 0; i < which.size(); i++) bind(i);
	}
	~Scene() { for(crthip_ctx::Half &h : ctx.set) h.release(); }
	void *addr() { next += 0x1000000; return (void *)next; }
	const BlobLayout &L(uint32_t i) const { return b.blobs[i].L; }
	int attr(uint32_t i, const char *n) const { int k = -1; for(size_t j = 0; j < L(i).h.attrs.size(); j++) if(L(i).h.attrs[j].name == n) k = (int)j; return k; }
	crthip_attr_binding &A(uint32_t i, const char *n) { static crthip_attr_binding absent; const int k = attr(i, n); return k < 0 ? absent : at[i][k]; }   // (absent: edits go nowhere)

	int call(const char *what, uint32_t i, int rc) {
		char t[64]; snprintf(t, sizeof t, "C %s blob=%u rc=%d", what, i, rc);
		log += t; if(rc) { log += " error="; log += crthip_last_error(); } log += "\n";
		return rc;
	}
	int bind(uint32_t i, uint32_t index_format = CRTHIP_FMT_UINT32) { return call("bind", i, crthip_batch_bind(&b, i, at[i].data(), index[i], index_format)); }
	int normals(uint32_t i, bool on = true, uint32_t fmt = CRTHIP_FMT_FLOAT, uint32_t stride = 0) {
		return call("normals", i, crthip_batch_bind_computed_normals(&b, i, on ? addr() : nullptr, fmt, stride)); }
	int tangents(uint32_t i, bool on = true, uint32_t fmt = CRTHIP_FMT_FLOAT, uint32_t stride = 0) {
		return call("tangents", i, crthip_batch_bind_computed_tangents(&b, i, on ? addr() : nullptr, fmt, stride)); }
	crthip_meshlet_binding meshlet_binding(uint32_t i, uint32_t segment_faces, bool counts) {
		crthip_meshlet_counts cap{};
		crthip_meshlet_bound(L(i).h.nface, (uint32_t)L(i).group_end.size(), L(i).group_end.data(), 64, 124, segment_faces, &cap);
		crthip_meshlet_binding m{};
		m.meshlets = (crthip_meshlet *)addr(); m.vertices = (uint32_t *)addr(); m.triangles = (uint8_t *)addr(); m.counts = counts ? (crthip_meshlet_counts *)addr() : nullptr;
		m.meshlet_capacity = cap.meshlets; m.vertex_capacity = cap.vertices; m.triangle_capacity = cap.triangle_bytes;
		m.max_vertices = 64; m.max_triangles = 124; m.segment_faces = segment_faces;
		return m;
	}
	int meshlets(uint32_t i, const crthip_meshlet_binding *m) { return call("meshlets", i, crthip_batch_bind_meshlets(&b, i, m)); }
	int meshlets(uint32_t i, uint32_t segment_faces = 0, bool counts = true) { const crthip_meshlet_binding m = meshlet_binding(i, segment_faces, counts); return meshlets(i, &m); }
	crthip_adjacency_binding adjacency_binding(uint32_t i, bool counts) {
		crthip_adjacency_binding a{};
		a.twin = (uint32_t *)addr(); a.counts = counts ? (crthip_adjacency_counts *)addr() : nullptr; a.capacity = 3*L(i).h.nface;
		return a;
	}
	int adjacency(uint32_t i, const crthip_adjacency_binding *a) { return call("adjacency", i, crthip_batch_bind_adjacency(&b, i, a)); }
	int adjacency(uint32_t i, bool counts = true) { const crthip_adjacency_binding a = adjacency_binding(i, counts); return adjacency(i, &a); }
	crthip_weld_binding weld_binding(uint32_t i, bool index, bool counts, uint32_t flags = 0) {
		crthip_weld_binding w{};
		w.remap = (uint32_t *)addr(); w.index = index ? (uint32_t *)addr() : nullptr; w.counts = counts ? (crthip_weld_counts *)addr() : nullptr;
		w.remap_capacity = L(i).h.nvert; w.index_capacity = index ? 3*L(i).h.nface : 0; w.flags = flags;
		return w;
	}
	int weld(uint32_t i, const crthip_weld_binding *w) { return call("weld", i, crthip_batch_bind_weld(&b, i, w)); }
	int weld(uint32_t i, bool index = true, bool counts = true, uint32_t flags = 0) { const crthip_weld_binding w = weld_binding(i, index, counts, flags); return weld(i, &w); }
	int bounds(uint32_t i, bool on = true, uint32_t capacity = ~0u) { return call("bounds", i, crthip_batch_bind_meshlet_bounds(&b, i, on ? (crthip_meshlet_bounds *)addr() : nullptr, capacity)); }

	// The staged image, word by word (8-byte words at 8-byte aligned device addresses).  No word is an unresolved scratch pointer - bit 63 set, the
	// rest below the block's size: a pointer field that upload() does not resolve would hand a kernel that address.  (Two adjacent uint32 fields
	// whose upper one is exactly 0x80000000 would look like one; no descriptor of this corpus holds such a pair.)  A word that upload() changed is a
	// resolved pointer - an SP offset, TopoJob::group_end, MeshletJob::segs: it lies in the scratch block.  (A word it left alone is a pointer to the
	// arena, a caller's buffer or the pinned block, null, or a pair of integers: without a list of the pointer fields - upload()'s own list over
	// again - nothing tells them apart, and pairs like (nvert, nface) = (0x8100, 0x4f7d) do fall among this program's fake addresses.)
	void check_image(const Planner &P, const Plan &pl, const std::vector<uint8_t> &before) {
		const uintptr_t base = (uintptr_t)P.base;
		CHECK(base == DEV_BASE, "the scratch block is at %llx", (unsigned long long)base);
		auto in = [](uint64_t w, uint64_t lo, uint64_t bytes) { return w >= lo && w < lo + bytes; };
		for(size_t o = (8 - pl.jobs_begin % 8) % 8; o + 8 <= pl.jobs_bytes; o += 8) {
			uint64_t w, w0; memcpy(&w, P.stage + o, 8); memcpy(&w0, before.data() + o, 8);
			CHECK(!((w >> 63) && (w & ~(1ull << 63)) < pl.total), "byte %zu of the staged image is the unresolved scratch pointer %016llx", o, (unsigned long long)w);
			if(w != w0) CHECK(in(w, base, pl.total), "byte %zu of the staged image was resolved to %016llx, outside the scratch block of %llu bytes", o, (unsigned long long)w, (unsigned long long)pl.total);
		}
		// the zeroing FillJobs of a scratch table cover it exactly: adjacency's ends of a blob beyond LDS, the weld's table of one
		auto zeroed = [&](const char *what, const void *table, uint64_t bytes) {
			uint64_t cur = (uintptr_t)table, sum = 0;
			for(bool more = true; more && cur < (uintptr_t)table + bytes;) {
				more = false;
				for(const FillJob &f : pl.fill.v) if((uintptr_t)f.dst == cur && f.value == 0 && f.size) { cur += f.size; more = true; break; }
			}
			for(const FillJob &f : pl.fill.v) if(in((uintptr_t)f.dst, (uintptr_t)table, bytes)) sum += f.size;
			CHECK(cur == (uintptr_t)table + bytes && sum == bytes, "the zero fills of %s end %lld bytes from the table's end and write %llu of its %llu bytes", what,
				(long long)((uintptr_t)table + bytes - cur), (unsigned long long)sum, (unsigned long long)bytes);
		};
		for(const AdjacencyJob &a : pl.adjacency.v) if(a.ends) zeroed("an adjacency job's ends", a.ends, ((uint64_t)a.nvert + 1)*4);
		for(const WeldJob &w : pl.weld.v) if(w.table) zeroed("a weld job's table", w.table, weld_scratch_layout(w.nvert).record);
	}

	// carve, jobs, group, upload; the plan as text (returned, and written to the dump behind the scenario's calls); the checks
	std::string plan(const Expect &ex = Expect{}) {
		crthip_ctx::Half &set = ctx_set(&ctx, &b);
		set.plan.reset();
		Planner P(&b);
		int rc = P.carve();
		if(!rc) rc = P.jobs();
		if(!rc) P.group();
		Plan &pl = set.plan;
		std::string s;
		put(s, "plan_rc", (uint64_t)(int64_t)rc); s += "\n";
		static const char *names[] = {"tun", "tun_dict", "tun_chunk_stream", "tun_group_ids", "tun_groups", "fill", "topo", "aux_u32", "topo_lds_ids", "topo_big_ids",
			"topo_glob_ids", "unpack", "unpack_chunk_job", "unpack_wave_ids", "delta", "delta_groups", "cloud", "cloud_chunk_job", "normal", "nv_block_job", "nv_block_first",
			"nf_block_job", "nf_block_first", "normal_fused_ids", "normal_computed_ids", "dequant", "dequant_block_job", "quant", "quant_blob_ids", "quant_block_job",
			"tangent", "tangent_blob_ids", "tan_fblock_job", "tan_vblock_job", "meshlet", "meshlet_blob_ids", "mlt_block_job", "meshlet_bounds", "mlb_block_job"};
		size_t k = 0;
		pl.each_array([&](auto &arr) {
			s += "A "; s += k < sizeof names/sizeof *names ? names[k] : "?";
			put(s, "size", sizeof(arr.v[0])); put(s, "n", arr.v.size()); put(s, "dev_off", arr.dev_off); s += " ";
			hex(s, arr.v.data(), arr.v.size()*sizeof(arr.v[0])); s += "\n";
			k++; narrays++;
		});
		CHECK(k == sizeof names/sizeof *names, "each_array has %zu arrays", k);
		static const char *optional[] = {"adjacency", "adjacency_blob_ids", "adj_big_ids", "adj_block_job", "weld", "weld_blob_ids", "weld_vblock_job", "weld_cblock_job"};
		k = 0;
		pl.each_optional_array([&](auto &arr) {
			s += "O "; s += k < sizeof optional/sizeof *optional ? optional[k] : "?";
			put(s, "size", sizeof(arr.v[0])); put(s, "n", arr.v.size()); put(s, "dev_off", arr.dev_off); s += " ";
			hex(s, arr.v.data(), arr.v.size()*sizeof(arr.v[0])); s += "\n";
			CHECK(!arr.v.empty() || arr.dev_off == 0, "the empty optional array %s is placed at %llu", optional[k < 8 ? k : 7], (unsigned long long)arr.dev_off);
			k++; narrays++;
		});
		CHECK(k == sizeof optional/sizeof *optional, "each_optional_array has %zu arrays", k);
		s += "P";
		put(s, "clers_groups", pl.clers_groups); put(s, "topo_lds", pl.topo_lds); put(s, "topo_big_lds", pl.topo_big_lds); put(s, "normal_fused_lds", pl.normal_fused_lds);
		put(s, "normal_computed_lds", pl.normal_computed_lds); put(s, "tangent_lds", pl.tangent_lds); put(s, "meshlet_waves", pl.meshlet_waves);
		put(s, "meshlet_records", pl.meshlet_records); put(s, "quant_records", pl.quant_records); put(s, "zero_begin", pl.zero_begin); put(s, "zero_end", pl.zero_end);
		put(s, "tables_off", pl.tables_off); put(s, "tun_partial_off", pl.tun_partial_off); put(s, "unpack_partial_off", pl.unpack_partial_off);
		put(s, "cloud_partial_off", pl.cloud_partial_off); put(s, "facen_off", pl.facen_off); put(s, "cnt_off", pl.cnt_off); put(s, "cursor_off", pl.cursor_off);
		put(s, "bnd_off", pl.bnd_off); put(s, "start_off", pl.start_off); put(s, "flag_off", pl.flag_off); put(s, "slot_off", pl.slot_off); put(s, "adj_off", pl.adj_off);
		put(s, "nscan_partial_off", pl.nscan_partial_off); put(s, "jobs_begin", pl.jobs_begin); put(s, "jobs_bytes", pl.jobs_bytes); put(s, "est_nvert", pl.est_nvert);
		put(s, "est_nface", pl.est_nface); put(s, "delta16_lds", pl.delta16_lds); put(s, "tun_multi_chunk", pl.tun_multi_chunk); put(s, "any_diff_normal", pl.any_diff_normal);
		put(s, "any_est_normal", pl.any_est_normal); put(s, "tun_max_nchunks", pl.tun_max_nchunks); put(s, "total", pl.total);
		s += " topo_need="; for(uint32_t nd : pl.topo_need) s += std::to_string(nd) + ",";
		s += "\nN";
		put(s, "unpack_state_words", P.unpack_state_words); put(s, "n_tun", P.n_tun); put(s, "stat_tin", P.stat_tin); put(s, "stat_tout", P.stat_tout); put(s, "stat_tt", P.stat_tt);
		put(s, "tun_chunks", P.tun_chunks); put(s, "unpack_chunks", P.unpack_chunks); put(s, "cloud_chunks", P.cloud_chunks); put(s, "clers_tun", P.clers_tun);
		put(s, "clers_chunks", P.clers_chunks); put(s, "clers_fill", P.clers_fill); put(s, "clers_dict", P.clers_dict); put(s, "share_clers", P.share_clers);
		put(s, "share_attrs", P.share_attrs); put(s, "hs_base", (uint64_t)(uintptr_t)P.hs_base);
		s += "\n";
		for(uint32_t i = 0; i < b.blobs.size(); i++) {
			const BlobPlan &B = b.blobs[i]; const BlobScratch &S = set.plan_scratch[i];
			s += "B"; put(s, "blob", i); put(s, "host_status", (uint64_t)(int64_t)B.host_status); put(s, "dbg_clers", B.dbg_clers); put(s, "dbg_pred", B.dbg_pred);
			put(s, "dbg_nclers", B.dbg_nclers); put(s, "clers_in_arena", B.clers_in_arena);
			put(s, "clers", S.clers); put(s, "pred", S.pred); put(s, "front_a", S.front_a); put(s, "front_b", S.front_b); put(s, "order", S.order); put(s, "delayed", S.delayed);
			put(s, "faces", S.faces); put(s, "progress", S.progress); put(s, "front_cap", S.front_cap); put(s, "aux_groups", S.aux_groups); put(s, "tan_acc", S.tan_acc);
			put(s, "mlt", S.mlt); put(s, "mlt_counts", S.mlt_counts); put(s, "cn_facen", S.cn_facen); put(s, "adj", S.adj); put(s, "weld", S.weld); s += "\n";
			for(size_t a = 0; a < S.nattr; a++) {
				const AttrScratch &T = S.attr[a];
				s += " T"; put(s, "attr", a); put(s, "color", T.color); put(s, "diffs", T.diffs); put(s, "vals", T.vals); put(s, "facen", T.facen); put(s, "qrange", T.qrange);
				s += " sym="; for(uint64_t y : T.sym) s += std::to_string(y) + ",";
				s += "\n";
			}
		}
		// upload(): the image of the job arrays before it (SP offsets) and as it staged them (addresses), the status block as it prefilled it
		std::vector<uint8_t> before;
		if(!rc) {
			before.assign(pl.jobs_bytes, 0);
			auto image = [&](auto &arr) { if(!arr.v.empty()) memcpy(before.data() + (arr.dev_off - pl.jobs_begin), arr.v.data(), arr.v.size()*sizeof(arr.v[0])); };
			pl.each_array(image); pl.each_optional_array(image);
			if(set.staging.p) memset(set.staging.p, 0, set.staging.cap);      // (upload() never writes the gaps between the arrays: an earlier plan's bytes would show)
			rc = P.upload();
			s += "U"; put(s, "upload_rc", (uint64_t)(int64_t)rc); put(s, "base", (uint64_t)(uintptr_t)P.base); put(s, "stage", (uint64_t)(uintptr_t)P.stage);
			if(!rc) { s += "\nI "; hex(s, P.stage, pl.jobs_bytes); s += "\nH "; hex(s, set.status_host.p, P.hs.bytes()); }
			s += "\n";
		}
		if(dump) { fprintf(dump, "S %s\n%s%s", name.c_str(), log.c_str(), s.c_str()); }
		log.clear(); nscenes++;
		if(rc) { CHECK(rc == 0, "the plan failed with %d", rc); return s; }
		check_image(P, pl, before);

		// every id below its job array's size
		auto ids = [&](const char *what, const std::vector<uint32_t> &v, size_t n) { for(uint32_t id : v) CHECK(id < n, "%s holds %u, the job array has %zu", what, id, n); };
		ids("tun_chunk_stream", pl.tun_chunk_stream.v, pl.tun.v.size()); ids("tun_group_ids", pl.tun_group_ids.v, pl.tun.v.size());
		ids("topo_lds_ids", pl.topo_lds_ids.v, pl.topo.v.size()); ids("topo_big_ids", pl.topo_big_ids.v, pl.topo.v.size()); ids("topo_glob_ids", pl.topo_glob_ids.v, pl.topo.v.size());
		ids("unpack_chunk_job", pl.unpack_chunk_job.v, pl.unpack.v.size()); ids("unpack_wave_ids", pl.unpack_wave_ids.v, pl.unpack.v.size());
		ids("cloud_chunk_job", pl.cloud_chunk_job.v, pl.cloud.v.size());
		ids("nv_block_job", pl.nv_block_job.v, pl.normal.v.size()); ids("nf_block_job", pl.nf_block_job.v, pl.normal.v.size());
		ids("normal_fused_ids", pl.normal_fused_ids.v, pl.normal.v.size()); ids("normal_computed_ids", pl.normal_computed_ids.v, pl.normal.v.size());
		ids("dequant_block_job", pl.dequant_block_job.v, pl.dequant.v.size());
		ids("quant_blob_ids", pl.quant_blob_ids.v, pl.quant.v.size()); ids("quant_block_job", pl.quant_block_job.v, pl.quant.v.size());
		ids("tangent_blob_ids", pl.tangent_blob_ids.v, pl.tangent.v.size()); ids("tan_fblock_job", pl.tan_fblock_job.v, pl.tangent.v.size()); ids("tan_vblock_job", pl.tan_vblock_job.v, pl.tangent.v.size());
		ids("meshlet_blob_ids", pl.meshlet_blob_ids.v, pl.meshlet.v.size()); ids("mlt_block_job", pl.mlt_block_job.v, pl.meshlet.v.size());
		ids("mlb_block_job", pl.mlb_block_job.v, pl.meshlet_bounds.v.size());
		ids("adjacency_blob_ids", pl.adjacency_blob_ids.v, pl.adjacency.v.size()); ids("adj_big_ids", pl.adj_big_ids.v, pl.adjacency.v.size()); ids("adj_block_job", pl.adj_block_job.v, pl.adjacency.v.size());
		ids("weld_blob_ids", pl.weld_blob_ids.v, pl.weld.v.size()); ids("weld_vblock_job", pl.weld_vblock_job.v, pl.weld.v.size()); ids("weld_cblock_job", pl.weld_cblock_job.v, pl.weld.v.size());
		for(const TunStream &t : pl.tun.v) CHECK(t.dict < pl.tun_dict.v.size(), "a stream's dictionary %u of %zu", t.dict, pl.tun_dict.v.size());
		for(const TunGroup &g : pl.tun_groups.v) CHECK((size_t)g.first + g.count <= pl.tun_group_ids.v.size(), "a stream group ends at %u", g.first + g.count);
		for(const DeltaGroup &g : pl.delta_groups.v) CHECK((size_t)g.first + g.count <= pl.delta.v.size(), "a delta group ends at %u", g.first + g.count);

		// an estimate has its position; the unfused ones take consecutive slices of the batch-wide arrays, in job order, and carve() sized those for their sum
		int computed = 0; uint32_t vsum = 0, fsum = 0;
		for(const NormalJob &n : pl.normal.v) {
			computed += n.prediction == 3;
			if(n.prediction == 0) continue;
			CHECK(n.position && n.faces, "an estimated normal job without its position or index");
			CHECK(!n.pos_out || n.fused, "a separate normal kernel asked to write the positions");
			if(ex.no_pos_out) CHECK(!n.pos_out, "the normal kernel finishes a position that is not FLOAT");
			if(n.fused) continue;
			CHECK(n.vbase == vsum && n.fbase == fsum, "an unfused job's slices start at %u / %u, the jobs before it end at %u / %u", n.vbase, n.fbase, vsum, fsum);
			vsum += n.nvert; fsum += n.nface;
		}
		bool refused = false;                                                // (a refused blob keeps the room carve() gave it)
		for(const BlobPlan &B : b.blobs) refused = refused || B.host_status;
		CHECK(refused ? vsum <= pl.est_nvert && fsum <= pl.est_nface : vsum == pl.est_nvert && fsum == pl.est_nface, "the unfused jobs take %u vertices and %u faces, carve() laid out %u and %u", vsum, fsum, pl.est_nvert, pl.est_nface);
		CHECK((size_t)computed >= pl.normal_computed_ids.v.size(), "%d computed jobs, %zu ids", computed, pl.normal_computed_ids.v.size());
		if(ex.no_derived) {
			CHECK(computed == 0 && pl.normal_computed_ids.v.empty(), "%d computed normal jobs", computed);
			CHECK(pl.tangent.v.empty() && pl.tangent_blob_ids.v.empty() && pl.tan_fblock_job.v.empty() && pl.tan_vblock_job.v.empty(), "%zu tangent jobs", pl.tangent.v.size());
			CHECK(pl.meshlet.v.empty() && pl.meshlet_blob_ids.v.empty() && pl.mlt_block_job.v.empty(), "%zu meshlet jobs", pl.meshlet.v.size());
			CHECK(pl.meshlet_bounds.v.empty() && pl.mlb_block_job.v.empty(), "%zu bounds jobs", pl.meshlet_bounds.v.size());
			CHECK(!pl.meshlet_records && !pl.quant_records, "records behind the status words: %u quant, meshlet %d", pl.quant_records, (int)pl.meshlet_records);
			pl.each_optional_array([&](auto &arr) { CHECK(arr.v.empty() && arr.dev_off == 0, "an optional array of %zu entries at %llu", arr.v.size(), (unsigned long long)arr.dev_off); });
		}
		if(ex.computed >= 0) CHECK(computed == ex.computed, "%d computed normal jobs, expected %d", computed, ex.computed);
		if(ex.tangent >= 0) CHECK((int)pl.tangent.v.size() == ex.tangent, "%zu tangent jobs, expected %d", pl.tangent.v.size(), ex.tangent);
		if(ex.meshlet >= 0) CHECK((int)pl.meshlet.v.size() == ex.meshlet && pl.meshlet_records == (ex.meshlet > 0), "%zu meshlet jobs, expected %d", pl.meshlet.v.size(), ex.meshlet);
		if(ex.bounds >= 0) CHECK((int)pl.meshlet_bounds.v.size() == ex.bounds, "%zu bounds jobs, expected %d", pl.meshlet_bounds.v.size(), ex.bounds);
		if(ex.adjacency >= 0) CHECK((int)pl.adjacency.v.size() == ex.adjacency && pl.adjacency.v.size() == pl.adjacency_blob_ids.v.size() + pl.adj_big_ids.v.size(), "%zu adjacency jobs, expected %d", pl.adjacency.v.size(), ex.adjacency);
		if(ex.weld >= 0) CHECK((int)pl.weld.v.size() == ex.weld, "%zu weld jobs, expected %d", pl.weld.v.size(), ex.weld);
		for(uint32_t i : ex.ints_kept) {
			const void *pos = b.blobs[i].bind[attr(i, "position")].buffer;
			int dq = 0;
			for(const DeltaJob &d : pl.delta.v) if(d.values == pos) CHECK(d.deq != 1, "blob %u: K-DELTA turns the position into floats in front of its integer readers", i);
			for(const DequantJob &q : pl.dequant.v) dq += q.buffer == pos;
			for(const NormalJob &n : pl.normal.v) CHECK(n.pos_out != pos, "blob %u: the normal kernel writes the float positions in front of later integer readers", i);
			CHECK(dq == 1, "blob %u: %d k_dequant jobs for the position", i, dq);
		}
		for(uint32_t i : ex.pos_by_normal) {
			const void *pos = b.blobs[i].bind[attr(i, "position")].buffer;
			int writers = 0;
			for(const NormalJob &n : pl.normal.v) if(n.position == pos) { CHECK(n.fused && n.pos_out == pos, "blob %u: the one fused reader does not write the float positions", i); writers++; }
			CHECK(writers == 1, "blob %u: %d normal jobs read the position", i, writers);
			for(const DequantJob &q : pl.dequant.v) CHECK(q.buffer != pos, "blob %u: a k_dequant job for a position the normal kernel finishes", i);
			for(const DeltaJob &d : pl.delta.v) if(d.values == pos) CHECK(d.deq == 0, "blob %u: K-DELTA finishes a position the normal kernel reads", i);
		}
		return s;
	}
};

// ------------------------------------------------------------------------------------------------
static void scenarios() {
	std::string name = "scenarios";
	const std::vector<int> small = {B_EST, B_BORDER, B_DIFF, B_NONORMAL, B_CLOUD};
	std::vector<int> all; for(int k = 0; k < B_COUNT; k++) all.push_back(k);
	Expect none; none.no_derived = true;

	// nothing derived: every blob of the corpus; K-DELTA's 32-bit layout; a single-stream context; the dictionary switches
	std::string plain_small;
	{ Scene s("plain, every blob", all); s.plan(none); }
	{ Scene s("plain, small blobs", small); Expect e = none; e.pos_by_normal = {0, 1}; plain_small = s.plan(e); }
	{ Options o; o.wide = true; Scene s("plain, delta.wide", all, o); s.plan(none); }
	{ Options o; o.single_stream = true; Scene s("plain, normal_fn_max 0", all, o); s.plan(none); }
	for(int share : {0, 1, 2}) { Options o; o.tun_share = share; Scene s(("plain, tun_share " + std::to_string(share)).c_str(), all, o); s.plan(none); }
	{ Scene s("two runs of one batch object", small); const std::string a = s.plan(none), c = s.plan(none); CHECK(a == c, "the second plan of one object differs"); }

	// the index: uint16, and none bound
	{ Scene s("index u16 / unbound", {B_EST, B_BORDER, B_NONORMAL, B_UNFUSED});
	  s.bind(0, CRTHIP_FMT_UINT16); s.index[1] = nullptr; s.bind(1); s.bind(2, CRTHIP_FMT_UINT16); s.index[3] = nullptr; s.bind(3);
	  s.normals(2); s.tangents(2); s.meshlets(2); s.bounds(2); s.tangents(0); s.meshlets(1, 1); s.bounds(1);
	  Expect e; e.computed = 1; e.tangent = 2; e.meshlet = 2; e.bounds = 2; e.ints_kept = {0, 1, 2}; s.plan(e); }

	// the position's binding: strided, DOUBLE, quantised in both size classes, stream values (a stored estimate is then refused, alone)
	for(int v = 0; v < 6; v++) {
		static const char *vn[] = {"strided", "DOUBLE", "INT16", "quantised, k_quant_out_blob", "quantised, k_quant_range", "stream values"};
		Options o; if(v == 4) o.qout_blob_max = 16;
		Scene s((std::string("position ") + vn[v]).c_str(), {B_EST, B_EST, B_NONORMAL, B_CLOUD, B_BEYOND16}, o);
		for(uint32_t i = 0; i < 5; i++) {
			crthip_attr_binding &p = s.A(i, "position");
			if(v == 0) p.stride = 16;
			if(v == 1) p.format = CRTHIP_FMT_DOUBLE;
			if(v == 2) p.format = CRTHIP_FMT_INT16;
			if(v == 3 || v == 4) { p.format = CRTHIP_FMT_UINT16; p.reserved = CRTHIP_BIND_QUANTIZED; if(i == 1) p.stride = 8; }
			if(v == 5) { p.format = CRTHIP_FMT_INT32; p.reserved = CRTHIP_BIND_STREAM_VALUES; }
			s.bind(i);
		}
		if(v == 3) s.call("quant_transforms", 0, crthip_batch_bind_quant_transforms(&s.b, s.addr()));
		s.normals(2); s.tangents(1); s.tangents(2); s.meshlets(1); s.bounds(1); s.meshlets(2, 32, false); s.bounds(2);
		Expect e; const bool ok = v != 5;
		e.computed = ok; e.tangent = ok ? 2 : 0; e.meshlet = 2; e.bounds = ok ? 2 : 0; e.no_pos_out = v >= 1 && v <= 4;
		s.plan(e);
		if(!ok) CHECK(s.b.blobs[0].host_status == CRTHIP_E_NORMAL_NEEDS_POSITION && s.b.blobs[2].host_status == 0, "host status %d, %d", s.b.blobs[0].host_status, s.b.blobs[2].host_status);
	}
	{ Scene s("position unbound under stored estimates", {B_EST, B_BORDER, B_DIFF, B_UNFUSED});
	  for(uint32_t i = 0; i < 4; i++) { s.A(i, "position").buffer = nullptr; s.bind(i); }
	  s.plan(none);
	  CHECK(s.b.blobs[0].host_status == CRTHIP_E_NORMAL_NEEDS_POSITION && s.b.blobs[1].host_status == CRTHIP_E_NORMAL_NEEDS_POSITION && s.b.blobs[2].host_status == 0 &&
		s.b.blobs[3].host_status == CRTHIP_E_NORMAL_NEEDS_POSITION, "host status of a refused stored normal"); }
	{ Scene s("quantised uv, colour and six components", {B_EST, B_SIXCOMP, B_CLOUD});
	  for(uint32_t i = 0; i < 3; i++) { crthip_attr_binding &u = s.A(i, "uv"); u.format = CRTHIP_FMT_UINT16; u.reserved = CRTHIP_BIND_QUANTIZED; s.A(i, "color").out_components = 4;
		s.A(i, "color").stride = 8; s.A(i, "normal").format = CRTHIP_FMT_INT16; s.bind(i); }
	  s.tangents(0); Expect e; e.tangent = 1; e.ints_kept = {0}; s.plan(e); }

	// each derived output alone
	{ Scene s("computed normals alone", {B_NONORMAL, B_EST, B_UNFUSED, B_UNFUSED, B_BEYOND16, B_TANBIG});
	  s.A(1, "normal").buffer = nullptr; s.bind(1); s.A(3, "normal").buffer = nullptr; s.bind(3); s.A(4, "normal").buffer = nullptr; s.bind(4);
	  s.normals(0); s.normals(1, true, CRTHIP_FMT_INT16); s.normals(3, true, CRTHIP_FMT_FLOAT, 16); s.normals(4);
	  Expect e; e.computed = 4; e.tangent = e.meshlet = e.bounds = 0; e.pos_by_normal = {0, 1, 5}; s.plan(e); }
	{ Options o; o.single_stream = true; Scene s("computed and stored normals, normal_fn_max 0", {B_NONORMAL, B_EST, B_BORDER, B_UNFUSED}, o);
	  s.normals(0); Expect e; e.computed = 1; e.pos_by_normal = {0, 1, 2}; s.plan(e); }
	{ Scene s("tangents over stored normals", {B_EST, B_BORDER, B_DIFF, B_TANBIG, B_UNFUSED, B_BEYOND16});
	  s.tangents(0); s.tangents(1, true, CRTHIP_FMT_INT16); s.tangents(2, true, CRTHIP_FMT_FLOAT, 32); s.tangents(3); s.tangents(4, true, CRTHIP_FMT_INT16, 16); s.tangents(5);
	  Expect e; e.computed = 0; e.tangent = 6; e.meshlet = e.bounds = 0; e.ints_kept = {0, 1, 2, 3, 4, 5}; s.plan(e); }
	{ Scene s("tangents over computed normals", {B_NONORMAL, B_EST, B_TANBIG});
	  for(uint32_t i = 1; i < 3; i++) { s.A(i, "normal").buffer = nullptr; s.bind(i); }
	  for(uint32_t i = 0; i < 3; i++) { s.normals(i, true, i == 1 ? CRTHIP_FMT_INT16 : CRTHIP_FMT_FLOAT); s.tangents(i); }
	  Expect e; e.computed = 3; e.tangent = 3; e.ints_kept = {0, 1, 2}; s.plan(e); }
	{ Scene s("meshlets, one segment", {B_EST, B_NONORMAL, B_CLOUD, B_DIFF}); s.meshlets(0); s.meshlets(1, 0, false);
	  Expect e; e.computed = e.tangent = e.bounds = 0; e.meshlet = 2; e.pos_by_normal = {0}; s.plan(e); }
	{ Scene s("meshlets, segments of one face and of 32", {B_EST, B_NONORMAL, B_UNFUSED}); s.meshlets(0, 1); s.meshlets(1, 32, false); s.meshlets(2, 4096);
	  Expect e; e.meshlet = 3; e.bounds = 0; s.plan(e); }
	{ Scene s("meshlet bounds, with and without a device counts record", {B_EST, B_BORDER, B_NONORMAL, B_TANBIG});
	  s.meshlets(0); s.bounds(0); s.meshlets(1, 0, false); s.bounds(1); s.meshlets(2, 1, false); s.bounds(2, true, 100000); s.meshlets(3, 1024); s.bounds(3);
	  Expect e; e.meshlet = 4; e.bounds = 4; e.tangent = 0; e.ints_kept = {0, 1, 2, 3}; s.plan(e); }

	// all four together
	{ Scene s("all four, tangents over stored normals", {B_EST, B_BORDER, B_DIFF, B_TANBIG, B_UNFUSED});
	  for(uint32_t i = 0; i < 5; i++) { s.tangents(i); s.meshlets(i, i == 1 ? 16 : 0, i != 2); s.bounds(i); }
	  Expect e; e.computed = 0; e.tangent = e.meshlet = e.bounds = 5; e.ints_kept = {0, 1, 2, 3, 4}; s.plan(e); }
	{ Scene s("all four, tangents over computed normals", {B_NONORMAL, B_EST, B_UNFUSED, B_EST});
	  for(uint32_t i = 1; i < 3; i++) { s.A(i, "normal").buffer = nullptr; s.bind(i); }
	  for(uint32_t i = 0; i < 3; i++) { s.normals(i); s.tangents(i); s.meshlets(i, i ? 8 : 0); s.bounds(i); }
	  Expect e; e.computed = 3; e.tangent = e.meshlet = e.bounds = 3; e.ints_kept = {0, 1, 2}; e.pos_by_normal = {3}; s.plan(e); }

	// adjacency and the weld: the 40-vertex sphere inside LDS, 33 024 vertices beyond adj_in_blob and weld_in_blob
	{ Scene s("adjacency alone, with and without a counts record", {B_EST, B_NONORMAL, B_BEYOND16, B_BEYOND16, B_CLOUD});
	  s.adjacency(0); s.adjacency(1, false); s.adjacency(2); s.adjacency(3, false);
	  Expect e; e.computed = e.tangent = e.meshlet = e.bounds = e.weld = 0; e.adjacency = 4; e.pos_by_normal = {0}; s.plan(e);
	  const Plan &pl = s.ctx.set[0].plan;
	  CHECK(pl.adjacency_blob_ids.v.size() == 2 && pl.adj_big_ids.v.size() == 2, "%zu adjacency jobs in LDS, %zu beyond it", pl.adjacency_blob_ids.v.size(), pl.adj_big_ids.v.size());
	  for(const AdjacencyJob &a : pl.adjacency.v) CHECK(!a.ends == !a.list && (a.counts || !a.ends), "an adjacency job with one of its two scratch arrays, or beyond LDS without a counts record"); }
	{ Scene s("weld alone, with and without the welded index and a counts record", {B_EST, B_EST, B_BEYOND16, B_BEYOND16, B_UNFUSED, B_CLOUD});
	  s.weld(0); s.weld(1, false, false); s.weld(2, true, false); s.weld(3, false, true); s.weld(4);
	  Expect e; e.computed = e.tangent = e.meshlet = e.bounds = e.adjacency = 0; e.weld = 5; e.ints_kept = {0, 1, 2, 3, 4}; s.plan(e);
	  const Plan &pl = s.ctx.set[0].plan;
	  CHECK(pl.weld_blob_ids.v.size() == 2 && !pl.weld_vblock_job.v.empty() && !pl.weld_cblock_job.v.empty(), "%zu weld jobs in LDS", pl.weld_blob_ids.v.size());
	  for(const WeldJob &w : pl.weld.v) CHECK(w.position && w.index && w.remap && (w.table ? w.counts != nullptr : true), "a weld job without an input, or one beyond LDS without a counts record"); }
	{ Scene s("CRTHIP_WELD_ADJACENCY", {B_EST, B_BEYOND16, B_EST, B_BEYOND16});
	  std::vector<const void *> welded;
	  for(uint32_t i = 0; i < 4; i++) {
		const crthip_weld_binding w = s.weld_binding(i, true, i & 1, i < 2 ? CRTHIP_WELD_ADJACENCY : 0u);
		welded.push_back(i < 2 ? (const void *)w.index : s.index[i]);
		if(i & 1) { s.adjacency(i); s.weld(i, &w); } else { s.weld(i, &w); s.adjacency(i, false); }     // (the order of the two calls does not matter)
	  }
	  Expect e; e.adjacency = e.weld = 4; s.plan(e);
	  const Plan &pl = s.ctx.set[0].plan;
	  for(size_t j = 0; j < pl.adjacency.v.size() && j < 4; j++)
		CHECK(pl.adjacency.v[j].index == welded[j] && (j >= 2 || !pl.adjacency.v[j].index_u16), "adjacency job %zu does not read the index its weld flag says", j); }

	// all six together
	{ Scene s("all six, tangents over stored and over computed normals", {B_EST, B_BORDER, B_TANBIG, B_BEYOND16, B_NONORMAL});
	  s.normals(4);
	  for(uint32_t i = 0; i < 5; i++) { s.tangents(i); s.meshlets(i, i == 3 ? 4096 : 0, i != 1); s.bounds(i); s.weld(i, i != 2, i != 0, i & 1 ? CRTHIP_WELD_ADJACENCY : 0u); s.adjacency(i, i != 4); }
	  Expect e; e.computed = 1; e.tangent = e.meshlet = e.bounds = e.adjacency = e.weld = 5; e.ints_kept = {0, 1, 2, 3, 4}; s.plan(e); }

	// the cascades: what each call drops
	{ Scene s("binding and unbinding adjacency and the weld", small);
	  s.adjacency(0); s.weld(0); s.adjacency(3, false); s.weld(3, true, false, CRTHIP_WELD_ADJACENCY);
	  { Expect e; e.adjacency = e.weld = 2; e.computed = e.tangent = e.meshlet = e.bounds = 0; s.plan(e); }
	  s.adjacency(0, nullptr); s.adjacency(3, nullptr);
	  { Expect e; e.adjacency = 0; e.weld = 2; s.plan(e); }
	  s.weld(0, nullptr); s.weld(3, nullptr);
	  Expect after = none; after.pos_by_normal = {0, 1};
	  CHECK(s.plan(after) == plain_small, "binding and then unbinding adjacency and the weld does not give the plan of a batch that never bound them"); }
	{ Scene s("a bind drops adjacency and the weld", small);
	  s.adjacency(0); s.weld(0); s.adjacency(3); s.weld(3);
	  { Expect e; e.adjacency = e.weld = 2; s.plan(e); }
	  s.bind(0); s.bind(3);
	  Expect after = none; after.pos_by_normal = {0, 1};
	  CHECK(s.plan(after) == plain_small, "a bind behind adjacency and the weld does not give the plan of a batch that never had them"); }
	{ Scene s("bind after everything derived", small);
	  s.normals(3); s.tangents(3); s.meshlets(3); s.bounds(3); s.tangents(0); s.meshlets(0); s.bounds(0);
	  Expect e; e.computed = 1; e.tangent = 2; e.meshlet = 2; e.bounds = 2; s.plan(e);
	  s.bind(3); s.bind(0);
	  Expect after = none; after.pos_by_normal = {0, 1};
	  CHECK(s.plan(after) == plain_small, "a bind behind the derived calls does not give the plan of a batch that never had them"); }
	{ Scene s("a normals call drops the tangents", {B_NONORMAL, B_EST});
	  s.normals(0); s.tangents(0); s.tangents(1); s.meshlets(0); s.bounds(0);
	  s.normals(0); s.normals(1, false);
	  Expect e; e.computed = 1; e.tangent = 0; e.meshlet = 1; e.bounds = 1; e.ints_kept = {0}; e.pos_by_normal = {1}; s.plan(e); }
	{ Scene s("a meshlets call drops the bounds", {B_NONORMAL, B_EST});
	  s.normals(0); s.tangents(0); s.meshlets(0); s.bounds(0); s.meshlets(1); s.bounds(1);
	  s.meshlets(0, 8); s.meshlets(1, nullptr);
	  Expect e; e.computed = 1; e.tangent = 1; e.meshlet = 1; e.bounds = 0; e.ints_kept = {0}; e.pos_by_normal = {1}; s.plan(e); }
	{ Scene s("unbinding with null, one output at a time", small);
	  s.normals(3); s.tangents(3); s.meshlets(3); s.bounds(3); s.tangents(0); s.meshlets(0); s.bounds(0);
	  s.bounds(3, false); s.bounds(0, false);
	  { Expect e; e.computed = 1; e.tangent = 2; e.meshlet = 2; e.bounds = 0; e.ints_kept = {0, 3}; s.plan(e); }
	  s.tangents(3, false); s.tangents(0, false);
	  { Expect e; e.computed = 1; e.tangent = 0; e.meshlet = 2; e.bounds = 0; e.pos_by_normal = {0, 1, 3}; s.plan(e); }
	  s.meshlets(3, nullptr); s.meshlets(0, nullptr);
	  { Expect e; e.computed = 1; e.tangent = e.meshlet = e.bounds = 0; s.plan(e); }
	  s.normals(3, false);
	  Expect after = none; after.pos_by_normal = {0, 1};
	  CHECK(s.plan(after) == plain_small, "binding and then unbinding every derived output does not give the plan of a batch that never bound them"); }

	// the refusals: every code and message, in the order of the checks; the bindings stay as they were
	{ Scene s("refusals", {B_EST, B_CLOUD, B_NONORMAL, B_SIXCOMP, B_EST});
	  { const crthip_meshlet_binding m{}; s.normals(9); s.tangents(9); s.meshlets(9, &m); s.bounds(9); } s.call("bind", 9, crthip_batch_bind(&s.b, 9, nullptr, nullptr, 0));
	  s.call("bind", 0, crthip_batch_bind(&s.b, 0, nullptr, nullptr, 0)); s.bind(0, CRTHIP_FMT_INT16);
	  s.normals(1); s.tangents(1); s.meshlets(1); s.bounds(1);                              // a point cloud
	  s.normals(0);                                                                           // stored normals bound
	  s.normals(2, true, CRTHIP_FMT_UINT8); s.normals(2, true, CRTHIP_FMT_FLOAT, 6);
	  s.tangents(2, true, CRTHIP_FMT_UINT8); s.tangents(2, true, CRTHIP_FMT_FLOAT, 12); s.tangents(2, true, CRTHIP_FMT_INT16, 7);
	  s.call("tangents", 2, crthip_batch_bind_computed_tangents(&s.b, 2, (void *)0x500000000002ull, CRTHIP_FMT_FLOAT, 0));
	  s.tangents(2);                                                                          // no normal source
	  { crthip_attr_binding keep = s.A(4, "uv"); s.A(4, "uv").buffer = nullptr; s.bind(4); s.tangents(4); s.A(4, "uv") = keep; }
	  { crthip_attr_binding keep = s.A(4, "uv"); s.A(4, "uv").format = CRTHIP_FMT_INT32; s.A(4, "uv").reserved = CRTHIP_BIND_STREAM_VALUES; s.bind(4); s.tangents(4); s.A(4, "uv") = keep; }
	  { crthip_attr_binding keep = s.A(4, "position"); s.A(4, "position").buffer = nullptr; s.A(4, "normal").buffer = nullptr; s.bind(4);
		s.normals(4); s.tangents(4); s.meshlets(4); s.bounds(4); s.A(4, "position") = keep; }
	  { crthip_attr_binding keep = s.A(4, "position"); s.A(4, "position").format = CRTHIP_FMT_INT32; s.A(4, "position").reserved = CRTHIP_BIND_STREAM_VALUES; s.bind(4);
		s.normals(4); s.tangents(4); s.bounds(4); s.A(4, "position") = keep; s.bind(4); }
	  s.bounds(2);                                                                            // no meshlet binding
	  { crthip_meshlet_binding m = s.meshlet_binding(2, 0, true);
		crthip_meshlet_binding x = m; x.max_vertices = 2; s.meshlets(2, &x);
		x = m; x.segment_faces = 70000; s.meshlets(2, &x);
		x = m; x.triangles = nullptr; s.meshlets(2, &x);
		x = m; x.counts = (crthip_meshlet_counts *)((uintptr_t)m.counts + 8); s.meshlets(2, &x);
		x = m; x.meshlet_capacity--; s.meshlets(2, &x);
		x = m; x.vertex_capacity--; s.meshlets(2, &x);
		x = m; x.triangle_capacity--; s.meshlets(2, &x);
		s.meshlets(2, &m); }
	  s.call("bounds", 2, crthip_batch_bind_meshlet_bounds(&s.b, 2, (crthip_meshlet_bounds *)0x500000000008ull, ~0u));
	  s.bounds(2, true, 0);
	  // check_binding through crthip_batch_bind: the flags, the formats, the alignments, the strides
	  auto refused = [&](uint32_t i, const char *a, uint32_t fmt, uint32_t stride, uint32_t flags, uint32_t oc = 0, uintptr_t skew = 0) {
		const crthip_attr_binding keep = s.A(i, a);
		crthip_attr_binding &d = s.A(i, a); d.format = fmt; d.stride = stride; d.reserved = flags; d.out_components = oc; d.buffer = (uint8_t *)d.buffer + skew;
		s.bind(i); s.A(i, a) = keep;
	  };
	  refused(3, "position", CRTHIP_FMT_FLOAT, 0, 4); refused(3, "position", CRTHIP_FMT_INT32, 0, CRTHIP_BIND_QUANTIZED); refused(3, "normal", CRTHIP_FMT_UINT16, 0, CRTHIP_BIND_QUANTIZED);
	  refused(3, "position", CRTHIP_FMT_UINT16, 0, 3); refused(3, "weights", CRTHIP_FMT_UINT16, 0, CRTHIP_BIND_QUANTIZED); refused(3, "position", CRTHIP_FMT_UINT16, 0, CRTHIP_BIND_QUANTIZED, 2);
	  refused(3, "position", CRTHIP_FMT_UINT16, 0, CRTHIP_BIND_QUANTIZED, 0, 1); refused(3, "position", CRTHIP_FMT_UINT16, 4, CRTHIP_BIND_QUANTIZED);
	  refused(3, "normal", CRTHIP_FMT_FLOAT, 0, CRTHIP_BIND_STREAM_VALUES); refused(3, "normal", CRTHIP_FMT_UINT8, 0, 0); refused(3, "normal", CRTHIP_FMT_INT16, 0, 0, 0, 1);
	  refused(3, "normal", CRTHIP_FMT_FLOAT, 8, 0); refused(3, "color", CRTHIP_FMT_FLOAT, 0, 0); refused(3, "color", CRTHIP_FMT_UINT8, 0, 0, 5); refused(3, "color", CRTHIP_FMT_UINT8, 2, 0, 4);
	  refused(3, "position", 8, 0, 0); refused(3, "position", CRTHIP_FMT_FLOAT, 4, CRTHIP_BIND_STREAM_VALUES); refused(3, "position", CRTHIP_FMT_DOUBLE, 0, 0, 0, 4);
	  refused(3, "position", CRTHIP_FMT_INT16, 12, 0); refused(3, "position", CRTHIP_FMT_FLOAT, 8, 0); refused(3, "position", CRTHIP_FMT_FLOAT, 14, 0);
	  s.call("bind_all", 0, crthip_batch_bind_all(nullptr, nullptr, nullptr, nullptr));
	  s.call("quant_transforms", 0, crthip_batch_bind_quant_transforms(&s.b, (void *)0x500000000008ull));
	  // what reads a decode's records before there was one
	  crthip_meshlet_counts mc; crthip_quant_transform qt;
	  s.call("meshlet_counts", 9, crthip_batch_meshlet_counts(&s.b, 9, &mc)); s.call("meshlet_counts", 2, crthip_batch_meshlet_counts(&s.b, 2, &mc));
	  s.call("quant_transform", 9, crthip_batch_quant_transform(&s.b, 9, 0, &qt)); s.call("quant_transform", 0, crthip_batch_quant_transform(&s.b, 0, 0, &qt));
	  s.b.decoded = true;
	  s.call("meshlet_counts", 2, crthip_batch_meshlet_counts(&s.b, 2, &mc)); s.call("quant_transform", 0, crthip_batch_quant_transform(&s.b, 0, 0, &qt));
	  Expect e; e.computed = 0; e.tangent = 0; e.meshlet = 1; e.bounds = 0; s.plan(e); }
	{ Scene s("refusals of adjacency and the weld", {B_EST, B_CLOUD, B_EST});
	  { const crthip_adjacency_binding a{}; const crthip_weld_binding w{}; s.adjacency(9, &a); s.weld(9, &w); s.adjacency(9, nullptr); s.weld(9, nullptr); }
	  s.adjacency(1); s.weld(1);                                                            // a point cloud
	  { const crthip_adjacency_binding a = s.adjacency_binding(0, true);
		crthip_adjacency_binding x = a; x.twin = nullptr; s.adjacency(0, &x);
		x = a; x.twin = (uint32_t *)((uintptr_t)a.twin + 2); s.adjacency(0, &x);
		x = a; x.counts = (crthip_adjacency_counts *)((uintptr_t)a.counts + 8); s.adjacency(0, &x);
		x = a; x.reserved = 1; s.adjacency(0, &x);
		x = a; x.capacity--; s.adjacency(0, &x); }
	  { const crthip_weld_binding w = s.weld_binding(0, true, true);
		crthip_weld_binding x = w; x.remap = nullptr; s.weld(0, &x);
		x = w; x.remap = (uint32_t *)((uintptr_t)w.remap + 2); s.weld(0, &x);
		x = w; x.index = (uint32_t *)((uintptr_t)w.index + 2); s.weld(0, &x);
		x = w; x.counts = (crthip_weld_counts *)((uintptr_t)w.counts + 8); s.weld(0, &x);
		x = w; x.remap_capacity--; s.weld(0, &x);
		x = w; x.index_capacity--; s.weld(0, &x);
		x = w; x.flags = 2; s.weld(0, &x);
		x = w; x.reserved = 1; s.weld(0, &x);
		x = w; x.index = nullptr; x.index_capacity = 0; x.flags = CRTHIP_WELD_ADJACENCY; s.weld(0, &x); }
	  { crthip_attr_binding keep = s.A(2, "position"); s.A(2, "position").buffer = nullptr; s.A(2, "normal").buffer = nullptr; s.bind(2); s.weld(2); s.adjacency(2); s.A(2, "position") = keep; }
	  { crthip_attr_binding keep = s.A(2, "position"); s.A(2, "position").format = CRTHIP_FMT_INT32; s.A(2, "position").reserved = CRTHIP_BIND_STREAM_VALUES; s.bind(2); s.weld(2); s.adjacency(2); s.A(2, "position") = keep; }
	  Expect e; e.adjacency = 1; e.weld = 0; s.plan(e); }                                   // (adjacency needs no attribute: blob 2 keeps the one call that was taken)
	{ Scene s("bind_all", small);
	  std::vector<crthip_attr_binding> flat; std::vector<uint32_t> fmt;
	  for(uint32_t i = 0; i < small.size(); i++) { flat.insert(flat.end(), s.at[i].begin(), s.at[i].end()); fmt.push_back(i & 1 ? CRTHIP_FMT_UINT16 : CRTHIP_FMT_UINT32); }
	  s.tangents(0);
	  s.call("bind_all", 0, crthip_batch_bind_all(&s.b, flat.data(), s.index.data(), fmt.data()));
	  s.plan(none); }
}

int main(int argc, char **argv) {
	if(argc < 2) { fprintf(stderr, "usage: plan_dump corpus.bin [--dump FILE]\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	uint32_t n = 0;
	if(!f || fread(&n, 4, 1, f) != 1 || n != B_COUNT) { fprintf(stderr, "plan_dump: %s is not a corpus of %d blobs\n", argv[1], (int)B_COUNT); return 2; }
	for(uint32_t i = 0; i < n; i++) {
		Blob bl;
		if(fread(&bl.len, 4, 1, f) != 1) return 2;
		bl.words.assign(((size_t)bl.len + 3)/4 + 4, 0u);
		if(fread(bl.words.data(), 1, bl.len, f) != bl.len) return 2;
		corpus.push_back(std::move(bl));
	}
	fclose(f);
	if(argc >= 4 && !strcmp(argv[2], "--dump")) { dump = fopen(argv[3], "w"); if(!dump) return 2; }
	scenarios();
	if(dump) fclose(dump);
	if(nfailed) { printf("plan_dump: %d checks failed\n", nfailed); return 1; }
	printf("plan_dump ok: %d scenarios, %d array records\n", nscenes, narrays);
	return 0;
}
