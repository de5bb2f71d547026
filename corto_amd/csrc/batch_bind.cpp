// batch_bind.cpp — what a caller binds to a batch's blobs and what reads a decode's records back: crthip_batch_bind / _bind_all, the ten derived
// outputs (computed normals, computed tangents, meshlets, meshlet bounds, adjacency, weld, levels of detail of meshes and of clouds, compaction, BVH: DerivedBindings, batch_internal.h), the quantised attributes' records and the
// meshlet counts.  Every check of a binding is made here, in the order corto_hip.h lists its errors, so that a decode has nothing new to fail on.
// No HIP call: a program without the runtime links these (tests/cpp/plan_dump.cpp).
#include "batch_internal.h"

static int check_binding(const AttrHeader &a, const crthip_attr_binding &bd) {
	if(!bd.buffer) return CRTHIP_OK;
	const uint32_t st = bd.stride;
	if(bd.reserved & ~(CRTHIP_BIND_STREAM_VALUES | CRTHIP_BIND_QUANTIZED)) return CRTHIP_E_ARGUMENT;
	if(bd.reserved & CRTHIP_BIND_QUANTIZED) {                              // uint16 grid values of a generic attribute (corto_hip.h)
		// (INT32 is the format of the OTHER flag's stream values: with this bit it stays the argument error it was before the bit had a meaning)
		if(a.codec == CRTHIP_CODEC_GENERIC && bd.format == CRTHIP_FMT_INT32) return CRTHIP_E_ARGUMENT;
		if(a.codec == CRTHIP_CODEC_NORMAL || a.codec == CRTHIP_CODEC_COLOR || bd.format != CRTHIP_FMT_UINT16 || a.N < 1) return CRTHIP_E_FORMAT;
		if(bd.reserved & CRTHIP_BIND_STREAM_VALUES) return CRTHIP_E_ARGUMENT;
		if(a.N > 4) return CRTHIP_E_LIMIT;
		if(bd.out_components && bd.out_components != a.N) return CRTHIP_E_ARGUMENT;
		if(((uintptr_t)bd.buffer) % 2) return CRTHIP_E_ARGUMENT;
		if(st && (st < 2*a.N || st % 2)) return CRTHIP_E_ARGUMENT;
		return CRTHIP_OK;
	}
	if((bd.reserved & CRTHIP_BIND_STREAM_VALUES) && a.codec != CRTHIP_CODEC_GENERIC) return CRTHIP_E_FORMAT;   // normals / colours have codecs of their own upstream too
	if(a.codec == CRTHIP_CODEC_NORMAL) {
		if(bd.format != CRTHIP_FMT_FLOAT && bd.format != CRTHIP_FMT_INT16) return CRTHIP_E_FORMAT;
		const uint32_t el = bd.format == CRTHIP_FMT_INT16 ? 2u : 4u;
		if(((uintptr_t)bd.buffer) % el) return CRTHIP_E_ARGUMENT;            // a float* / int16_t* (decoder.h:52-53) is aligned by its type
		if(st && (st < 3*el || st % el)) return CRTHIP_E_ARGUMENT;
		return CRTHIP_OK;
	}
	if(a.codec == CRTHIP_CODEC_COLOR) {
		// FLOAT colour output is broken upstream (color_attribute.cpp:96-110)
		if(bd.format != CRTHIP_FMT_UINT8) return CRTHIP_E_FORMAT;
		uint32_t oc = bd.out_components ? bd.out_components : 4;
		if(a.N < 1 || a.N > 4 || oc > 4 || oc < a.N) return CRTHIP_E_FORMAT;
		if(st && st < oc) return CRTHIP_E_ARGUMENT;
		return CRTHIP_OK;
	}
	if(a.N < 1 || bd.format > CRTHIP_FMT_DOUBLE) return CRTHIP_E_FORMAT;
	// the device half of a caller-supplied codec object: int32 stream values, packed (corto_hip.h: CRTHIP_BIND_STREAM_VALUES)
	if(bd.reserved & CRTHIP_BIND_STREAM_VALUES) return bd.format == CRTHIP_FMT_INT32 && !st && ((uintptr_t)bd.buffer) % 4 == 0 ? CRTHIP_OK : CRTHIP_E_ARGUMENT;
	// a packed buffer doubles as the int32 workspace and K-DELTA turns it into floats with dword / 16-byte accesses: a float* that is
	// not 4-byte aligned (never one a C++ caller's setPositions(float*) could pass) is refused, not decoded into integers
	if(((uintptr_t)bd.buffer) % (bd.format == CRTHIP_FMT_DOUBLE ? 8 : 4)) return CRTHIP_E_ARGUMENT;
	// the integer formats and DOUBLE (setAttribute(name, buffer, format): vertex_attribute.h:195-228) are upstream's in-place layouts:
	// packed only
	if(bd.format != CRTHIP_FMT_FLOAT) return st ? CRTHIP_E_ARGUMENT : CRTHIP_OK;
	if(st && (st < 4*a.N || st % 4)) return CRTHIP_E_ARGUMENT;
	return CRTHIP_OK;
}

extern "C" int crthip_batch_bind(crthip_batch *b, uint32_t i, const crthip_attr_binding *attrs, void *index, uint32_t index_format) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT);
	BlobPlan &P = b->blobs[i];
	if(P.bind.size() && !attrs) return fail(CRTHIP_E_ARGUMENT);
	if(index && index_format != CRTHIP_FMT_UINT32 && index_format != CRTHIP_FMT_UINT16) return fail(CRTHIP_E_FORMAT);
	for(size_t k = 0; k < P.bind.size(); k++) {
		int err = check_binding(P.L.h.attrs[k], attrs[k]);
		if(err) return fail(err, std::string(crthip_strerror(err)) + " (attribute '" + P.L.h.attrs[k].name + "')");
	}
	for(size_t k = 0; k < P.bind.size(); k++) {
		P.bind[k].buffer = attrs[k].buffer; P.bind[k].format = attrs[k].format;
		P.bind[k].out_components = attrs[k].out_components ? attrs[k].out_components : 4;
		// a stride equal to the packed element size is the packed layout (the buffer then doubles as int32 workspace, as upstream's does)
		const AttrHeader &a = P.L.h.attrs[k];
		P.bind[k].stream_values = (attrs[k].reserved & CRTHIP_BIND_STREAM_VALUES) != 0;
		P.bind[k].quantized = attrs[k].buffer && (attrs[k].reserved & CRTHIP_BIND_QUANTIZED) != 0;
		const uint32_t packed = a.codec == CRTHIP_CODEC_NORMAL ? (attrs[k].format == CRTHIP_FMT_INT16 ? 6u : 12u)
		                      : a.codec == CRTHIP_CODEC_COLOR ? P.bind[k].out_components : P.bind[k].quantized ? 2u*a.N : 4u*a.N;
		P.bind[k].stride = attrs[k].stride == packed ? 0u : attrs[k].stride;
	}
	P.index = index; P.index_u16 = index && index_format == CRTHIP_FMT_UINT16;
	P.derived.clear();                                                      // (the derived outputs are bound behind the bind)
	b->dirty = true;
	return CRTHIP_OK;
}

// Normals for a mesh whose blob stores none (or leaves its stored ones unbound): every check is made here, so that the decode has nothing new to fail on
extern "C" int crthip_batch_bind_computed_normals(crthip_batch *b, uint32_t i, void *buffer, uint32_t format, uint32_t stride) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_computed_normals: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	P.derived.normals_change();                                           // (the tangents are bound behind this call)
	if(!buffer) { P.derived.normals = Binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "computed normals need faces: a point cloud has none" + who);
	// (whatever its codec: not tangent_normal_source's test)
	for(size_t k = 0; k < P.bind.size(); k++)
		if(P.L.h.attrs[k].name == "normal" && P.bind[k].buffer) return fail(CRTHIP_E_ARGUMENT, "the blob's stored normals are bound: computed normals take an unbound or absent attribute" + who);
	// what a stored normal's binding must be (check_binding)
	AttrHeader as_normal; as_normal.codec = CRTHIP_CODEC_NORMAL;
	crthip_attr_binding bd{};
	bd.buffer = buffer; bd.format = format; bd.stride = stride;
	const int err = check_binding(as_normal, bd);
	if(err) return fail(err, std::string(crthip_strerror(err)) + " (computed normals)" + who);
	// ... and what a stored ESTIMATED normal asks of the position (plan_jobs.cpp; src/normal_attribute.cpp:210-227)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "computed normals need a bound three-component \"position\" (bind the blob first)" + who);
	Binding &out = P.derived.normals;
	out.buffer = buffer; out.format = format;
	out.stride = stride == (format == CRTHIP_FMT_INT16 ? 6u : 12u) ? 0u : stride;
	b->dirty = true;
	return CRTHIP_OK;
}

// Tangents from the blob's integer positions and uvs, its index and its final normals (corto_hip.h has the value): every check is made here
extern "C" int crthip_batch_bind_computed_tangents(crthip_batch *b, uint32_t i, void *buffer, uint32_t format, uint32_t stride) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_computed_tangents: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!buffer) { P.derived.tangents_change(); P.derived.tangents = Binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "computed tangents need faces: a point cloud has none" + who);
	if(format != CRTHIP_FMT_FLOAT && format != CRTHIP_FMT_INT16) return fail(CRTHIP_E_FORMAT, "computed tangents are FLOAT or INT16" + who);
	const uint32_t el = format == CRTHIP_FMT_INT16 ? 2u : 4u;
	if(((uintptr_t)buffer) % el || (stride && (stride < 4*el || stride % el)))
		return fail(CRTHIP_E_ARGUMENT, "computed tangents: the buffer is not aligned to its element, or the stride is below four elements or no multiple of one" + who);
	// (what computed normals ask of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "computed tangents need a bound three-component \"position\" (bind the blob first)" + who);
	if(!generic_source_ok(P, attr_named(P, "uv"), 2))
		return fail(CRTHIP_E_ARGUMENT, "computed tangents need a bound two-component generic \"uv\" (bind the blob first)" + who);
	if(!tangent_normal_source(P))
		return fail(CRTHIP_E_ARGUMENT, "computed tangents need a normal source: a stored \"normal\" bound as FLOAT or INT16, or crthip_batch_bind_computed_normals before this call" + who);
	P.derived.tangents_change();                                          // (a compaction that gathers the tangents is bound behind this call)
	Binding &out = P.derived.tangents;
	out.buffer = buffer; out.format = format; out.out_components = 4;
	out.stride = stride == 4*el ? 0u : stride;
	b->dirty = true;
	return CRTHIP_OK;
}

// Meshlets from the blob's decoded index (corto_hip.h has the contract): every check is made here, against the bound of this blob's index
extern "C" int crthip_batch_bind_meshlets(crthip_batch *b, uint32_t i, const crthip_meshlet_binding *m) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_meshlets: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	P.derived.meshlets_change();                                          // (the bounds are bound behind this call)
	if(!m) { P.derived.meshlets = crthip_meshlet_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "meshlets need faces: a point cloud has none" + who);
	crthip_meshlet_counts bound;
	const bool ok = mlt_plan_of(P, *m, nullptr, bound);
	if(const char *why = meshlet_binding_error(m, ok, bound)) return fail(CRTHIP_E_ARGUMENT, why + who);
	P.derived.meshlets = *m;
	b->dirty = true;
	return CRTHIP_OK;
}

// A box, a sphere and a normal cone a meshlet (corto_hip.h has the record): every check is made here, against the meshlet binding of this blob
extern "C" int crthip_batch_bind_meshlet_bounds(crthip_batch *b, uint32_t i, crthip_meshlet_bounds *bounds, uint32_t capacity) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_meshlet_bounds: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!bounds) { P.derived.bounds = nullptr; b->dirty = true; return CRTHIP_OK; }
	if(!builds_meshlets(P)) return fail(CRTHIP_E_ARGUMENT, "meshlet bounds need a meshlet binding: crthip_batch_bind_meshlets comes first" + who);
	if((uintptr_t)bounds % 16) return fail(CRTHIP_E_ARGUMENT, "meshlet bounds: the records are 16-byte aligned" + who);
	crthip_meshlet_counts bound;
	if(!mlt_plan_of(P, P.derived.meshlets, nullptr, bound) || capacity < bound.meshlets)
		return fail(CRTHIP_E_ARGUMENT, "meshlet bounds: capacity is below crthip_meshlet_bound's meshlets" + who);
	// (what computed tangents ask of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "meshlet bounds need a bound three-component \"position\" (bind the blob first)" + who);
	P.derived.bounds = bounds;
	b->dirty = true;
	return CRTHIP_OK;
}

// The half-edge twins of the blob's decoded index (corto_hip.h has the contract): every check is made here, in the header's order.  It reads the
// index alone, so no other derived binding drops it and it drops none
extern "C" int crthip_batch_bind_adjacency(crthip_batch *b, uint32_t i, const crthip_adjacency_binding *a) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_adjacency: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!a) { P.derived.adjacency = crthip_adjacency_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "adjacency needs faces: a point cloud has none" + who);
	if(const char *why = adjacency_binding_error(a, P.L.h.nface)) return fail(CRTHIP_E_ARGUMENT, why + who);
	P.derived.adjacency = *a;
	b->dirty = true;
	return CRTHIP_OK;
}

// The weld map of the blob's integer positions and its welded index (corto_hip.h has the contract): every check is made here, in the header's
// order.  It reads what the bind binds, like every derived binding; no other derived binding drops it and it drops none (CRTHIP_WELD_ADJACENCY is
// looked at when a decode is planned)
extern "C" int crthip_batch_bind_weld(crthip_batch *b, uint32_t i, const crthip_weld_binding *w) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_weld: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!w) { P.derived.source_change(CRTHIP_COMPACT_WELD); P.derived.weld = crthip_weld_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "a weld needs faces: a point cloud has none" + who);
	if(const char *why = weld_binding_error(w, P.L.h.nvert, P.L.h.nface)) return fail(CRTHIP_E_ARGUMENT, why + who);
	// (what meshlet bounds ask of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "a weld needs a bound three-component \"position\" (bind the blob first)" + who);
	P.derived.source_change(CRTHIP_COMPACT_WELD);                         // (a compaction of the welded index is bound behind this call)
	P.derived.weld = *w;
	b->dirty = true;
	return CRTHIP_OK;
}

// Clustered levels of detail of the blob's index (corto_hip.h has the contract): every check is made here, in the header's order.  It reads what
// the bind binds, like every derived binding; no other derived binding drops it and it drops none
extern "C" int crthip_batch_bind_lod(crthip_batch *b, uint32_t i, const crthip_lod_binding *l) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_lod: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!l) { P.derived.source_change(CRTHIP_COMPACT_LOD); P.derived.lod = crthip_lod_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "levels of detail need faces: a point cloud has none" + who);
	if(const char *why = lod_binding_error(l, P.L.h.nvert, P.L.h.nface)) return fail(CRTHIP_E_ARGUMENT, why + who);
	// (what the weld asks of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "levels of detail need a bound three-component \"position\" (bind the blob first)" + who);
	P.derived.source_change(CRTHIP_COMPACT_LOD);                          // (a compaction of a level is bound behind this call)
	P.derived.lod = *l;
	b->dirty = true;
	return CRTHIP_OK;
}

// Levels of detail of a point cloud (corto_hip.h has the contract): every check is made here, in the header's order.  It reads what the bind
// binds, like every derived binding; no other derived binding drops it and it drops none
extern "C" int crthip_batch_bind_cloud_lod(crthip_batch *b, uint32_t i, const crthip_cloud_lod_binding *l) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_cloud_lod: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!l) { P.derived.source_change(CRTHIP_COMPACT_CLOUD_LOD); P.derived.cloud_lod = crthip_cloud_lod_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface > 0) return fail(CRTHIP_E_ARGUMENT, "a cloud's levels of detail: the blob has faces, it is not a point cloud" + who);
	if(P.L.h.nvert == 0) return fail(CRTHIP_E_ARGUMENT, "a cloud's levels of detail: the cloud has no points" + who);
	if(const char *why = cloud_lod_binding_error(l, P.L.h.nvert)) return fail(CRTHIP_E_ARGUMENT, why + who);
	// (what the weld asks of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "a cloud's levels of detail need a bound three-component \"position\" (bind the blob first)" + who);
	P.derived.source_change(CRTHIP_COMPACT_CLOUD_LOD);                    // (a compaction of a level is bound behind this call)
	P.derived.cloud_lod = *l;
	b->dirty = true;
	return CRTHIP_OK;
}

// Compaction (corto_hip.h has the contract): what a binding on blob P is refused for, in the header's order behind "no such blob"; CRTHIP_OK: fine.
// The planner asks again (compact_jobs), so that a decode has nothing new to fail on
int compact_binding_error(const BlobPlan &P, const crthip_compact_binding *c, std::string &why) {
	if(c->sets < 1 || c->sets > CRTHIP_COMPACT_MAX_SETS) { why = "compact: sets is not in 1..CRTHIP_COMPACT_MAX_SETS"; return CRTHIP_E_ARGUMENT; }
	if(c->flags) { why = "compact: unknown flag bits"; return CRTHIP_E_ARGUMENT; }
	if(c->reserved[0] || c->reserved[1]) { why = "compact: reserved is not 0"; return CRTHIP_E_ARGUMENT; }
	const bool mesh = P.L.h.nface > 0;
	const uint32_t nvert = P.L.h.nvert;
	for(uint32_t s = 0; s < c->sets; s++) {
		const crthip_compact_set &t = c->set[s];
		const std::string set = "compact, set " + std::to_string(s) + ": ";
		auto bad = [&](const char *m) { why = set + m; return CRTHIP_E_ARGUMENT; };
		if(t.source > CRTHIP_COMPACT_CLOUD_LOD) return bad("an unknown source");
		if(t.reserved[0] || t.reserved[1]) return bad("reserved is not 0");
		const bool cloud = t.source == CRTHIP_COMPACT_CLOUD_LOD;
		if(cloud && mesh) return bad("the cloud source on a mesh");
		if(!cloud && !mesh) return bad("a mesh source on a point cloud");
		if(t.source == CRTHIP_COMPACT_WELD && !(binds_weld(P) && P.derived.weld.index)) return bad("the blob has no weld binding with an index");
		if(t.source == CRTHIP_COMPACT_LOD && !(binds_lod(P) && t.level < P.derived.lod.levels)) return bad("the blob's lod binding has no such level");
		if(cloud && !(binds_cloud_lod(P) && t.level < P.derived.cloud_lod.levels)) return bad("the blob's cloud lod binding has no such level");
		if(cloud && (t.newid || t.order || t.index)) return bad("a cloud source takes no newid, order or index");
		if((uintptr_t)t.newid % 4 || (uintptr_t)t.order % 4 || (uintptr_t)t.index % 4) return bad("newid, order or index is not 4-byte aligned");
		if((uintptr_t)t.counts % 16) return bad("counts is not 16-byte aligned");
		if(t.newid && t.newid_capacity < nvert) return bad("newid_capacity is below nvert");
		if(t.ngather > CRTHIP_COMPACT_MAX_GATHERS) return bad("ngather is above CRTHIP_COMPACT_MAX_GATHERS");
		for(uint32_t q = 0; q < t.ngather; q++) {
			const crthip_compact_gather &g = t.gather[q];
			const std::string gather = set + "gather " + std::to_string(q) + ": ";
			const CompactSource src = compact_source_of(P, g.source);
			if(src.err) { why = gather + src.why; return src.err; }
			if(!g.dst || (uintptr_t)g.dst % src.A) { why = gather + "dst is NULL or not aligned to the source's element"; return CRTHIP_E_ARGUMENT; }
			if(g.dst_stride && (g.dst_stride < src.E || g.dst_stride % src.A)) { why = gather + "dst_stride is below the element size or no multiple of its alignment"; return CRTHIP_E_ARGUMENT; }
		}
	}
	return CRTHIP_OK;
}

// Every check is made here, in the header's order.  The binding reads other bindings' outputs: a later call that changes one of them drops it
// (DerivedBindings::source_change, normals_change, tangents_change), and it drops none
extern "C" int crthip_batch_bind_compact(crthip_batch *b, uint32_t i, const crthip_compact_binding *c) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_compact: no such blob");
	BlobPlan &P = b->blobs[i];
	if(!c) { P.derived.compact = crthip_compact_binding{}; b->dirty = true; return CRTHIP_OK; }
	std::string why;
	if(const int err = compact_binding_error(P, c, why)) return fail(err, why + " (blob " + std::to_string(i) + ")");
	P.derived.compact = *c;
	b->dirty = true;
	return CRTHIP_OK;
}

// The BVH (corto_hip.h has the contract).  Every check is made here, in the header's order; it reads no other binding's output and no other
// binding reads its own, so no later call but a bind of the blob or a reset drops it
extern "C" int crthip_batch_bind_bvh(crthip_batch *b, uint32_t i, const crthip_bvh_binding *v) {
	if(!b || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_bvh: no such blob");
	BlobPlan &P = b->blobs[i];
	const std::string who = " (blob " + std::to_string(i) + ")";
	if(!v) { P.derived.bvh = crthip_bvh_binding{}; b->dirty = true; return CRTHIP_OK; }
	if(P.L.h.nface == 0) return fail(CRTHIP_E_ARGUMENT, "a BVH needs faces: a point cloud has none" + who);
	if(const char *why = bvh_binding_error(v, P.L.h.nface)) return fail(CRTHIP_E_ARGUMENT, why + who);
	// (what the weld asks of the position)
	if(!generic_source_ok(P, attr_named(P, "position"), 3))
		return fail(CRTHIP_E_NORMAL_NEEDS_POSITION, "a BVH needs a bound three-component \"position\" (bind the blob first)" + who);
	P.derived.bvh = *v;
	b->dirty = true;
	return CRTHIP_OK;
}

// a decode's records are read only behind its sync
static bool records_ready(const crthip_batch *b) { return b->decoded && !(b->ctx && b->ctx->in_flight == b) && !b->staged; }

extern "C" int crthip_batch_meshlet_counts(const crthip_batch *b, uint32_t i, crthip_meshlet_counts *out) {
	if(!b || !out || i >= b->blobs.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_meshlet_counts: no such blob");
	if(!records_ready(b)) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_meshlet_counts: decode and sync the batch first");
	if(i >= b->meshlet_bound.size() || i >= b->meshlet_recs.size() || !b->meshlet_bound[i])
		return fail(CRTHIP_E_ARGUMENT, "crthip_batch_meshlet_counts: the blob had no meshlet binding in that decode (blob " + std::to_string(i) + ")");
	*out = b->meshlet_recs[i];
	return CRTHIP_OK;
}

// CRTHIP_BIND_QUANTIZED: the record of one attribute as the last synced decode left it; the caller's device copy of the records
extern "C" int crthip_batch_quant_transform(const crthip_batch *b, uint32_t i, uint32_t attr, crthip_quant_transform *out) {
	if(!b || !out || i >= b->blobs.size() || attr >= b->blobs[i].bind.size()) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_quant_transform: no such blob or attribute");
	if(!records_ready(b)) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_quant_transform: decode and sync the batch first");
	size_t r = attr;
	for(uint32_t k = 0; k < i; k++) r += b->blobs[k].bind.size();
	if(r >= b->quant_bound.size() || r >= b->quant_recs.size() || !b->quant_bound[r])
		return fail(CRTHIP_E_ARGUMENT, "crthip_batch_quant_transform: the attribute was not bound with CRTHIP_BIND_QUANTIZED (blob " + std::to_string(i) + ")");
	*out = b->quant_recs[r];
	return CRTHIP_OK;
}

extern "C" int crthip_batch_bind_quant_transforms(crthip_batch *b, void *device_records) {
	if(!b) return fail(CRTHIP_E_ARGUMENT);
	if((uintptr_t)device_records & 15) return fail(CRTHIP_E_ARGUMENT, "crthip_batch_bind_quant_transforms: the record array must be 16-byte aligned");
	b->quant_dev = device_records;
	b->dirty = true;
	return CRTHIP_OK;
}

extern "C" int crthip_batch_bind_all(crthip_batch *b, const crthip_attr_binding *attrs, void *const *index, const uint32_t *index_format) {
	if(!b) return fail(CRTHIP_E_ARGUMENT);
	size_t k = 0;
	for(uint32_t i = 0; i < b->blobs.size(); i++) {
		int err = crthip_batch_bind(b, i, attrs ? attrs + k : nullptr, index ? index[i] : nullptr, index_format ? index_format[i] :
			CRTHIP_FMT_UINT32);
		if(err) return err;
		k += b->blobs[i].bind.size();
	}
	return CRTHIP_OK;
}
