// plan_launch.cpp — Planner::launch / account: the schedule's shape, the kernels enqueued stage by stage in the order of crt::Decoder::decodeMesh /
// decodePointCloud (src/decoder.cpp:133-196), crthip_batch_stats filled.  (Planner::upload: plan_group.cpp)
#include "batch_internal.h"

// The schedule has two stages (batch_internal.h: PH_*).  Stage E - the descriptor copy, the zeroing, K-TAB, K-STREAM, k_fill - reads the batch's arena and
// descriptors and writes only the batch's own scratch; stage M is everything behind it and writes the caller's outputs and the status words.
// crthip_batch_decode runs both in one call.  crthip_batch_decode_with_next runs stage M of one batch with stage E of the lane's next batch:
// as launches of its own (PH_TUN), or - `carry`, the next batch's K-TAB / K-STREAM arguments - inside this batch's k_front / k_delta_lds16 grids.
Planner::Shape Planner::shape() const {
	if(pl.tun_multi_chunk) return Shape::LongStreams;
	const bool attr_work = pl.tun.v.size() > clers_tun || pl.fill.v.size() > clers_fill || unpack_chunks || !pl.unpack_wave_ids.v.empty();
	return !pl.topo.v.empty() && attr_work && !ctx->single_stream ? Shape::Forked : Shape::OneStream;
}
// one stream: the automata and the attributes' bit-unpack in one grid (k_front) when the batch has nothing else for either -
// no big or HBM-front automaton, no chunked K-BIT - and the automata ask for little LDS (K-BIT's waves hold the same request)
bool Planner::takes_front() const {
	return shape() == Shape::OneStream && ctx->single_stream && !ctx->dbg.front_off && !pl.topo_lds_ids.v.empty() && !pl.unpack_wave_ids.v.empty() &&
		pl.topo_big_ids.v.empty() && pl.topo_glob_ids.v.empty() && !unpack_chunks && pl.topo_lds <= FRONT_LDS_MAX;
}
// every stream of the batch through shared dictionaries of up to 64 symbols, in one K-TAB and one K-STREAM launch: what another batch's grids can carry
bool Planner::carry_args(Carry &c) const {
	const uint32_t ntun = (uint32_t)pl.tun.v.size(), ndict = (uint32_t)pl.tun_dict.v.size(), ngroups = (uint32_t)pl.tun_groups.v.size();
	if(ctx->dbg.carry_off || !ctx->single_stream || !splits() || !ntun || !ndict || !ngroups) return false;
	if((clers_tun > 0 && !share_clers) || (ntun > clers_tun && !share_attrs)) return false;
	for(const TunStream &d : pl.tun_dict.v) if(d.nsym > 64) return false;
	// a carried dictionary holds k_front's LDS request (~10 KB) for its ~45 us beside other lanes' automata, which wait for LDS to come free: the ~250
	// distinct tables of a batch whose blobs repeat one another's add 0.1 GB.us to the ~2.4 the step holds, a dictionary PER STREAM (2 304 a batch,
	// $CORTO_TUN_SHARE=2) 1 GB.us - measured 10 % slower than not carrying (profiles/pool_carry.md)
	if(ndict > TUN_CARRY_DICTS_MAX) return false;
	c.dicts = (const TunStream *)(base + pl.tun_dict.dev_off); c.ndicts = ndict; c.tables = (TunTable *)(base + pl.tables_off);
	c.streams = (const TunStream *)(base + pl.tun.dev_off); c.ids = (const uint32_t *)(base + pl.tun_group_ids.dev_off);
	c.groups = (const TunGroup *)(base + pl.tun_groups.dev_off); c.ngroups = ngroups;
	return true;
}
// ... and a batch whose grids can carry them: k_front with room for the dictionaries' growth state in the automata's LDS request, and k_delta_lds16
bool Planner::hosts_carry() const {
	return !ctx->dbg.carry_off && takes_front() && pl.topo_lds >= TUN_CARRY_GROW_LDS && !pl.delta.v.empty() && !pl.delta_groups.v.empty();
}

int tun_chain(Launch &LT, hipStream_t st, const std::vector<TunStream> &tun, const TunStream *streams, const uint32_t *chunk_stream, uint32_t chunks,
	TunTable *tables, uint64_t *partial, uint32_t max_nchunks, bool multi, const FillJob *fill, uint32_t nfill) {
	const uint32_t ntun = (uint32_t)tun.size();
	if(ntun) {
		// (an alphabet of more than 64 symbols builds its words in LDS: tun_tables.h)
		uint32_t big = 0;
		for(auto &t : tun) if(t.nsym > 64) big = TUN_TABLE_BYTES;
		LT.run("tunstall_tables", k_tun_tables, dim3(ntun), dim3(64), big, st, streams, ntun, tables);
		// (up to 256 chunks a stream: every decode wave adds up the sums in front of it itself; longer streams: one workgroup per stream
		// scans them)
		const bool scanned = max_nchunks > 256;
		if(multi) LT.run("tunstall_chunk_sums", k_tun_chunk_sums, dim3(chunks), dim3(256), 0, st, streams, chunk_stream, chunks, tables, partial, 0u);
		if(multi && scanned) LT.run("tunstall_stream_scan", k_tun_stream_scan, dim3(ntun), dim3(256), 0, st, streams, ntun, partial);
		LT.begin("tunstall_decode", st);
		if(multi) { if(launch_tun_decode_staged(st, streams, chunk_stream, chunks, tables, partial, scanned ? 0u : 1u)) return fail(CRTHIP_E_DEVICE); }
		else hipLaunchKernelGGL(k_tun_decode, dim3(chunks), dim3(256), 0, st, streams, chunk_stream, chunks, tables, partial, 0u);
		LT.end();
	}
	if(nfill) LT.run("fill", k_fill, dim3(nfill), dim3(256), 0, st, fill, nfill);
	return CRTHIP_OK;
}

// the attribute streams' side of a fork: the context's second stream behind everything on the main one so far, and the main one behind it again
int Planner::fork(hipStream_t *s2) {
	{ int e_ = ctx_stream2(ctx, s2); if(e_) return e_; }
	HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
	HIP_TRY(hipStreamWaitEvent(*s2, ctx->ev_fork, 0));
	return CRTHIP_OK;
}
int Planner::join(hipStream_t s2) {
	HIP_TRY(hipEventRecord(ctx->ev_join, s2));
	HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
	return CRTHIP_OK;
}

// K-TAB / K-STREAM of the streams [t0, t1) and k_fill of the fills [f0, f1): every stream here is one chunk, one wave per stream
void Planner::entropy(hipStream_t s, uint32_t phases, uint32_t t0, uint32_t t1, uint32_t f0, uint32_t f1) {
	const uint32_t ntun = (uint32_t)pl.tun.v.size(), ndict = (uint32_t)pl.tun_dict.v.size();
	if(t1 > t0 && (phases & PH_TUN)) {
		// [t0, t1) is the CLERS streams, the attribute streams, or both (dictionaries are numbered the same way)
		const bool has_clers = t0 == 0 && clers_tun > 0, has_attrs = t1 == ntun && ntun > clers_tun;
		const bool share = (!has_clers || share_clers) && (!has_attrs || share_attrs) && (has_clers || has_attrs);
		// distinct tables first, then every stream decodes from its (shared) dictionary
		if(share) {
			const uint32_t d0 = has_clers ? 0u : clers_dict, d1 = has_attrs ? ndict : clers_dict;
			// (an alphabet of more than 64 symbols builds its words in LDS: tun_tables.h)
			uint32_t big = 0;
			for(uint32_t d = d0; d < d1; d++) if(pl.tun_dict.v[d].nsym > 64) big = TUN_TABLE_BYTES;
			TunTable *tables = (TunTable *)(base + pl.tables_off);
			LT.run("tunstall_tables", k_tun_tables, dim3(d1 - d0), dim3(64), big, s, D(pl.tun_dict) + d0, d1 - d0, tables);
			const uint32_t g0 = has_clers ? 0u : pl.clers_groups, g1 = has_attrs ? (uint32_t)pl.tun_groups.v.size() : pl.clers_groups;
			LT.run("tunstall_stream", k_tun_stream_grouped, dim3(g1 - g0), dim3(256), 0, s, D(pl.tun), D(pl.tun_group_ids), D(pl.tun_groups) + g0, g1 - g0, tables);
		} else LT.run("tunstall_stream", k_tun_stream, dim3(t1 - t0), dim3(64), 0, s, D(pl.tun) + t0, t1 - t0);   // dictionary + decode in one kernel
	}
	if(f1 > f0 && (phases & PH_FILL)) LT.run("fill", k_fill, dim3(f1 - f0), dim3(256), 0, s, D(pl.fill) + f0, f1 - f0);
}
void Planner::unpack(hipStream_t s) {
	const uint32_t nuw = (uint32_t)pl.unpack_wave_ids.v.size();
	if(nuw) LT.run("unpack_wave", k_unpack_wave, dim3(xcd_grid(nuw)), dim3(64), 0, s, D(pl.unpack), D(pl.unpack_wave_ids), nuw);
	if(unpack_chunks) LT.run("unpack_extract", k_unpack_extract, dim3(unpack_chunks), dim3(256), 0, s, D(pl.unpack), D(pl.unpack_chunk_job), unpack_chunks,
		(uint64_t *)(base + pl.unpack_partial_off));
}
// the automata: the two LDS size classes under one record, then those on the HBM front
void Planner::topology() {
	hipStream_t st = ctx->stream;
	if(!pl.topo_lds_ids.v.empty() || !pl.topo_big_ids.v.empty()) {
		const uint32_t nbg = (uint32_t)pl.topo_big_ids.v.size(), nl = (uint32_t)pl.topo_lds_ids.v.size();
		LT.begin("topology_lds");
		if(nbg) hipLaunchKernelGGL(k_topology_lds_big, dim3(nbg), dim3(64), pl.topo_big_lds, st, D(pl.topo), D(pl.topo_big_ids), nbg);
		if(nl) hipLaunchKernelGGL(k_topology_lds, dim3(nl), dim3(64), pl.topo_lds, st, D(pl.topo), D(pl.topo_lds_ids), nl);
		LT.end();
	}
	by_ids("topology", k_topology, 64, 0, pl.topo, pl.topo_glob_ids);
}
// K-DELTA's big jobs in tiles of 1 024 vertices (k_delta_tiles).  On a lone context this goes to the SECOND stream, behind the attribute streams' bit-unpack
// and BESIDE the automaton, whose progress word the tiles wait for: a single big mesh's delta inversion trails its topology instead of following it
// (config C2: 1.5 of 4.0 ms).  The automaton is enqueued first on its own stream and waits for nothing of this kernel.
// BESIDE the automaton only a handful of workgroups: they hold 66 KB of LDS each while they wait, and a batch of hundreds of big meshes' tiles, resident
// first, could keep the automata (up to 156 KB a workgroup) from ever finding a CU - the tiles would wait for a progress word nobody can write.  Up to 48
// (sixteen big meshes' three attributes; a slice of an attribute of more than four components counts as one) leave most of the chip free; more run
// behind the automaton as on a pool context.
constexpr uint32_t TILES_BESIDE_MAX = 48;
void Planner::delta_tiles(hipStream_t s) {
	if(!nbig) return;
	if(s != ctx->stream && nbig > TILES_BESIDE_MAX) return;
	LT.begin("delta_tiles", s);
	if(nbig > nslices) hipLaunchKernelGGL(k_delta_tiles<false>, dim3(nbig - nslices), dim3(DELTA_THREADS), 0, s, D(pl.delta), nbig - nslices);
	if(nslices) hipLaunchKernelGGL(k_delta_tiles<true>, dim3(nslices), dim3(DELTA_THREADS), 0, s, D(pl.delta) + (nbig - nslices), nslices);
	LT.end();
	tiles_launched = true;
}
// long streams (scaled Tunstall runs, very large meshes): chunk offsets need one scan over all chunks; single stream
int Planner::long_streams() {
	hipStream_t st = ctx->stream;
	const uint32_t nfill = (uint32_t)pl.fill.v.size();
	{ int e_ = tun_chain(LT, st, pl.tun.v, D(pl.tun), D(pl.tun_chunk_stream), tun_chunks, (TunTable *)(base + pl.tables_off), (uint64_t *)(base + pl.tun_partial_off),
		pl.tun_max_nchunks, true, D(pl.fill), nfill); if(e_) return e_; }
	if(ctx->single_stream || !nbig || nbig > TILES_BESIDE_MAX || pl.topo.v.empty()) { topology(); unpack(st); return CRTHIP_OK; }
	// a big mesh alone: every stream is decoded; the automaton (one serial chain: 2.2 of C2's 4 ms) goes on on the main stream, the attributes'
	// bit-unpack and their delta inversion in tiles on the second one, the tiles trailing the automaton's progress word
	hipStream_t s2;
	{ int e_ = fork(&s2); if(e_) return e_; }
	topology();
	unpack(s2);
	delta_tiles(s2);
	return join(s2);
}
// fork: attribute streams on stream2, CLERS + topology on the main stream
int Planner::forked() {
	const uint32_t ntun = (uint32_t)pl.tun.v.size(), nfill = (uint32_t)pl.fill.v.size();
	hipStream_t s2;
	{ int e_ = fork(&s2); if(e_) return e_; }
	entropy(ctx->stream, PH_ALL, 0, clers_tun, 0, clers_fill);
	topology();
	entropy(s2, PH_ALL, clers_tun, ntun, clers_fill, nfill);
	unpack(s2);
	delta_tiles(s2);
	return join(s2);
}
// the automata and K-BIT of a one-stream batch: k_front where it takes them (takes_front; with `carry`, hosts_carry(): the next batch's dictionaries
// behind K-BIT's waves), else the two launches
void Planner::front(const Carry *carry) {
	hipStream_t st = ctx->stream;
	const uint32_t nuw = (uint32_t)pl.unpack_wave_ids.v.size(), ntl = (uint32_t)pl.topo_lds_ids.v.size();
	if(!takes_front()) { topology(); unpack(st); }
	else if(carry) LT.run("front", k_front_carry, dim3(front_topo_blocks(ntl) + xcd_grid(nuw) + carry->ndicts), dim3(64), pl.topo_lds, st, D(pl.topo),
		D(pl.topo_lds_ids), ntl, D(pl.unpack), D(pl.unpack_wave_ids), nuw, carry->dicts, carry->ndicts, carry->tables);
	else LT.run("front", k_front, dim3(front_topo_blocks(ntl) + xcd_grid(nuw)), dim3(64), pl.topo_lds, st, D(pl.topo), D(pl.topo_lds_ids), ntl, D(pl.unpack),
		D(pl.unpack_wave_ids), nuw);
}
void Planner::delta(const Carry *carry) {
	if(pl.delta.v.empty()) return;
	hipStream_t st = ctx->stream;
	const uint32_t ngroups = (uint32_t)pl.delta_groups.v.size();
	if(!tiles_launched) delta_tiles(st);                    // (too big for the LDS records, and not launched beside the automaton above)
	if(ngroups && carry)                                    // ... and the next batch's stream groups behind this batch's blobs
		LT.run("delta_lds16", k_delta_lds16_carry, dim3(ngroups + carry->ngroups), dim3(256), std::max(pl.delta16_lds, TUN_CARRY_GROUP_LDS), st, D(pl.delta),
			D(pl.delta_groups), ngroups, carry->streams, carry->ids, carry->groups, carry->ngroups, carry->tables);
	else if(ngroups) LT.run("delta_lds16", k_delta_lds16, dim3(ngroups), dim3(256), pl.delta16_lds, st, D(pl.delta), D(pl.delta_groups), ngroups);
}
void Planner::cloud() {
	if(!cloud_chunks) return;
	hipStream_t st = ctx->stream;
	uint64_t *cloud_partial = (uint64_t *)(base + pl.cloud_partial_off);
	LT.run("cloud_sums", k_cloud_sums, dim3(cloud_chunks), dim3(256), 0, st, D(pl.cloud), D(pl.cloud_chunk_job), cloud_chunks, cloud_partial);
	LT.run("scan", k_scan_u64, dim3(1), dim3(1024), 0, st, cloud_partial, cloud_chunks);
	LT.run("cloud_apply", k_cloud_apply, dim3(cloud_chunks), dim3(256), 0, st, D(pl.cloud), D(pl.cloud_chunk_job), cloud_chunks, cloud_partial);
}
// the normals: the fused kernel over stored estimates, over blobs that store none (crthip_batch_bind_computed_normals), the unfused chain over the
// batch-wide arrays, the stored differences
void Planner::normals() {
	hipStream_t st = ctx->stream;
	by_ids("normal_blob", k_normal_blob<false>, 256, pl.normal_fused_lds, pl.normal, pl.normal_fused_ids, pl.normal_fused_lds);
	by_ids("normal_blob_computed", k_normal_blob<true>, 256, pl.normal_computed_lds, pl.normal, pl.normal_computed_ids, pl.normal_computed_lds);
	const uint32_t nvb = (uint32_t)pl.nv_block_job.v.size(), nfb = (uint32_t)pl.nf_block_job.v.size();
	if(pl.any_est_normal) {
		float *facen = (float *)(base + pl.facen_off);
		uint32_t *cnt = (uint32_t *)(base + pl.cnt_off), *cursor = (uint32_t *)(base + pl.cursor_off), *bnd = (uint32_t *)(base + pl.bnd_off);
		uint32_t *start = (uint32_t *)(base + pl.start_off), *flag = (uint32_t *)(base + pl.flag_off), *slot = (uint32_t *)(base + pl.slot_off);
		uint32_t *adj = (uint32_t *)(base + pl.adj_off);
		uint64_t *npart = (uint64_t *)(base + pl.nscan_partial_off);
		const uint32_t nv = pl.est_nvert, nch = (nv + CHUNK - 1)/CHUNK;
		auto scan = [&](uint32_t *in, uint32_t *out) {          // an exclusive scan over the batch's vertices: three launches, one record
			LT.begin("normal_scan");
			hipLaunchKernelGGL(k_u32_chunk_sums, dim3(nch), dim3(256), 0, st, in, nv, npart);
			hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, npart, nch);
			hipLaunchKernelGGL(k_u32_chunk_apply, dim3(nch), dim3(256), 0, st, in, out, nv, npart);
			LT.end();
		};
		LT.run("normal_faces", k_normal_faces, dim3(nfb), dim3(256), 0, st, D(pl.normal), D(pl.nf_block_job), D(pl.nf_block_first), nfb, facen, cnt, bnd);
		scan(cnt, start);
		LT.run("normal_fill", k_normal_fill, dim3(nfb), dim3(256), 0, st, D(pl.normal), D(pl.nf_block_job), D(pl.nf_block_first), nfb, start, cursor, adj);
		LT.run("normal_flags", k_normal_flags, dim3(nvb), dim3(256), 0, st, D(pl.normal), D(pl.nv_block_job), D(pl.nv_block_first), nvb, bnd, flag);
		scan(flag, slot);
		LT.run("normal_vertex", k_normal_vertex, dim3(nvb), dim3(256), 0, st, D(pl.normal), D(pl.nv_block_job), D(pl.nv_block_first), nvb, facen, start, cnt, adj,
			flag, slot);
	}
	if(pl.any_diff_normal) LT.run("normal_diff", k_normal_diff, dim3(nvb), dim3(256), 0, st, D(pl.normal), D(pl.nv_block_job), D(pl.nv_block_first), nvb);
}
// the derived outputs, each in its blob kernel or in its kernels over scratch
void Planner::derived() {
	// computed tangents: behind every normal kernel (the normals are final), in front of k_dequant (packed position and uv buffers hold integers)
	by_ids("tangent_blob", k_tangent_blob, TAN_THREADS, pl.tangent_lds, pl.tangent, pl.tangent_blob_ids);
	by_ids("tangent_faces", k_tangent_faces, TAN_THREADS, 0, pl.tangent, pl.tan_fblock_job);
	by_ids("tangent_vertex", k_tangent_vertex, TAN_THREADS, 0, pl.tangent, pl.tan_vblock_job);
	// meshlets: the index has been final since the automata
	by_ids("meshlet_blob", k_meshlet_blob, 64*pl.meshlet_waves, pl.meshlet_waves*(uint32_t)sizeof(MltWaveMem), pl.meshlet, pl.meshlet_blob_ids);
	by_ids("meshlet_segments", k_meshlet_segments, 64, 0, pl.meshlet, pl.mlt_block_job);
	by_ids("meshlet_place", k_meshlet_place, MLT_PLACE_THREADS, 0, pl.meshlet, pl.mlt_block_job);
	// meshlet bounds: the meshlets are final, the positions still integers
	by_ids("meshlet_bounds", k_meshlet_bounds, 64*MB_WAVES, 0, pl.meshlet_bounds, pl.mlb_block_job);
	// the weld: the integer positions (k_dequant runs behind) and the index; in front of adjacency, which may read the welded index
	by_ids("weld_blob", k_weld_blob, WELD_THREADS, pl.weld_lds, pl.weld, pl.weld_blob_ids);
	by_ids("weld_insert", k_weld_insert, WELD_THREADS, 0, pl.weld, pl.weld_vblock_job);
	by_ids("weld_lookup", k_weld_lookup, WELD_THREADS, 0, pl.weld, pl.weld_vblock_job);
	by_ids("weld_index", k_weld_index, WELD_THREADS, 0, pl.weld, pl.weld_cblock_job);
	// adjacency: the index alone, final since the automata
	by_ids("adjacency_blob", k_adjacency_blob, ADJ_THREADS, pl.adjacency_lds, pl.adjacency, pl.adjacency_blob_ids);
	by_ids("adjacency_count", k_adjacency_count, ADJ_THREADS, 0, pl.adjacency, pl.adj_block_job);
	by_ids("adjacency_offsets", k_adjacency_offsets, ADJ_THREADS, 0, pl.adjacency, pl.adj_big_ids);
	by_ids("adjacency_fill", k_adjacency_fill, ADJ_THREADS, 0, pl.adjacency, pl.adj_block_job);
	by_ids("adjacency_twin", k_adjacency_twin, ADJ_THREADS, 0, pl.adjacency, pl.adj_block_job);
	// levels of detail: a job a level; the integer positions (k_dequant runs behind) and the index
	by_ids("lod_blob", k_lod_blob, LOD_THREADS, pl.lod_lds, pl.lod, pl.lod_blob_ids);
	by_ids("lod_insert", k_lod_insert, LOD_THREADS, 0, pl.lod, pl.lod_vblock_job);
	by_ids("lod_lookup", k_lod_lookup, LOD_THREADS, 0, pl.lod, pl.lod_vblock_job);
	by_ids("lod_faces", k_lod_faces, LOD_THREADS, 0, pl.lod, pl.lod_fblock_job);
	by_ids("lod_keep", k_lod_keep, LOD_THREADS, 0, pl.lod, pl.lod_fblock_job);
	by_ids("lod_offsets", k_lod_offsets, LOD_THREADS, 0, pl.lod, pl.lod_big_ids);
	by_ids("lod_scatter", k_lod_scatter, LOD_THREADS, 0, pl.lod, pl.lod_fblock_job);
	// a cloud's levels of detail: a job a level; the integer positions, final since cloud() (k_dequant runs behind)
	by_ids("cloud_lod_blob", k_cloud_lod_blob, LOD_THREADS, pl.cloud_lod_lds, pl.cloud_lod, pl.cloud_lod_blob_ids);
	by_ids("cloud_lod_insert", k_cloud_lod_insert, LOD_THREADS, 0, pl.cloud_lod, pl.cloud_lod_vblock_job);
	by_ids("cloud_lod_lookup", k_cloud_lod_lookup, LOD_THREADS, 0, pl.cloud_lod, pl.cloud_lod_vblock_job);
	by_ids("cloud_lod_offsets", k_cloud_lod_offsets, LOD_THREADS, 0, pl.cloud_lod, pl.cloud_lod_big_ids);
	by_ids("cloud_lod_scatter", k_cloud_lod_scatter, LOD_THREADS, 0, pl.cloud_lod, pl.cloud_lod_vblock_job);
	by_ids("cloud_lod_chunks", k_cloud_lod_chunks, LOD_THREADS, 0, pl.cloud_lod, pl.cloud_lod_cblock_job);
	// compaction: a job a mesh set; every id list it reads - the index, the welded index, a level's index with its record - is final here
	by_ids("compact_blob", k_compact_blob, COMPACT_THREADS, 0, pl.compact, pl.compact_blob_ids);
	by_ids("compact_mark", k_compact_mark, COMPACT_THREADS, 0, pl.compact, pl.compact_cblock_job);
	by_ids("compact_count", k_compact_count, COMPACT_THREADS, 0, pl.compact, pl.compact_vblock_job);
	by_ids("compact_offsets", k_compact_offsets, COMPACT_THREADS, 0, pl.compact, pl.compact_big_ids);
	by_ids("compact_place", k_compact_place, COMPACT_THREADS, 0, pl.compact, pl.compact_vblock_job);
	by_ids("compact_index", k_compact_index, COMPACT_THREADS, 0, pl.compact, pl.compact_cblock_job);
	// the BVH: one more reader of the integer positions (k_dequant runs behind) and of the final index
	by_ids("bvh_blob", k_bvh_blob, BVH_THREADS, pl.bvh_lds, pl.bvh, pl.bvh_blob_ids);
	by_ids("bvh_boxes", k_bvh_boxes, BVH_THREADS, 0, pl.bvh, pl.bvh_fblock_job);
	by_ids("bvh_keys", k_bvh_keys, BVH_THREADS, 0, pl.bvh, pl.bvh_fblock_job);
	for(uint32_t pass = 0; pass < BVH_PASSES; pass++) {                      // a stable LSD radix sort, 8 bits a pass
		by_ids("bvh_sort_count", k_bvh_sort_count, BVH_THREADS, 0, pl.bvh, pl.bvh_tblock_job, pass);
		by_ids("bvh_sort_offsets", k_bvh_sort_offsets, BVH_THREADS, 0, pl.bvh, pl.bvh_big_ids);
		by_ids("bvh_sort_scatter", k_bvh_sort_scatter, BVH_THREADS, 0, pl.bvh, pl.bvh_tblock_job, pass);
	}
	by_ids("bvh_tree", k_bvh_tree, BVH_THREADS, 0, pl.bvh, pl.bvh_fblock_job);
	by_ids("bvh_refit", k_bvh_refit, BVH_THREADS, 0, pl.bvh, pl.bvh_fblock_job);
}
// the scratch path's finishers: k_dequant, and where it would sit the kernels of CRTHIP_BIND_QUANTIZED
void Planner::finish() {
	by_ids("dequantize", k_dequant, 256, 0, pl.dequant, pl.dequant_block_job);
	by_ids("quant_out_blob", k_quant_out_blob, 256, 0, pl.quant, pl.quant_blob_ids);
	by_ids("quant_range", k_quant_range, 256, 0, pl.quant, pl.quant_block_job);
	by_ids("quant_store", k_quant_store, 256, 0, pl.quant, pl.quant_block_job);
	// compaction's gathers: behind every kernel that writes a final vertex byte (dequantisation, normals, tangents and the quantised stores above)
	by_ids("compact_gather", k_compact_gather, COMPACT_THREADS, 0, pl.compact_gather, pl.compact_gblock_job);
}

int Planner::launch(uint32_t phases, const Carry *carry) {
	hipStream_t st = ctx->stream;
	if(phases != PH_ALL && !splits()) return fail(CRTHIP_E_ARGUMENT, "this batch's schedule has no separate entropy stage");
	if(phases & PH_UP) {
		if(pl.jobs_bytes) HIP_TRY(hipMemcpyAsync(base + pl.jobs_begin, stage, pl.jobs_bytes, hipMemcpyHostToDevice, st));
		if(pl.zero_end > pl.zero_begin) HIP_TRY(hipMemsetAsync(base + pl.zero_begin, 0, pl.zero_end - pl.zero_begin, st));
		for(uint32_t i = 0; i < nblobs; i++)                                         // the progress words of big meshes (a handful a batch at most)
			if(bs[i].progress != ~0ull) HIP_TRY(hipMemsetAsync(base + bs[i].progress, 0, TOPO_PROGRESS_BYTES, st));
	}
	const uint32_t ntun = (uint32_t)pl.tun.v.size(), nfill = (uint32_t)pl.fill.v.size(), ndict = (uint32_t)pl.tun_dict.v.size();
	// (a launch's streams share dictionaries when at least half of them repeat another one's table and there are enough of them for it to
	// matter: share_clers / share_attrs, decided where the groups were made)
	stat_dicts = (share_clers ? clers_dict : clers_tun) + (share_attrs ? ndict - clers_dict : ntun - clers_tun);
	nbig = nslices = 0; tiles_launched = false;
	for(auto &d : pl.delta.v) if(!delta_in_lds(d, wide)) { nbig++; nslices += d.N > 4 ? 1u : 0u; }
	switch(shape()) {
	case Shape::LongStreams: { int e_ = long_streams(); if(e_) return e_; } break;
	case Shape::Forked: { int e_ = forked(); if(e_) return e_; } break;
	case Shape::OneStream:
		entropy(st, phases, 0, ntun, 0, nfill);
		if(!(phases & PH_MESH)) { HIP_TRY(hipGetLastError()); return CRTHIP_OK; }
		front(carry);
	}
	delta(carry);
	cloud();
	normals();
	derived();
	finish();
	// (status: written by the kernels straight into the pinned block)
	HIP_TRY(hipGetLastError());
	return CRTHIP_OK;
}

// the event a call's sync / done wait for, behind everything the call enqueued (on the set of the batch whose stage M the call ran)
int Planner::mark_done() {
	HIP_TRY(hipEventRecord(ctx->ev_done, ctx->stream));
	set.done_covers_seq = set.upload_seq;
	return CRTHIP_OK;
}

void Planner::account() {
	const uint32_t ntun = (uint32_t)pl.tun.v.size();
	// stats
	b->stats.tunstall_in = stat_tin; b->stats.tunstall_out = stat_tout; b->stats.tunstall_tables = stat_tt; b->stats.tunstall_streams =
		ntun; b->stats.tunstall_dictionaries = (uint32_t)stat_dicts;
	b->stats.scratch_bytes = pl.total;
	b->stats.descriptor_bytes = (uint32_t)pl.jobs_bytes;
	b->stats.int16_streams = 0;
	for(const UnpackJob &u : pl.unpack.v) b->stats.int16_streams += u.out_kind == UNPACK_OUT_I16;
	b->stats.topology_scale = std::max(ctx->topo.scale, (ctx->topo.pool_q8 + 7)/8); b->stats.delta_wide = wide ? 1u : 0u;
	uint64_t ob = 0;
	for(auto &P : b->blobs) {
		const BlobLayout &L = P.L;
		if(P.index) ob += (uint64_t)L.h.nface*3*(P.index_u16 ? 2 : 4);
		for(size_t k = 0; k < P.bind.size(); k++) {
			if(!P.bind[k].buffer) continue;
			const AttrHeader &a = L.h.attrs[k];
			if(a.codec == CRTHIP_CODEC_NORMAL) ob += (uint64_t)L.h.nvert*3*(P.bind[k].format == CRTHIP_FMT_INT16 ? 2 : 4);
			else if(a.codec == CRTHIP_CODEC_COLOR) ob += (uint64_t)L.h.nvert*P.bind[k].out_components;
			else ob += (uint64_t)L.h.nvert*a.N*(P.bind[k].quantized ? 2u : generic_work_bytes(P.bind[k].format));
		}
		if(computes_normals(P)) ob += (uint64_t)L.h.nvert*3*(P.derived.normals.format == CRTHIP_FMT_INT16 ? 2 : 4);
		if(computes_tangents(P)) ob += (uint64_t)L.h.nvert*4*(P.derived.tangents.format == CRTHIP_FMT_INT16 ? 2 : 4);
	}
	b->stats.output_bytes = ob;
	ctx->in_flight = b; ctx->last_decoded = b;
	{ Carry c; b->carriable = carry_args(c) && hosts_carry(); }
	b->decoded = true; b->planned_wide = wide;
	b->quant_bound.assign(pl.quant_records, 0); b->quant_recs.clear();        // (the records: harvest)
	if(pl.quant_records) { size_t r = 0; for(auto &P : b->blobs) for(const Binding &bd : P.bind) b->quant_bound[r++] = bd.buffer && bd.quantized; }
	b->meshlet_bound.clear(); b->meshlet_recs.clear();                        // (the records: harvest)
	if(pl.meshlet_records) for(auto &P : b->blobs) b->meshlet_bound.push_back(builds_meshlets(P) && !P.host_status);
	b->dirty = false;
}
