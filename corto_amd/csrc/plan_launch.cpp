// plan_launch.cpp — Planner::upload / launch / account: the blocks reserved, the descriptors' scratch pointers resolved (SP: batch_internal.h)
// and the arrays staged, the kernels enqueued in the order of crt::Decoder::decodeMesh / decodePointCloud (src/decoder.cpp:133-196),
// crthip_batch_stats filled.
#include "batch_internal.h"

int Planner::upload() {
	// ---- reserve device + pinned memory; one batch in flight per context ----
	// one batch in flight per context: the previous one's status is kept in its object
	if(harvest(ctx) != CRTHIP_OK) return fail(CRTHIP_E_DEVICE);
	if(set.scratch.reserve(pl.total + 256) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	if(set.staging.reserve(pl.jobs_bytes + 256) != CRTHIP_OK) return fail(CRTHIP_E_NOMEM);
	base = (uint8_t *)set.scratch.p;
	// every pointer field of every descriptor (SP offsets become base + offset; TopoJob.group_end: bytes into aux_u32)
	for(auto &t : pl.tun.v) { resolve(t.src); resolve(t.dst); resolve(t.probs); }
	for(auto &t : pl.tun_dict.v) { resolve(t.src); resolve(t.dst); resolve(t.probs); }
	for(auto &f : pl.fill.v) resolve(f.dst);
	for(auto &t : pl.topo.v) {
		t.group_end = (const uint32_t *)(base + pl.aux_u32.dev_off + (uintptr_t)t.group_end);
		resolve(t.clers); resolve(t.split_words); resolve(t.faces); resolve(t.pred); resolve(t.front_a); resolve(t.front_b); resolve(t.order);
		resolve(t.delayed); resolve(t.status); resolve(t.flags);
	}
	for(auto &u : pl.unpack.v) { resolve(u.logs); resolve(u.words); resolve(u.out); }
	for(auto &d : pl.delta.v) { resolve(d.values); resolve(d.pred); resolve(d.progress); resolve(d.out); resolve(d.flags); }
	for(auto &c : pl.cloud.v) resolve(c.values);
	for(auto &n : pl.normal.v) {
		resolve(n.diffs); resolve(n.out); resolve(n.position); resolve(n.faces); resolve(n.status); resolve(n.pos_out); resolve(n.fn_scratch);
	}
	for(auto &q : pl.dequant.v) { resolve(q.buffer); resolve(q.src); }
	for(auto &q : pl.quant.v) { resolve(q.values); resolve(q.range); }
	for(auto &t : pl.tangent.v) { resolve(t.position); resolve(t.uv); resolve(t.faces); resolve(t.acc); }
	for(auto &q : pl.meshlet_bounds.v) { resolve(q.position); resolve(q.counts); }
	for(auto &m : pl.meshlet.v) { m.segs = base + pl.aux_u32.dev_off + (uintptr_t)m.segs; resolve(m.faces); resolve(m.scratch); resolve(m.rec_dev); }
	for(auto &a : pl.adjacency.v) { resolve(a.index); resolve(a.counts); resolve(a.ends); resolve(a.list); }
	for(auto &w : pl.weld.v) { resolve(w.position); resolve(w.index); resolve(w.counts); resolve(w.table); }

	// host image -> device (one copy)
	stage = (uint8_t *)set.staging.p;
	memset(stage + (pl.unpack_partial_off - pl.jobs_begin), 0, unpack_state_words*8);
	// (after the harvest above: the previous batch's words have been read)
	memset(set.status_host.p, 0, hs.bytes());
	if(pl.quant_records) {                                               // a quantised attribute of a blob without vertices has no job: its record is all zero, written
		crthip_quant_transform *rec = (crthip_quant_transform *)((uint8_t *)set.status_host.p + hs.records());
		for(const BlobPlan &P : b->blobs) {
			for(size_t k = 0; k < P.bind.size(); k++) if(P.bind[k].buffer && P.bind[k].quantized && P.L.h.nvert == 0) rec[k].written = 1;
			rec += P.bind.size();
		}
	}
	auto stage_array = [&](auto &arr) { if(!arr.v.empty()) memcpy(stage + (arr.dev_off - pl.jobs_begin), arr.v.data(), arr.v.size()*sizeof(arr.v[0])); };
	pl.each_array(stage_array); pl.each_optional_array(stage_array);

	return CRTHIP_OK;
}

// The schedule has two stages (batch_internal.h: PH_*).  Stage E - the descriptor copy, the zeroing, K-TAB, K-STREAM, k_fill - reads the batch's arena and
// descriptors and writes only the batch's own scratch; stage M is everything behind it and writes the caller's outputs and the status words.
// crthip_batch_decode runs both in one call.  crthip_batch_decode_with_next runs stage M of one batch with stage E of the lane's next batch:
// as launches of its own (PH_TUN), or - `carry`, the next batch's K-TAB / K-STREAM arguments - inside this batch's k_front / k_delta_lds16 grids.
bool Planner::splits() const {
	const uint32_t ntun = (uint32_t)pl.tun.v.size(), nfill = (uint32_t)pl.fill.v.size();
	if(pl.tun_multi_chunk) return false;
	return !(!pl.topo.v.empty() && (ntun > clers_tun || nfill > clers_fill || unpack_chunks || !pl.unpack_wave_ids.v.empty()) && !ctx->single_stream);
}
bool Planner::takes_front() const {
	return ctx->single_stream && !ctx->dbg.front_off && !pl.topo_lds_ids.v.empty() && !pl.unpack_wave_ids.v.empty() && pl.topo_big_ids.v.empty() &&
		pl.topo_glob_ids.v.empty() && !unpack_chunks && pl.topo_lds <= FRONT_LDS_MAX;
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
	return !ctx->dbg.carry_off && splits() && takes_front() && pl.topo_lds >= TUN_CARRY_GROW_LDS && !pl.delta.v.empty() && !pl.delta_groups.v.empty();
}

int Planner::launch(uint32_t phases, const Carry *carry) {
	hipStream_t st = ctx->stream;
	Launch LT{ctx};
	if(phases != PH_ALL && !splits()) return fail(CRTHIP_E_ARGUMENT, "this batch's schedule has no separate entropy stage");
	if(phases & PH_UP) {
		if(pl.jobs_bytes) HIP_TRY(hipMemcpyAsync(base + pl.jobs_begin, stage, pl.jobs_bytes, hipMemcpyHostToDevice, st));
		if(pl.zero_end > pl.zero_begin) HIP_TRY(hipMemsetAsync(base + pl.zero_begin, 0, pl.zero_end - pl.zero_begin, st));
		for(uint32_t i = 0; i < nblobs; i++)                                         // the progress words of big meshes (a handful a batch at most)
			if(bs[i].progress != ~0ull) HIP_TRY(hipMemsetAsync(base + bs[i].progress, 0, TOPO_PROGRESS_BYTES, st));
	}

	auto D = [&](auto &arr) { return (decltype(arr.v.data()))(base + arr.dev_off); };
	TunTable *tables = (TunTable *)(base + pl.tables_off);
	uint64_t *tun_partial = (uint64_t *)(base + pl.tun_partial_off);
	uint64_t *unpack_partial = (uint64_t *)(base + pl.unpack_partial_off);
	uint64_t *cloud_partial = (uint64_t *)(base + pl.cloud_partial_off);

	const uint32_t ntun = (uint32_t)pl.tun.v.size();
	const uint32_t nfill = (uint32_t)pl.fill.v.size();
	const uint32_t ndict = (uint32_t)pl.tun_dict.v.size();
	// (a launch's streams share dictionaries when at least half of them repeat another one's table and there are enough of them for it to
	// matter: share_clers / share_attrs, decided where the groups were made)
	stat_dicts = (share_clers ? clers_dict : clers_tun) + (share_attrs ? ndict - clers_dict : ntun - clers_tun);
	auto tunstall = [&](hipStream_t s, uint32_t t0, uint32_t t1, uint32_t c0, uint32_t c1, uint32_t f0, uint32_t f1) {
		if(t1 > t0 && (phases & PH_TUN)) {                   // every stream here is one chunk: one wave per stream
			(void)c0; (void)c1;
			// [t0, t1) is the CLERS streams, the attribute streams, or both (dictionaries are numbered the same way)
			const bool has_clers = t0 == 0 && clers_tun > 0, has_attrs = t1 == ntun && ntun > clers_tun;
			const bool share = (!has_clers || share_clers) && (!has_attrs || share_attrs) && (has_clers || has_attrs);
			// distinct tables first, then every stream decodes from its (shared) dictionary
			if(share) {
				const uint32_t d0 = has_clers ? 0u : clers_dict, d1 = has_attrs ? ndict : clers_dict;
				// (an alphabet of more than 64 symbols builds its words in LDS: tun_tables.h)
				uint32_t big = 0;
				for(uint32_t d = d0; d < d1; d++) if(pl.tun_dict.v[d].nsym > 64) big = TUN_TABLE_BYTES;
				LT.begin("tunstall_tables", s); hipLaunchKernelGGL(k_tun_tables, dim3(d1 - d0), dim3(64), big, s, D(pl.tun_dict) + d0,
					d1 - d0, tables); LT.end();
				const uint32_t g0 = has_clers ? 0u : pl.clers_groups, g1 = has_attrs ? (uint32_t)pl.tun_groups.v.size() : pl.clers_groups;
				LT.begin("tunstall_stream", s); hipLaunchKernelGGL(k_tun_stream_grouped, dim3(g1 - g0), dim3(256), 0, s, D(pl.tun),
					D(pl.tun_group_ids), D(pl.tun_groups) + g0, g1 - g0, tables); LT.end();
			} else {                                           // dictionary + decode in one kernel
				LT.begin("tunstall_stream", s); hipLaunchKernelGGL(k_tun_stream, dim3(t1 - t0), dim3(64), 0, s, D(pl.tun) + t0, t1 - t0);
					LT.end();
			}
		}
		if(f1 > f0 && (phases & PH_FILL)) { LT.begin("fill", s); hipLaunchKernelGGL(k_fill, dim3(f1 - f0), dim3(256), 0, s, D(pl.fill) + f0, f1 - f0); LT.end(); }
	};
	auto unpack = [&](hipStream_t s) {
		const uint32_t nuw = (uint32_t)pl.unpack_wave_ids.v.size();
		if(nuw) { LT.begin("unpack_wave", s); hipLaunchKernelGGL(k_unpack_wave, dim3(xcd_grid(nuw)), dim3(64), 0, s, D(pl.unpack),
			D(pl.unpack_wave_ids), nuw); LT.end(); }
		if(!unpack_chunks) return;
		LT.begin("unpack_extract", s); hipLaunchKernelGGL(k_unpack_extract, dim3(unpack_chunks), dim3(256), 0, s, D(pl.unpack),
			D(pl.unpack_chunk_job), unpack_chunks, unpack_partial); LT.end();
	};
	// K-DELTA's jobs too big for the LDS records (sorted to the front; behind them the groups of k_delta_lds16)
	uint32_t nbig = 0, nslices = 0;                                              // (the slices: the last nslices of the nbig)
	for(auto &d : pl.delta.v) if(!delta_in_lds(d, wide)) { nbig++; nslices += d.N > 4 ? 1u : 0u; }
	bool tiles_launched = false;
	// the big ones in tiles of 1 024 vertices (k_delta_tiles).  On a lone context this goes to the SECOND stream, behind the attribute streams' bit-unpack
	// and BESIDE the automaton, whose progress word the tiles wait for: a single big mesh's delta inversion trails its topology instead of following it
	// (config C2: 1.5 of 4.0 ms).  The automaton is enqueued first on its own stream and waits for nothing of this kernel.
	// BESIDE the automaton only a handful of workgroups: they hold 66 KB of LDS each while they wait, and a batch of hundreds of big meshes' tiles, resident
	// first, could keep the automata (up to 156 KB a workgroup) from ever finding a CU - the tiles would wait for a progress word nobody can write.  Up to 48
	// (sixteen big meshes' three attributes; a slice of an attribute of more than four components counts as one) leave most of the chip free; more run
	// behind the automaton as on a pool context.
	constexpr uint32_t TILES_BESIDE_MAX = 48;
	auto delta_tiles = [&](hipStream_t s) {
		if(!nbig) return;
		if(s != st && nbig > TILES_BESIDE_MAX) return;
		LT.begin("delta_tiles", s);
		if(nbig > nslices) hipLaunchKernelGGL(k_delta_tiles<false>, dim3(nbig - nslices), dim3(DELTA_THREADS), 0, s, D(pl.delta), nbig - nslices);
		if(nslices) hipLaunchKernelGGL(k_delta_tiles<true>, dim3(nslices), dim3(DELTA_THREADS), 0, s, D(pl.delta) + (nbig - nslices), nslices);
		LT.end();
		tiles_launched = true;
	};
	auto topology = [&]() -> int {
		if(!pl.topo_lds_ids.v.empty() || !pl.topo_big_ids.v.empty()) {
			LT.begin("topology_lds");
			if(!pl.topo_big_ids.v.empty()) { const uint32_t nj = (uint32_t)pl.topo_big_ids.v.size(); hipLaunchKernelGGL(k_topology_lds_big,
				dim3(nj), dim3(64), pl.topo_big_lds, st, D(pl.topo), D(pl.topo_big_ids), nj); }
			if(!pl.topo_lds_ids.v.empty()) { const uint32_t nj = (uint32_t)pl.topo_lds_ids.v.size(); hipLaunchKernelGGL(k_topology_lds,
				dim3(nj), dim3(64), pl.topo_lds, st, D(pl.topo), D(pl.topo_lds_ids), nj); }
			LT.end();
		}
		if(!pl.topo_glob_ids.v.empty()) {
			const uint32_t nj = (uint32_t)pl.topo_glob_ids.v.size();
			LT.begin("topology"); hipLaunchKernelGGL(k_topology, dim3(nj), dim3(64), 0, st, D(pl.topo), D(pl.topo_glob_ids), nj); LT.end();
		}
		return CRTHIP_OK;
	};
	if(pl.tun_multi_chunk) {
		// long streams (scaled Tunstall runs, very large meshes): chunk offsets need one scan over all chunks; single stream
		uint32_t big = 0;
		for(auto &t : pl.tun.v) if(t.nsym > 64) big = TUN_TABLE_BYTES;
		LT.begin("tunstall_tables"); hipLaunchKernelGGL(k_tun_tables, dim3(ntun), dim3(64), big, st, D(pl.tun), ntun, tables); LT.end();
		LT.begin("tunstall_chunk_sums"); hipLaunchKernelGGL(k_tun_chunk_sums, dim3(tun_chunks), dim3(256), 0, st, D(pl.tun),
			D(pl.tun_chunk_stream), tun_chunks, tables, tun_partial, 0u); LT.end();
		// (up to 256 chunks a stream: every decode wave adds up the sums in front of it itself; longer streams: one workgroup per stream
		// scans them)
		const bool scanned = pl.tun_max_nchunks > 256;
		if(scanned) { LT.begin("tunstall_stream_scan"); hipLaunchKernelGGL(k_tun_stream_scan, dim3(ntun), dim3(256), 0, st, D(pl.tun),
			ntun, tun_partial); LT.end(); }
		LT.begin("tunstall_decode");
		if(launch_tun_decode_staged(st, D(pl.tun), D(pl.tun_chunk_stream), tun_chunks, tables, tun_partial, scanned ? 0u : 1u)) return fail(CRTHIP_E_DEVICE);
		LT.end();
		if(nfill) { LT.begin("fill"); hipLaunchKernelGGL(k_fill, dim3(nfill), dim3(256), 0, st, D(pl.fill), nfill); LT.end(); }
		if(!ctx->single_stream && nbig && nbig <= TILES_BESIDE_MAX && !pl.topo.v.empty()) {
			// a big mesh alone: every stream is decoded; the automaton (one serial chain: 2.2 of C2's 4 ms) goes on on the main stream, the attributes'
			// bit-unpack and their delta inversion in tiles on the second one, the tiles trailing the automaton's progress word
			hipStream_t s2;
			{ int e_ = ctx_stream2(ctx, &s2); if(e_) return e_; }
			HIP_TRY(hipEventRecord(ctx->ev_fork, st));
			HIP_TRY(hipStreamWaitEvent(s2, ctx->ev_fork, 0));
			{ int e_ = topology(); if(e_) return e_; }
			unpack(s2);
			delta_tiles(s2);
			HIP_TRY(hipEventRecord(ctx->ev_join, s2));
			HIP_TRY(hipStreamWaitEvent(st, ctx->ev_join, 0));
		} else {
			{ int e_ = topology(); if(e_) return e_; }
			unpack(st);
		}
	} else if(!pl.topo.v.empty() && (ntun > clers_tun || nfill > clers_fill || unpack_chunks || !pl.unpack_wave_ids.v.empty()) &&
		!ctx->single_stream) {
		// fork: attribute streams on stream2, CLERS + topology on the main stream
		hipStream_t s2;
		{ int e_ = ctx_stream2(ctx, &s2); if(e_) return e_; }
		HIP_TRY(hipEventRecord(ctx->ev_fork, st));
		HIP_TRY(hipStreamWaitEvent(s2, ctx->ev_fork, 0));
		tunstall(st, 0, clers_tun, 0, clers_chunks, 0, clers_fill);
		{ int e_ = topology(); if(e_) return e_; }
		tunstall(s2, clers_tun, ntun, clers_chunks, tun_chunks, clers_fill, nfill);
		unpack(s2);
		delta_tiles(s2);
		HIP_TRY(hipEventRecord(ctx->ev_join, s2));
		HIP_TRY(hipStreamWaitEvent(st, ctx->ev_join, 0));
	} else {
		tunstall(st, 0, ntun, 0, tun_chunks, 0, nfill);
		if(!(phases & PH_MESH)) { HIP_TRY(hipGetLastError()); return CRTHIP_OK; }
		// one stream: the automata and the attributes' bit-unpack in one grid (k_front) when the batch has nothing else for either -
		// no big or HBM-front automaton, no chunked K-BIT - and the automata ask for little LDS (K-BIT's waves hold the same request)
		const uint32_t nuw = (uint32_t)pl.unpack_wave_ids.v.size(), ntl = (uint32_t)pl.topo_lds_ids.v.size();
		if(takes_front() && carry) {                            // (hosts_carry(): the next batch's dictionaries behind K-BIT's waves)
			LT.begin("front"); hipLaunchKernelGGL(k_front_carry, dim3(front_topo_blocks(ntl) + xcd_grid(nuw) + carry->ndicts), dim3(64), pl.topo_lds, st,
				D(pl.topo), D(pl.topo_lds_ids), ntl, D(pl.unpack), D(pl.unpack_wave_ids), nuw, carry->dicts, carry->ndicts, carry->tables); LT.end();
		} else if(takes_front()) {
			LT.begin("front"); hipLaunchKernelGGL(k_front, dim3(front_topo_blocks(ntl) + xcd_grid(nuw)), dim3(64), pl.topo_lds, st, D(pl.topo),
				D(pl.topo_lds_ids), ntl, D(pl.unpack), D(pl.unpack_wave_ids), nuw); LT.end();
		} else {
			{ int e_ = topology(); if(e_) return e_; }
			unpack(st);
		}
	}
	if(!pl.delta.v.empty()) {
		const uint32_t ngroups = (uint32_t)pl.delta_groups.v.size();
		if(!tiles_launched) delta_tiles(st);                    // (too big for the LDS records, and not launched beside the automaton above)
		if(ngroups && carry) {                                  // ... and its stream groups behind this batch's blobs
			LT.begin("delta_lds16"); hipLaunchKernelGGL(k_delta_lds16_carry, dim3(ngroups + carry->ngroups), dim3(256), std::max(pl.delta16_lds, TUN_CARRY_GROUP_LDS), st,
				D(pl.delta), D(pl.delta_groups), ngroups, carry->streams, carry->ids, carry->groups, carry->ngroups, carry->tables); LT.end();
		} else if(ngroups) { LT.begin("delta_lds16"); hipLaunchKernelGGL(k_delta_lds16, dim3(ngroups), dim3(256), pl.delta16_lds, st, D(pl.delta), D(pl.delta_groups),
			ngroups); LT.end(); }
	}
	if(cloud_chunks) {
		LT.begin("cloud_sums"); hipLaunchKernelGGL(k_cloud_sums, dim3(cloud_chunks), dim3(256), 0, st, D(pl.cloud), D(pl.cloud_chunk_job),
			cloud_chunks, cloud_partial); LT.end();
		LT.begin("scan"); hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, cloud_partial, cloud_chunks); LT.end();
		LT.begin("cloud_apply"); hipLaunchKernelGGL(k_cloud_apply, dim3(cloud_chunks), dim3(256), 0, st, D(pl.cloud),
			D(pl.cloud_chunk_job), cloud_chunks, cloud_partial); LT.end();
	}
	const uint32_t nvb = (uint32_t)pl.nv_block_job.v.size(), nfb = (uint32_t)pl.nf_block_job.v.size();
	if(!pl.normal_fused_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.normal_fused_ids.v.size();
		LT.begin("normal_blob"); hipLaunchKernelGGL(k_normal_blob<false>, dim3(nj), dim3(256), pl.normal_fused_lds, st, D(pl.normal),
			D(pl.normal_fused_ids), nj, pl.normal_fused_lds); LT.end();
	}
	if(!pl.normal_computed_ids.v.empty()) {                     // blobs that store no normals (crthip_batch_bind_computed_normals)
		const uint32_t nj = (uint32_t)pl.normal_computed_ids.v.size();
		LT.begin("normal_blob_computed"); hipLaunchKernelGGL(k_normal_blob<true>, dim3(nj), dim3(256), pl.normal_computed_lds, st, D(pl.normal),
			D(pl.normal_computed_ids), nj, pl.normal_computed_lds); LT.end();
	}
	if(pl.any_est_normal) {
		float *facen = (float *)(base + pl.facen_off);
		uint32_t *cnt = (uint32_t *)(base + pl.cnt_off), *cursor = (uint32_t *)(base + pl.cursor_off), *bnd = (uint32_t *)(base +
			pl.bnd_off);
		uint32_t *start = (uint32_t *)(base + pl.start_off), *flag = (uint32_t *)(base + pl.flag_off), *slot = (uint32_t *)(base +
			pl.slot_off);
		uint32_t *adj = (uint32_t *)(base + pl.adj_off);
		uint64_t *npart = (uint64_t *)(base + pl.nscan_partial_off);
		const uint32_t nv = pl.est_nvert, nch = (nv + CHUNK - 1)/CHUNK;
		LT.begin("normal_faces"); hipLaunchKernelGGL(k_normal_faces, dim3(nfb), dim3(256), 0, st, D(pl.normal), D(pl.nf_block_job),
			D(pl.nf_block_first), nfb, facen, cnt, bnd); LT.end();
		LT.begin("normal_scan");
		hipLaunchKernelGGL(k_u32_chunk_sums, dim3(nch), dim3(256), 0, st, cnt, nv, npart);
		hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, npart, nch);
		hipLaunchKernelGGL(k_u32_chunk_apply, dim3(nch), dim3(256), 0, st, cnt, start, nv, npart);
		LT.end();
		LT.begin("normal_fill"); hipLaunchKernelGGL(k_normal_fill, dim3(nfb), dim3(256), 0, st, D(pl.normal), D(pl.nf_block_job),
			D(pl.nf_block_first), nfb, start, cursor, adj); LT.end();
		LT.begin("normal_flags"); hipLaunchKernelGGL(k_normal_flags, dim3(nvb), dim3(256), 0, st, D(pl.normal), D(pl.nv_block_job),
			D(pl.nv_block_first), nvb, bnd, flag); LT.end();
		LT.begin("normal_scan");
		hipLaunchKernelGGL(k_u32_chunk_sums, dim3(nch), dim3(256), 0, st, flag, nv, npart);
		hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, st, npart, nch);
		hipLaunchKernelGGL(k_u32_chunk_apply, dim3(nch), dim3(256), 0, st, flag, slot, nv, npart);
		LT.end();
		LT.begin("normal_vertex"); hipLaunchKernelGGL(k_normal_vertex, dim3(nvb), dim3(256), 0, st, D(pl.normal), D(pl.nv_block_job),
			D(pl.nv_block_first), nvb, facen, start, cnt, adj, flag, slot); LT.end();
	}
	if(pl.any_diff_normal) { LT.begin("normal_diff"); hipLaunchKernelGGL(k_normal_diff, dim3(nvb), dim3(256), 0, st, D(pl.normal),
		D(pl.nv_block_job), D(pl.nv_block_first), nvb); LT.end(); }
	// computed tangents: behind every normal kernel (the normals are final), in front of k_dequant (packed position and uv buffers hold integers)
	if(!pl.tangent_blob_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.tangent_blob_ids.v.size();
		LT.begin("tangent_blob"); hipLaunchKernelGGL(k_tangent_blob, dim3(nj), dim3(TAN_THREADS), pl.tangent_lds, st, D(pl.tangent), D(pl.tangent_blob_ids), nj); LT.end();
	}
	if(!pl.tan_fblock_job.v.empty()) {
		const uint32_t ntf = (uint32_t)pl.tan_fblock_job.v.size(), ntv = (uint32_t)pl.tan_vblock_job.v.size();
		LT.begin("tangent_faces"); hipLaunchKernelGGL(k_tangent_faces, dim3(ntf), dim3(TAN_THREADS), 0, st, D(pl.tangent), D(pl.tan_fblock_job), ntf); LT.end();
		LT.begin("tangent_vertex"); hipLaunchKernelGGL(k_tangent_vertex, dim3(ntv), dim3(TAN_THREADS), 0, st, D(pl.tangent), D(pl.tan_vblock_job), ntv); LT.end();
	}
	// meshlets: the index has been final since the automata
	if(!pl.meshlet_blob_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.meshlet_blob_ids.v.size();
		LT.begin("meshlet_blob"); hipLaunchKernelGGL(k_meshlet_blob, dim3(nj), dim3(64*pl.meshlet_waves), pl.meshlet_waves*(uint32_t)sizeof(MltWaveMem), st, D(pl.meshlet),
			D(pl.meshlet_blob_ids), nj); LT.end();
	}
	if(!pl.mlt_block_job.v.empty()) {
		const uint32_t nb = (uint32_t)pl.mlt_block_job.v.size();
		LT.begin("meshlet_segments"); hipLaunchKernelGGL(k_meshlet_segments, dim3(nb), dim3(64), 0, st, D(pl.meshlet), D(pl.mlt_block_job), nb); LT.end();
		LT.begin("meshlet_place"); hipLaunchKernelGGL(k_meshlet_place, dim3(nb), dim3(MLT_PLACE_THREADS), 0, st, D(pl.meshlet), D(pl.mlt_block_job), nb); LT.end();
	}
	// meshlet bounds: the meshlets are final, the positions still integers
	if(!pl.mlb_block_job.v.empty()) {
		const uint32_t nb = (uint32_t)pl.mlb_block_job.v.size();
		LT.begin("meshlet_bounds"); hipLaunchKernelGGL(k_meshlet_bounds, dim3(nb), dim3(64*MB_WAVES), 0, st, D(pl.meshlet_bounds), D(pl.mlb_block_job), nb); LT.end();
	}
	// the weld: the integer positions (k_dequant runs behind) and the index; in front of adjacency, which may read the welded index
	if(!pl.weld_blob_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.weld_blob_ids.v.size();
		LT.begin("weld_blob"); hipLaunchKernelGGL(k_weld_blob, dim3(nj), dim3(WELD_THREADS), pl.weld_lds, st, D(pl.weld), D(pl.weld_blob_ids), nj); LT.end();
	}
	if(!pl.weld_vblock_job.v.empty()) {
		const uint32_t nb = (uint32_t)pl.weld_vblock_job.v.size(), nc = (uint32_t)pl.weld_cblock_job.v.size();
		LT.begin("weld_insert"); hipLaunchKernelGGL(k_weld_insert, dim3(nb), dim3(WELD_THREADS), 0, st, D(pl.weld), D(pl.weld_vblock_job), nb); LT.end();
		LT.begin("weld_lookup"); hipLaunchKernelGGL(k_weld_lookup, dim3(nb), dim3(WELD_THREADS), 0, st, D(pl.weld), D(pl.weld_vblock_job), nb); LT.end();
		if(nc) { LT.begin("weld_index"); hipLaunchKernelGGL(k_weld_index, dim3(nc), dim3(WELD_THREADS), 0, st, D(pl.weld), D(pl.weld_cblock_job), nc); LT.end(); }
	}
	// adjacency: the index alone, final since the automata
	if(!pl.adjacency_blob_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.adjacency_blob_ids.v.size();
		LT.begin("adjacency_blob"); hipLaunchKernelGGL(k_adjacency_blob, dim3(nj), dim3(ADJ_THREADS), pl.adjacency_lds, st, D(pl.adjacency), D(pl.adjacency_blob_ids), nj); LT.end();
	}
	if(!pl.adj_big_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.adj_big_ids.v.size(), nb = (uint32_t)pl.adj_block_job.v.size();
		LT.begin("adjacency_count"); hipLaunchKernelGGL(k_adjacency_count, dim3(nb), dim3(ADJ_THREADS), 0, st, D(pl.adjacency), D(pl.adj_block_job), nb); LT.end();
		LT.begin("adjacency_offsets"); hipLaunchKernelGGL(k_adjacency_offsets, dim3(nj), dim3(ADJ_THREADS), 0, st, D(pl.adjacency), D(pl.adj_big_ids), nj); LT.end();
		LT.begin("adjacency_fill"); hipLaunchKernelGGL(k_adjacency_fill, dim3(nb), dim3(ADJ_THREADS), 0, st, D(pl.adjacency), D(pl.adj_block_job), nb); LT.end();
		LT.begin("adjacency_twin"); hipLaunchKernelGGL(k_adjacency_twin, dim3(nb), dim3(ADJ_THREADS), 0, st, D(pl.adjacency), D(pl.adj_block_job), nb); LT.end();
	}
	const uint32_t ndq = (uint32_t)pl.dequant_block_job.v.size();
	if(ndq) { LT.begin("dequantize"); hipLaunchKernelGGL(k_dequant, dim3(ndq), dim3(256), 0, st, D(pl.dequant), D(pl.dequant_block_job),
		ndq); LT.end(); }
	// CRTHIP_BIND_QUANTIZED: the scratch path's other finisher, where k_dequant sits
	if(!pl.quant_blob_ids.v.empty()) {
		const uint32_t nj = (uint32_t)pl.quant_blob_ids.v.size();
		LT.begin("quant_out_blob"); hipLaunchKernelGGL(k_quant_out_blob, dim3(nj), dim3(256), 0, st, D(pl.quant), D(pl.quant_blob_ids), nj); LT.end();
	}
	if(!pl.quant_block_job.v.empty()) {
		const uint32_t nqb = (uint32_t)pl.quant_block_job.v.size();
		LT.begin("quant_range"); hipLaunchKernelGGL(k_quant_range, dim3(nqb), dim3(256), 0, st, D(pl.quant), D(pl.quant_block_job), nqb); LT.end();
		LT.begin("quant_store"); hipLaunchKernelGGL(k_quant_store, dim3(nqb), dim3(256), 0, st, D(pl.quant), D(pl.quant_block_job), nqb); LT.end();
	}

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
