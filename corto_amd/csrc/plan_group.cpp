// plan_group.cpp — Planner::group: streams sorted by dictionary, attributes into K-DELTA workgroups, the automata into launch classes, the
// job arrays placed; Planner::upload: the blocks reserved, the scratch pointers resolved, the arrays staged.
#include "batch_internal.h"

void Planner::group() {
	// streams of a launch that share dictionaries: sorted by dictionary (counting sort), cut into groups of one dictionary each
	const uint32_t ntun_all = (uint32_t)pl.tun.v.size(), ndict_all = (uint32_t)pl.tun_dict.v.size();
	// dictionaries by one kernel (K-TAB, 6 KB of LDS per wave), decodes by another (10 KB for a few us), instead of both in one wave per
	// stream
	// (16 KB for ~37 us): a batch of many streams is bound by LDS.time, so the split pays even when NO two streams share a
	// table
	auto shares = [&](uint32_t nstreams, uint32_t ndicts) { (void)ndicts; return ctx->dbg.tun_share == 0 ? false :
		ctx->dbg.tun_share == 1 ? true : nstreams >= 64; };
	share_clers = !pl.tun_multi_chunk && shares(clers_tun, clers_dict); share_attrs = !pl.tun_multi_chunk && shares(ntun_all - clers_tun,
		ndict_all - clers_dict);
	{
		std::vector<uint32_t> &cnt = ctx->dict_count;
		auto group_range = [&](uint32_t t0, uint32_t t1, uint32_t d0, uint32_t d1) {
			if(t1 <= t0) return;
			cnt.assign((size_t)(d1 - d0) + 1, 0u);
			for(uint32_t t = t0; t < t1; t++) cnt[pl.tun.v[t].dict - d0 + 1]++;
			for(uint32_t d = 1; d <= d1 - d0; d++) cnt[d] += cnt[d - 1];
			const uint32_t base = (uint32_t)pl.tun_group_ids.v.size();
			pl.tun_group_ids.v.resize((size_t)base + (t1 - t0));
			// (cnt[d] .. cnt[d + 1]: the dictionary's slots; groups before the fill moves the cursors)
			for(uint32_t d = 0; d < d1 - d0; d++)
				for(uint32_t k = cnt[d]; k < cnt[d + 1]; k += TUN_GROUP_MAX) pl.tun_groups.v.push_back(TunGroup{base + k,
					std::min(TUN_GROUP_MAX, cnt[d + 1] - k)});
			for(uint32_t t = t0; t < t1; t++) pl.tun_group_ids.v[base + cnt[pl.tun.v[t].dict - d0]++] = t;
		};
		if(share_clers) group_range(0, clers_tun, 0, clers_dict);
		pl.clers_groups = (uint32_t)pl.tun_groups.v.size();
		if(share_attrs) group_range(clers_tun, ntun_all, clers_dict, ndict_all);
	}

	// block maps of the normal jobs (per vertex / per face, 256 per block)
	for(uint32_t j = 0; j < pl.normal.v.size(); j++) {
		const NormalJob &n = pl.normal.v[j];
		pl.nv_block_first.v.push_back((uint32_t)pl.nv_block_job.v.size());
		push_blocks(pl.nv_block_job, j, (n.nvert + 255)/256);
		pl.nf_block_first.v.push_back((uint32_t)pl.nf_block_job.v.size());
		if(n.prediction != 0 && !n.fused) push_blocks(pl.nf_block_job, j, (n.nface + 255)/256);
	}

	// the LDS automata go up in ONE launch whose LDS request is the largest of theirs - unless some ask for much more than the others (a
	// 66K-triangle
	// mesh among 4K-triangle blobs): those get a launch of their own, so that a big mesh does not cost the small ones their occupancy. 
	// "Much more": beyond
	// 32 KB AND beyond twice the smallest request (round 5: a batch of Delaunay discs asks for 20-40 KB a blob, and cut at 32 KB it became
	// two launches
	// one after the other, each as long as its slowest blob - 1.07 ms instead of 0.57)
	if(!pl.topo_lds_ids.v.empty()) {
		uint32_t lo = 0xFFFFFFFFu;
		for(uint32_t nd : pl.topo_need) lo = std::min(lo, nd);
		const uint32_t cut = std::max(32u*1024u, 2u*lo);
		std::vector<uint32_t> small_ids;
		for(size_t k = 0; k < pl.topo_lds_ids.v.size(); k++) {
			const uint32_t nd = pl.topo_need[k], id = pl.topo_lds_ids.v[k];
			// (a blob whose automaton keeps a progress word - an attribute goes through k_delta_tiles - runs in the big launch: k_topology_lds_big is the kernel that does)
			if(nd <= cut && !(pl.topo.v[id].opts & TOPO_OPT_PROGRESS)) { small_ids.push_back(id); pl.topo_lds = std::max(pl.topo_lds, nd); }
			else { pl.topo_big_ids.v.push_back(id); pl.topo_big_lds = std::max(pl.topo_big_lds, nd); }
		}
		pl.topo_lds_ids.v.swap(small_ids);
	}
	// the jobs of k_delta_tiles first - whole attributes, then the slices of those of more than four components (a launch each); then attributes of
	// one blob that fit LDS together share a workgroup and the prediction graph: consecutive jobs with the same prediction array, up to DELTA_GROUP_MAX
	{
		const auto lds_begin = std::stable_partition(pl.delta.v.begin(), pl.delta.v.end(), [wide_ = wide](const DeltaJob &d) { return !delta_in_lds(d, wide_); });
		std::stable_partition(pl.delta.v.begin(), lds_begin, [](const DeltaJob &d) { return d.N <= 4; });
		size_t j = (size_t)(lds_begin - pl.delta.v.begin());
		while(j < pl.delta.v.size()) {
			const DeltaJob &d0 = pl.delta.v[j];
			DeltaGroup g{(uint32_t)j, 1};
			uint64_t vals = delta_vbytes(d0.nvert, d0.N, d0.is_u8 != 0, wide);
			bool hosted = delta_hosts_a(d0);
			while(j + g.count < pl.delta.v.size() && g.count < DELTA_GROUP_MAX) {
				const DeltaJob &d = pl.delta.v[j + g.count];
				if(d.pred != d0.pred || d.nvert != d0.nvert) break;
				const uint64_t more = delta_vbytes(d.nvert, d.N, d.is_u8 != 0, wide);
				const bool h2 = hosted || delta_hosts_a(d);
				if(vals + more + delta16_graph_lds(d0.nvert, h2) > DELTA16_LDS_MAX) break;
				vals += more; hosted = h2; g.count++;
			}
			pl.delta16_lds = std::max<uint32_t>(pl.delta16_lds, (uint32_t)(vals + delta16_graph_lds(d0.nvert, hosted)));
			pl.delta_groups.v.push_back(g);
			j += g.count;
		}
	}

	pl.tun_partial_off = cv.take(((uint64_t)tun_chunks*4 + 4)*8);
	pl.cloud_partial_off = cv.take(((uint64_t)cloud_chunks + 1)*8);
	// job arrays region
	pl.jobs_begin = cv.take(0);
	unpack_state_words = (uint64_t)unpack_chunks + 1;                    // (plan_carve's count was every bound stream's; the bit blocks that go a wave a stream keep no state)
	pl.unpack_partial_off = cv.take(unpack_state_words*8, 16);           // (first thing in the uploaded block: zeros)
	pl.each_array([&](auto &arr) { arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.each_optional_array([&](auto &arr) { if(!arr.v.empty()) arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.each_lod_array([&](auto &arr) { if(!arr.v.empty()) arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.each_cloud_lod_array([&](auto &arr) { if(!arr.v.empty()) arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.each_compact_array([&](auto &arr) { if(!arr.v.empty()) arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.each_bvh_array([&](auto &arr) { if(!arr.v.empty()) arr.dev_off = cv.take(arr.v.size()*sizeof(arr.v[0]) + 16, 16); });
	pl.jobs_bytes = cv.take(0) - pl.jobs_begin;
	pl.total = cv.take(0);
}

// upload() finishes the placing: the blocks reserved, the descriptors' scratch pointers resolved (SP: batch_internal.h), the arrays staged.  No kernel
// and no stream call, so a program without the HIP runtime links it and scans the staged image (tests/cpp/plan_dump.cpp): a pointer field missing from
// the list below would hand a kernel an address with bit 63 set
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
	for(auto &l : pl.lod.v) { resolve(l.position); resolve(l.index); resolve(l.counts); resolve(l.triples); resolve(l.vtable); resolve(l.ftable); resolve(l.blocks); }
	for(auto &c : pl.cloud_lod.v) { resolve(c.position); resolve(c.counts); resolve(c.table); resolve(c.wacc); resolve(c.blocks); }
	for(auto &c : pl.compact.v) { resolve(c.src); resolve(c.src_rec); resolve(c.newid); resolve(c.order); resolve(c.counts); resolve(c.mask); resolve(c.blocks); }
	for(auto &g : pl.compact_gather.v) { resolve(g.order); resolve(g.count_rec); resolve(g.cloud_rec); }
	for(auto &v : pl.bvh.v) { resolve(v.position); resolve(v.index); resolve(v.parent); resolve(v.scratch); }

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
	pl.each_array(stage_array); pl.each_optional_array(stage_array); pl.each_lod_array(stage_array); pl.each_cloud_lod_array(stage_array); pl.each_compact_array(stage_array); pl.each_bvh_array(stage_array);

	return CRTHIP_OK;
}

