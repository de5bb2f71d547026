// tun_stream.h — the decode of short Tunstall streams from a dictionary in LDS, as device functions: K-STREAM's kernels (k_tunstall.hip)
// and the grid that carries the NEXT batch's stream groups behind its own workgroups (k_delta.hip: k_delta_lds16).  Include inside
// namespace corto_hip, after kernels_common.h / device_plan.h and <type_traits>.
#pragma once

// Emit one thread's run (its up-to-4 words back to back) at byte pointer d.  Table words are read as ALIGNED dwords
// (v_alignbyte shifts out the word's byte phase) into a 64-bit byte FIFO; the run is written as <=3 head bytes (up to the next 4-aligned destination address),
// aligned dwords, and <=3 tail bytes: no unaligned accesses (on gfx950 those stall the LDS pipeline ~70 % of the time, PMC
// SQ_LDS_UNALIGNED_STALL) and no overlap with the neighbouring threads' runs.
template <typename DPtr>
__device__ __forceinline__ void tun_emit_run(DPtr d, uint32_t daddr, CRT_LDS const uint32_t *tab32, const uint32_t (&wo)[4], const uint32_t (&nb)[4]) {
	typedef typename std::conditional<std::is_same<DPtr, CRT_LDS uint8_t *>::value, CRT_LDS uint32_t, CRT_GLOBAL uint32_t>::type dword_t;
	// The FIFO starts at the 4-aligned address at or below d with m = d & 3 placeholder bytes (they belong to the previous
	// thread's run), so that every dword leaves on an aligned address; the first dword is then written byte-wise without
	// its m placeholder bytes, and the last partial dword byte-wise too.
	const uint32_t m = daddr & 3u;
	d -= m;
	uint32_t lo = 0, na = m;                                   // lo holds na (< 4) pending bytes
	bool first = m != 0;
#pragma unroll
	for(int k = 0; k < 4; k++) {
		if(nb[k] == 0) continue;
		CRT_LDS const uint32_t *src = tab32 + (wo[k] >> 2);
		const uint32_t sh = wo[k] & 3u;                        // words keep the reference's shared-suffix layout: any byte offset
		uint32_t prev = *src++;
		for(uint32_t i = 0; i < nb[k]; i += 4) {
			const uint32_t next = *src++;
			uint32_t dw = __builtin_amdgcn_alignbyte(next, prev, sh);
			prev = next;
			const uint32_t vb = min(4u, nb[k] - i);
			if(vb < 4) dw &= (1u << (8*vb)) - 1u;
			const uint32_t full = lo | (dw << (8*na));          // na < 4
			if(na + vb >= 4) {
				if(first) { for(uint32_t b = m; b < 4; b++) d[b] = (uint8_t)(full >> (8*b)); first = false; }
				else *(dword_t *)d = full;
				d += 4;
				lo = na ? dw >> (32 - 8*na) : 0u;
				na = na + vb - 4;
			} else { lo = full; na += vb; }
		}
	}
	for(uint32_t b = first ? m : 0u; b < na; b++) d[b] = (uint8_t)(lo >> (8*b));
}

// the decode of one short stream by one wave from a dictionary in LDS (offsets, lengths, word bytes): four codewords per lane and step
__device__ __forceinline__ void tun_stream_decode(const TunStream &st, const uint16_t *loff, const uint8_t *llen, const uint8_t *words) {
	const uint32_t lane = lane_id(), csize = st.csize;
	const uint64_t size = st.size;
	CRT_GLOBAL const uint8_t *src = as_global(st.src);
	CRT_GLOBAL uint8_t *gdst = as_global(st.dst);
	CRT_LDS const uint8_t *len8 = as_lds(llen);
	CRT_LDS const uint16_t *off16 = as_lds(loff);
	CRT_LDS const uint32_t *tab32 = (CRT_LDS const uint32_t *)as_lds(words);
	uint64_t base = 0;
	for(uint32_t tile = 0; tile < csize; tile += 256) {
		const uint32_t j0 = tile + 4*lane;
		// the lane's (up to) four codewords as ONE load: an unaligned dword at j0, or - the stream's last, partial group - the stream's last
		// dword shifted down; then the four lengths and the four offsets, every read unconditional and pinned.  (Written as four
		// `ok ? src[j0 + k] : 0` the compiler makes four exec-masked byte loads, each with its own wait and a dependent LDS read behind
		// it: eight serial round trips per 256 codewords - most of this kernel's time on a stream of a few hundred.)
		const uint32_t r = j0 < csize ? min(csize - j0, 4u) : 0u;            // valid codewords of this lane
		uint32_t raw;
		if(csize >= 4) {                                                    // (uniform)
			uint32_t dw = *(CRT_GLOBAL const uint32_t *)(src + (r == 4u ? j0 : r ? csize - 4u : 0u));
			asm volatile("" : "+v"(dw));
			raw = r == 4u ? dw : r ? dw >> (8u*(4u - r)) : 0u;
		} else {
			raw = 0;
			for(uint32_t k = 0; k < r; k++) raw |= (uint32_t)src[j0 + k] << (8u*k);
		}
		uint32_t code[4], l[4], sum = 0;
#pragma unroll
		for(int k = 0; k < 4; k++) code[k] = (raw >> (8*k)) & 255u;          // (0 beyond the stream's end: a valid table index)
#pragma unroll
		for(int k = 0; k < 4; k++) l[k] = (uint32_t)len8[code[k]];
		asm volatile("" : "+v"(l[0]), "+v"(l[1]), "+v"(l[2]), "+v"(l[3]));
#pragma unroll
		for(int k = 0; k < 4; k++) { l[k] = (uint32_t)k < r ? l[k] : 0u; sum += l[k]; }
		const uint32_t inc = wave_inclusive_scan_u32(sum);
		const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
		uint64_t oo = base + inc - sum;
		const uint64_t o_run = oo;
		uint32_t wo[4], nb[4];
#pragma unroll
		for(int k = 0; k < 4; k++) wo[k] = off16[code[k]];
		asm volatile("" : "+v"(wo[0]), "+v"(wo[1]), "+v"(wo[2]), "+v"(wo[3]));
#pragma unroll
		for(int k = 0; k < 4; k++) {                       // every word whole; the stream's last codeword emits what is left (tunstall.cpp:447-451)
			uint32_t n_ = l[k];
			if(j0 + k < csize) {
				if(j0 + k + 1 == csize) n_ = oo < size ? (uint32_t)min((uint64_t)(TUN_TABLE_BYTES - wo[k]), size - oo) : 0u;
				else if(oo + n_ > size) n_ = oo < size ? (uint32_t)(size - oo) : 0u;
			} else n_ = 0;
			nb[k] = n_;
			oo += l[k];
		}
		CRT_GLOBAL uint8_t *d = gdst + o_run;
		tun_emit_run(d, (uint32_t)(uintptr_t)d, tab32, wo, nb);
		base += total;
	}
}

// One group of k_tun_stream_grouped: up to TUN_GROUP_MAX streams of ONE dictionary, by a workgroup of 256 threads.  `dict`: TUN_GROUP_LDS
// bytes of LDS, 16-byte aligned (offsets | lengths | word bytes) - static in the kernel of its own, the head of the dynamic block in a
// grid that carries groups.  The dictionary was finished by an earlier launch.
constexpr uint32_t TUN_GROUP_LDS = 512 + 256 + TUN_TABLE_BYTES;
__device__ __forceinline__ void tun_group_body(const TunStream *__restrict__ streams, const uint32_t *__restrict__ ids, const TunGroup G,
                                               const TunTable *__restrict__ tables, uint8_t *dict) {
	typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
	uint16_t *loff = (uint16_t *)dict;
	uint8_t *llen = dict + 512, *words = dict + 768;
	const uint32_t t = threadIdx.x;
	const TunTable &T = tables[streams[ids[G.first]].dict];
	{
		CRT_GLOBAL const u32x4_t *o4 = (CRT_GLOBAL const u32x4_t *)as_global(T.off);
		CRT_GLOBAL const u32x4_t *w4 = (CRT_GLOBAL const u32x4_t *)as_global(T.bytes);
		u32x4_t hv = o4[t < 48 ? t : 47u], wv = w4[t];                          // (the table has 576 vectors of words: t < 256 is inside)
		asm volatile("" : "+v"(hv), "+v"(wv));
		if(t < 32) ((CRT_LDS u32x4_t *)as_lds(loff))[t] = hv;
		else if(t < 48) ((CRT_LDS u32x4_t *)as_lds(llen))[t - 32] = hv;
		((CRT_LDS u32x4_t *)as_lds(words))[t] = wv;
		const uint32_t nv = (min(T.used, TUN_TABLE_BYTES) + 15u) >> 4;
		for(uint32_t i = t + 256; i < nv; i += 256) ((CRT_LDS u32x4_t *)as_lds(words))[i] = w4[i];
	}
	__syncthreads();
	for(uint32_t k = wave_id(); k < G.count; k += 4) tun_stream_decode(streams[ids[G.first + k]], loff, llen, words);
}
