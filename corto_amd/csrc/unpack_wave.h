// unpack_wave.h — K-BIT for the attributes of LDS-sized blobs, one wave per log stream: the body of k_unpack_wave (k_stream.hip),
// shared with k_front (k_mesh.hip), which runs the same waves behind the automata in one grid.  `block`: the workgroup's index among
// the K-BIT workgroups of its launch.
#pragma once
#include <type_traits>

#include "kernels_common.h"

namespace corto_hip {

// the (up to four) logs at i0 .. of a stream as one load: an unaligned dword, or - the stream's last, partial group - its last dword
// shifted down (streams shorter than four logs: bytewise).  r = the number of valid ones.
__device__ __forceinline__ uint32_t unpack_logs4(CRT_GLOBAL const uint8_t *logs, uint32_t count, uint32_t i0, uint32_t &r) {
	r = i0 < count ? min(count - i0, 4u) : 0u;
	if(count >= 4) {
		uint32_t dw = *(CRT_GLOBAL const uint32_t *)(logs + (r == 4u ? i0 : r ? count - 4u : 0u));
		asm volatile("" : "+v"(dw));
		return r == 4u ? dw : r ? dw >> (8u*(4u - r)) : 0u;
	}
	uint32_t raw = 0;
	for(uint32_t k = 0; k < r; k++) raw |= (uint32_t)logs[i0 + k] << (8u*k);
	return raw;
}

// K-BIT for the attributes of LDS-sized blobs (round 3): ONE WAVE PER LOG STREAM, lanes interleaved over the vertices.
// The chunked kernel above gives every 1 024 logs a workgroup of four waves (a C4 batch: 5 632 workgroups, 22 528 waves, each living
// ~6 us, two thirds of it waiting for its loads) and finds a chunk's bit offset by look-back through memory; launched twice it cost a
// pipelined decode 11.8 us of its 89 us per batch (profiles/r03_what_bounds_the_pipeline.txt) - more than its 31 us alone would suggest,
// because what it takes is wave slots and issue slots, 88 M wave-cycles a batch, more than every other kernel of the path together.
// Here a stream is ONE wave's: lane l takes logs l, l + 64, ... (every load and store of a round is 64 consecutive elements), a round's
// bit offsets are one DPP scan, the cursor is carried in a scalar - and the streams in front of it in the bit block (one per
// component, component-major: cstream.h:300-317) are simply added up again from their logs (a few KB), so nobody waits for anybody:
// no state words, no atomics.  A tenth of the waves, a quarter of the wave-cycles (the instruction count is the same).
constexpr uint32_t UW_R = 4;                                                // rounds of 64 logs per block: their loads in flight together
// Bit offsets are 32-bit here (the planner sends a bit block this way only when it has fewer than 2^26 words): round 3's 64-bit cursors made
// every window two 64-bit compares, a 64-bit shift and two 64-bit address computations - a third of the kernel's vector instructions, and
// the pipelined rate is within 2x of the chip's VALU issue rate.
__device__ __forceinline__ void unpack_wave_body(const UnpackJob *__restrict__ jobs, const uint32_t *__restrict__ job_ids, uint32_t njobs, uint32_t block) {
	// (one stream a workgroup of one wave; four streams a workgroup was measured level in round 4)
	// XCD-aware slots (kernels_common.h): the streams of one attribute are consecutive jobs - the four colour components write the bytes of the SAME lines
	// (out[4*i + comp]), and every stream re-adds the logs of the ones in front of it: through one L2, a C4 launch's WRITE_SIZE 23.5 -> 13.1 MB, FETCH_SIZE 5.8 -> 3.5
	const uint32_t slot = xcd_slot(block, njobs);
	if(slot >= njobs) return;
	const uint32_t jid = job_ids[slot];
	const UnpackJob J = jobs[jid];
	const uint32_t lane = threadIdx.x, count = J.count, fields = J.fields;
	CRT_GLOBAL const uint8_t *logs = as_global(J.logs);
	auto width = [](uint32_t l) -> uint32_t { return l > 32u ? 32u : l; };   // >32 cannot be produced by the encoder (UB in the reference)
	// the first block's logs, and everything in front of this stream in its bit block, in flight together
	uint32_t lg[UW_R];
#pragma unroll
	for(uint32_t r = 0; r < UW_R; r++) { const uint32_t i = r*64u + lane; lg[r] = logs[i < count ? i : (count ? count - 1u : 0u)]; }
	uint32_t running = 0;
	for(uint32_t jp = J.chain_chunk0; jp < jid; jp++) {                        // (chain_chunk0: for this kernel, the first JOB of the bit block)
		const UnpackJob &K = jobs[jp];
		CRT_GLOBAL const uint8_t *kl = as_global(K.logs);
		const uint32_t kc = K.count, kf = K.fields;
		uint32_t t = 0;
		for(uint32_t i0 = 4u*lane; i0 < kc; i0 += 4u*64u*4u) {                // four dwords per lane and pass
			uint32_t w4[4], r4[4];
#pragma unroll
			for(uint32_t u = 0; u < 4; u++) w4[u] = unpack_logs4(kl, kc, i0 + 256u*u, r4[u]);
#pragma unroll
			for(uint32_t u = 0; u < 4; u++)
#pragma unroll
				for(uint32_t k = 0; k < 4; k++) if(k < r4[u]) t += width((w4[u] >> (8u*k)) & 255u);
		}
		t = wave_inclusive_scan_u32(t);
		running += (uint32_t)__builtin_amdgcn_readlane((int)t, 63)*kf;
	}
	CRT_GLOBAL const uint32_t *words = as_global(J.words);
	const uint32_t nwords = J.nwords, last_word = nwords ? nwords - 1u : 0u, nbits = nwords << 5;   // (nwords < 2^26: the planner)
	// two words of the bit block at bit offset `at`.  INSIDE: the field lies inside the bit block - every field of a well-formed stream -
	// so only the second word's index can run one past the end (a field that ends on a word boundary) and nothing needs masking;
	// otherwise clamped loads, and field() masks what bit_field() would not have read
	auto window = [&](auto INSIDE, uint32_t at, uint32_t &hi, uint32_t &lo) {
		const uint32_t wi = at >> 5;
		hi = words[min(wi, last_word)];                                         // (a zero-width lane of an exactly full block sits AT nbits: clamp in both modes)
		lo = words[min(wi + 1u, last_word)];
	};
	auto field = [&](auto INSIDE, uint32_t at, uint32_t n, uint32_t hi, uint32_t lo) -> uint32_t {   // = bit_field(words, nwords, at, n); n == 0 -> 0
		const uint32_t sh = at & 31u;
		uint32_t h = hi, l = lo;
		if constexpr(!decltype(INSIDE)::value) {
			const uint32_t wi = at >> 5;
			h = wi < nwords ? hi : 0u; l = (sh + n > 32 && wi + 1 < nwords) ? lo : 0u;
		}
		const uint32_t top = sh ? __builtin_amdgcn_alignbit(h, l, 32u - sh) : h;   // the 32 bits from bit `sh` on: a funnel shift, not a 64-bit one (sh = 0: the shift count 32 would wrap to 0 and give l)
		return (n ? top : 0u) >> ((32u - n) & 31u);                           // top >> (32 - n) with neither the shift by 32 at n = 0 nor the one by -1 at n = 32 (a full word: ADVICE r4)
	};
	const bool values = (J.mode & 1u) != 0;
	const uint32_t stride = J.stride, comp = J.comp, out_limit = J.out_limit;
	const bool out_u8 = J.out_kind == UNPACK_OUT_U8, out_i16 = J.out_kind == UNPACK_OUT_I16;              // (I16: every width of the stream is <= 16 bits - its table says so, plan_jobs.cpp - and K-DELTA / K-NRM read int16)
	for(uint32_t base = 0; base < count; base += UW_R*64u) {
		// this block's widths and bit offsets (a scan per round, the cursor a scalar), then the next block's logs go out before the windows
		uint32_t d[UW_R], at[UW_R];
		bool ok = true;
#pragma unroll
		for(uint32_t r = 0; r < UW_R; r++) {
			const uint32_t i = base + r*64u + lane;
			d[r] = i < count ? width(lg[r]) : 0u;
			const uint32_t bits = d[r]*fields, incl = wave_inclusive_scan_u32(bits);
			at[r] = running + (incl - bits);
			ok = ok && running + incl <= nbits;
			running += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		}
		const bool inside = __all(ok) && nwords != 0;                            // (uniform) the whole block's fields inside the bit block
		if(base + UW_R*64u < count) {
#pragma unroll
			for(uint32_t r = 0; r < UW_R; r++) { const uint32_t i = base + (UW_R + r)*64u + lane; lg[r] = logs[i < count ? i : count - 1u]; }
		}
		auto body = [&](auto INSIDE) {
		if(values) {                                                           // decodeValues: sign folding (cstream.h:304-316); one field per log
			uint32_t hi[UW_R], lo[UW_R];
			if(nwords) {
#pragma unroll
				for(uint32_t r = 0; r < UW_R; r++) window(INSIDE, at[r], hi[r], lo[r]);
#pragma unroll
				for(uint32_t r = 0; r < UW_R; r++) asm volatile("" : "+v"(hi[r]), "+v"(lo[r]));
			} else {
#pragma unroll
				for(uint32_t r = 0; r < UW_R; r++) hi[r] = lo[r] = 0;
			}
#pragma unroll
			for(uint32_t r = 0; r < UW_R; r++) {
				const uint32_t i = base + r*64u + lane, dd = d[r];
				int32_t v = (int32_t)field(INSIDE, at[r], dd, hi[r], lo[r]);
				const int32_t mid = (int32_t)(dd ? 1u << (dd - 1u) : 0u);        // (dd == 0: v = 0, mid = 0: stays 0; dd == 32: 2^31, as the chunked kernel and the oracle)
				v = v < mid ? -v - mid : v;
				if(i < count && i < out_limit) {
					if(out_u8) as_global((uint8_t *)J.out)[i*stride + comp] = (uint8_t)v;
					else if(out_i16) as_global((int16_t *)J.out)[i*stride + comp] = (int16_t)v;
					else as_global((int32_t *)J.out)[i*stride + comp] = v;
				}
			}
		} else {                                                                 // decodeArray: v = raw - 2^(d-1); d == 0 -> zeros (cstream.h:337-357); `fields` values per log
#pragma unroll
			for(uint32_t g = 0; g < UW_R; g += 2) {                               // two rounds at a time: up to eight fields' windows in flight
				uint32_t hi[2][4], lo[2][4];
				const bool fast = fields <= 4 && nwords;                         // (uniform)
				if(fast) {
#pragma unroll
					for(uint32_t k = 0; k < 2; k++)
#pragma unroll
						for(uint32_t f = 0; f < 4; f++) window(INSIDE, at[g + k] + (f < fields ? f : 0u)*d[g + k], hi[k][f], lo[k][f]);
#pragma unroll
					for(uint32_t k = 0; k < 2; k++) asm volatile("" : "+v"(hi[k][0]), "+v"(lo[k][0]), "+v"(hi[k][1]), "+v"(lo[k][1]), "+v"(hi[k][2]), "+v"(lo[k][2]), "+v"(hi[k][3]), "+v"(lo[k][3]));
				}
#pragma unroll
				for(uint32_t k = 0; k < 2; k++) {
					const uint32_t i = base + (g + k)*64u + lane, dd = d[g + k];
					const bool store = i < count && i < out_limit;
					CRT_GLOBAL int32_t *out = as_global((int32_t *)J.out) + i*stride;
					CRT_GLOBAL int16_t *out16 = as_global((int16_t *)J.out) + i*stride;
					const uint32_t half = (uint32_t)((int32_t)(1u << (dd & 31u)) >> 1);   // upstream's `(1<<diff)>>1` in INT (cstream.h:343): 0 at dd = 32 (shift count mod 32), -2^30 at dd = 31 (arithmetic shift of INT_MIN), as k_unpack_extract
					if(fast) {
						int32_t v[4];
#pragma unroll
						for(uint32_t f = 0; f < 4; f++) v[f] = (int32_t)(field(INSIDE, at[g + k] + (f < fields ? f : 0u)*dd, dd, hi[k][f], lo[k][f]) - half);
						if(store && out_i16) {                                       // halfwords: the vertex' record is 2-byte aligned (4 when it has two or four fields)
							typedef int16_t i16x2_t __attribute__((ext_vector_type(2)));
							typedef int16_t i16x4_t __attribute__((ext_vector_type(4)));
							typedef i16x2_t __attribute__((aligned(4))) i16x2u; typedef i16x4_t __attribute__((aligned(4))) i16x4u;
							if(fields == 3) { out16[0] = (int16_t)v[0]; out16[1] = (int16_t)v[1]; out16[2] = (int16_t)v[2]; }
							else if(fields == 2) *(CRT_GLOBAL i16x2u *)out16 = i16x2_t{(int16_t)v[0], (int16_t)v[1]};
							else if(fields == 4) *(CRT_GLOBAL i16x4u *)out16 = i16x4_t{(int16_t)v[0], (int16_t)v[1], (int16_t)v[2], (int16_t)v[3]};
							else out16[0] = (int16_t)v[0];
						} else
						if(store) {                                                  // one vector store a vertex (the caller's ints are 4-byte aligned)
							typedef int32_t i32x2_t __attribute__((ext_vector_type(2)));
							typedef int32_t i32x3_t __attribute__((ext_vector_type(3)));
							typedef int32_t i32x4_t __attribute__((ext_vector_type(4)));
							typedef i32x2_t __attribute__((aligned(4))) i32x2u; typedef i32x3_t __attribute__((aligned(4))) i32x3u; typedef i32x4_t __attribute__((aligned(4))) i32x4u;
							if(fields == 3) *(CRT_GLOBAL i32x3u *)out = i32x3_t{v[0], v[1], v[2]};
							else if(fields == 2) *(CRT_GLOBAL i32x2u *)out = i32x2_t{v[0], v[1]};
							else if(fields == 4) *(CRT_GLOBAL i32x4u *)out = i32x4_t{v[0], v[1], v[2], v[3]};
							else out[0] = v[0];
						}
					} else {
						uint32_t oo = at[g + k];
						for(uint32_t f = 0; f < fields; f++) {
							const int32_t v = dd ? (int32_t)(bit_field(words, nwords, (uint64_t)oo, dd) - half) : 0;
							oo += dd;
							if(store) { if(out_i16) out16[f] = (int16_t)v; else out[f] = v; }
						}
					}
				}
			}
		}
		};
		if(inside) body(std::true_type{}); else body(std::false_type{});
	}
}

} // namespace corto_hip
