// meshlet.h — crthip_batch_bind_meshlets: meshlets cut from a blob's decoded index (include/corto_hip.h has the contract).  The cut rule, the
// bound, one step of the builder and the placement rule as __host__ __device__ code, so that the host runs the very same source in the kernels'
// partition (crthip_meshlet_model, meshlet_host.cpp).
//
//   cuts     mlt_segments: the sorted group ends (clamped to nface) and nface, every stretch cut again every segment_faces faces.  Made on the
//            host; a segment reaches the kernels as an MltSeg: its faces and where its pieces go while their final place is not known -
//            meshlets from the bound's running sum, vertices from 3*first face, triangle bytes from 3*first face + 3*meshlets rounded up to 4.
//   builder  one WAVE a segment (mlt_segment).  A step takes the segment's next 64 faces, one a lane.  A corner is NEW if its vertex is not in
//            the current meshlet and no earlier corner of the window has it.  The inclusive wave sum of the faces' new counts gives the first
//            face that breaks a limit: the cut.  Faces before it are committed - a new corner's local id is |V| + the new corners before it -
//            and the next window starts at the cut.  A face's count depends only on the faces before it since the last cut, so this IS the
//            sequential rule.  A window whose first face breaks emits the meshlet and is taken again.
//   table    membership is an open-addressed table of MLT_TAB 64-bit entries a wave, keyed by vertex id: id << 32 | serial << 8 | payload.  A
//            serial comes from one counter a segment: a meshlet takes one when it starts (its entries are MEMBERS, payload the local id),
//            every window takes one (its entries are CLAIMS, payload the corner 3*lane + c).  An entry with any other serial is empty, so
//            nothing is ever cleared.  A corner claims an empty slot with a 64-bit compare-and-swap and lowers a claim of its own vertex
//            with a 64-bit min: the claim that stays is the window's FIRST corner of that vertex.  Committed claims become members in
//            place.  Claims of faces behind a cut die with the meshlet, which is emitted right there - so within a meshlet's life a live
//            entry never turns empty and a probe sequence never breaks.  Live entries: at most 255 members + 192 claims < MLT_TAB.
//   bytes    the meshlet's local ids are staged in LDS (3 x 512 bytes a wave) and leave as whole words with the pad bytes zeroed.
//   place    mlt_place: a segment's pieces move from scratch to prefix sums of the segments before it, offsets added.  A blob of ONE
//            segment has nothing in front: its wave writes the caller's arrays directly and there is no scratch and no move.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/corto_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MLT_HD __host__ __device__ inline
#else
#define MLT_HD inline
#endif
// k_meshlet.hip defines MLT_KERNELS: pointers into device memory and into LDS carry their address space there (global_* / ds_* and never
// flat_*: kernels_common.h); everywhere else, and in the host pass, the qualifiers are empty
#if defined(MLT_KERNELS) && defined(__HIP_DEVICE_COMPILE__)
#define MLT_MEM __attribute__((address_space(1)))
#define MLT_LDS __attribute__((address_space(3)))
#define MLT_DEVICE_PASS 1
#else
#define MLT_MEM
#define MLT_LDS
#define MLT_DEVICE_PASS 0
#endif

namespace corto_hip {

constexpr uint32_t MLT_WAVE = 64;                          // faces a window
constexpr uint32_t MLT_TAB = 512;                          // entries of a wave's table: a power of two above 255 + 192
constexpr uint32_t MLT_MAX_VERTICES = 255, MLT_MAX_TRIANGLES = 512;
constexpr uint32_t MLT_SEGMENT_DEFAULT = 4096, MLT_SEGMENT_MAX = 65536;
constexpr uint32_t MLT_PLACE_THREADS = 256;

// a segment as the host cuts it: faces [f0, f1); its provisional meshlet records start at mbase, its triangle bytes at tbase (a multiple
// of 4), its vertex words at 3*f0
struct MltSeg { uint32_t f0, f1, mbase, tbase; };
// what a segment came to: meshlets, vertex words, triangle bytes (a multiple of 4)
struct MltCount { uint32_t meshlets, vertices, triangle_bytes, pad; };
// sixteen bytes as one access (a plain vector: HIP's uint4 is a class whose assignment takes a generic `this`, which makes the store FLAT)
typedef uint32_t mlt_u32x4 __attribute__((ext_vector_type(4)));

// one wave's working memory: LDS in the kernels, heap in the host pass
struct MltWaveMem {
	uint64_t tab[MLT_TAB];                                 // the membership table
	uint32_t tri[MLT_MAX_TRIANGLES*3/4];                   // the current meshlet's local ids, 3 bytes a face
	uint16_t pub[MLT_WAVE];                                // a window's lanes to one another: (new corners in front of the face) << 3 | which corners are new
};
static_assert(sizeof(MltWaveMem) == 4096 + 1536 + 128, "a wave's LDS");

MLT_HD bool mlt_params_ok(uint32_t max_vertices, uint32_t max_triangles, uint32_t segment_faces) {
	return max_vertices >= 3 && max_vertices <= MLT_MAX_VERTICES && max_triangles >= 1 && max_triangles <= MLT_MAX_TRIANGLES && segment_faces <= MLT_SEGMENT_MAX;
}
MLT_HD uint32_t mlt_tmin(uint32_t max_vertices, uint32_t max_triangles) { const uint32_t tv = (max_vertices - 2 + 2)/3; return tv < max_triangles ? tv : max_triangles; }

// The cut rule.  ends: the group table as stored; emit(f0, f1) is called for every segment in face order.  `sorted`: scratch of ngroups + 1 words.
template <class Emit> inline void mlt_segments(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t segment_faces, uint32_t *sorted, Emit emit) {
	const uint32_t seg = segment_faces ? segment_faces : MLT_SEGMENT_DEFAULT;
	for(uint32_t g = 0; g < ngroups; g++) sorted[g] = group_end[g] < nface ? group_end[g] : nface;
	sorted[ngroups] = nface;
	for(uint32_t i = 1; i <= ngroups; i++) {                                 // insertion sort: group tables are short and nearly always in order
		const uint32_t x = sorted[i]; uint32_t j = i;
		for(; j > 0 && sorted[j - 1] > x; j--) sorted[j] = sorted[j - 1];
		sorted[j] = x;
	}
	uint32_t s = 0;
	for(uint32_t i = 0; i <= ngroups; i++) {
		const uint32_t e = sorted[i];
		while(s < e) { const uint32_t n = e - s > seg ? seg : e - s; emit(s, s + n); s += n; }
	}
}

// ---- the builder --------------------------------------------------------------------------------------------------------------------------

struct MltIn { MLT_MEM const void *faces; uint32_t faces_u16, max_vertices, max_triangles; };
// where a segment's pieces go (its first record, word and triangle word): the caller's arrays for a blob of one segment, else scratch
struct MltOut { MLT_MEM crthip_meshlet *meshlets; MLT_MEM uint32_t *vertices; MLT_MEM uint32_t *triangles; };
// the wave's uniform state
struct MltState {
	uint32_t pos, end;                                     // next face, the segment's end
	uint32_t t, nv;                                        // the current meshlet's faces and vertices
	uint32_t m, w, ctr;                                    // the meshlet's serial, the window's, the counter both come from
	uint32_t nm, voff, toff;                               // emitted so far: meshlets, vertex words, triangle bytes
};
// a lane's window state
struct MltLane { uint32_t v[3]; uint32_t slot[3]; uint32_t in, newmask, cnt, incl; };

MLT_HD uint32_t mlt_hash(uint32_t v) { return (v*0x9E3779B1u) >> 23; }       // 9 bits: MLT_TAB
static_assert(MLT_TAB == 512, "mlt_hash gives 9 bits");
MLT_HD uint64_t mlt_entry(uint32_t v, uint32_t serial, uint32_t payload) { return (uint64_t)v << 32 | (uint64_t)(serial << 8 | payload); }

MLT_HD uint64_t mlt_cas(MLT_LDS uint64_t *p, uint64_t expect, uint64_t val) {
#if MLT_DEVICE_PASS
	unsigned long long e = expect;
	__hip_atomic_compare_exchange_strong((MLT_LDS unsigned long long *)p, &e, (unsigned long long)val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	return e;
#else
	const uint64_t old = *p; if(old == expect) *p = val; return old;
#endif
}
MLT_HD void mlt_min(MLT_LDS uint64_t *p, uint64_t val) {
#if MLT_DEVICE_PASS
	__hip_atomic_fetch_min((MLT_LDS unsigned long long *)p, (unsigned long long)val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	if(val < *p) *p = val;
#endif
}
MLT_HD uint64_t mlt_peek(MLT_LDS const uint64_t *p) {
#if MLT_DEVICE_PASS
	return __hip_atomic_load((MLT_LDS const unsigned long long *)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
	return *p;
#endif
}

MLT_HD void mlt_load_face(const MltIn &J, uint32_t f, uint32_t v[3]) {
	if(J.faces_u16) { MLT_MEM const uint16_t *p = (MLT_MEM const uint16_t *)J.faces + (size_t)f*3; v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; }
	else { MLT_MEM const uint32_t *p = (MLT_MEM const uint32_t *)J.faces + (size_t)f*3; v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; }
}

// step 1, a lane: every corner finds its vertex's entry or makes one
MLT_HD void mlt_probe(MLT_LDS MltWaveMem &W, const MltState &S, uint32_t lane, MltLane &L) {
	if(!L.in) return;
	for(uint32_t c = 0; c < 3; c++) {
		const uint32_t v = L.v[c];
		const uint64_t mine = mlt_entry(v, S.w, 3*lane + c);
		uint32_t h = mlt_hash(v);
		for(;;) {
			const uint64_t e = mlt_peek(&W.tab[h]);
			const uint32_t ser = (uint32_t)e >> 8;
			if(ser == S.m || ser == S.w) {                                   // live
				if((uint32_t)(e >> 32) == v) { if(ser == S.w) mlt_min(&W.tab[h], mine); break; }
				h = (h + 1) & (MLT_TAB - 1);
				continue;
			}
			if(mlt_cas(&W.tab[h], e, mine) == e) break;                      // (lost to another lane: look at the slot again)
		}
		L.slot[c] = h;
	}
}
// step 2, a lane: which of its corners are new
MLT_HD void mlt_count(MLT_LDS MltWaveMem &W, const MltState &S, uint32_t lane, MltLane &L) {
	L.newmask = 0; L.cnt = 0;
	if(!L.in) return;
	for(uint32_t c = 0; c < 3; c++) {
		const uint64_t e = mlt_peek(&W.tab[L.slot[c]]);
		if(((uint32_t)e >> 8) == S.w && ((uint32_t)e & 255u) == 3*lane + c) { L.newmask |= 1u << c; L.cnt++; }
	}
}
// does the face of `lane` break a limit, given the inclusive sum of new corners up to it
MLT_HD bool mlt_breaks(const MltIn &J, const MltState &S, uint32_t lane, const MltLane &L) {
	return L.in && (S.t + lane + 1 > J.max_triangles || S.nv + L.incl > J.max_vertices);
}
MLT_HD void mlt_publish(MLT_LDS MltWaveMem &W, uint32_t lane, const MltLane &L) { W.pub[lane] = (uint16_t)((L.incl - L.cnt) << 3 | L.newmask); }
// step 3, a lane in front of the cut: local ids, the vertex words, the table's members, the bytes
MLT_HD void mlt_commit(MLT_LDS MltWaveMem &W, const MltState &S, const MltOut &O, uint32_t lane, uint32_t cut, const MltLane &L) {
	if(lane >= cut) return;
	MLT_LDS uint8_t *bytes = (MLT_LDS uint8_t *)W.tri;
	// (a slot read here may already be the member another lane of this step made of it: the same id)
	for(uint32_t c = 0; c < 3; c++) {
		const uint64_t e = mlt_peek(&W.tab[L.slot[c]]);
		uint32_t id = (uint32_t)e & 255u;
		if(((uint32_t)e >> 8) == S.w) {                                      // a claim: the id its first corner gets
			const uint32_t p = W.pub[id/3], fc = id%3;
			id = S.nv + (p >> 3) + (uint32_t)__builtin_popcount(p & ((1u << fc) - 1u));
		}
		if(L.newmask >> c & 1u) { O.vertices[S.voff + id] = L.v[c]; W.tab[L.slot[c]] = mlt_entry(L.v[c], S.m, id); }
		bytes[3*(S.t + lane) + c] = (uint8_t)id;
	}
}
// emission, a lane: the pad bytes, then the words and the record
MLT_HD void mlt_emit_pad(MLT_LDS MltWaveMem &W, const MltState &S, uint32_t lane) {
	MLT_LDS uint8_t *bytes = (MLT_LDS uint8_t *)W.tri;
	if(3*S.t + lane < ((3*S.t + 3) & ~3u)) bytes[3*S.t + lane] = 0;
}
MLT_HD void mlt_emit_store(MLT_LDS MltWaveMem &W, const MltState &S, const MltOut &O, uint32_t lane) {
	const uint32_t nw = (3*S.t + 3) >> 2;
	for(uint32_t i = lane; i < nw; i += MLT_WAVE) O.triangles[(S.toff >> 2) + i] = W.tri[i];
	if(lane == 0) {
#if MLT_DEVICE_PASS
		*(MLT_MEM mlt_u32x4 *)&O.meshlets[S.nm] = mlt_u32x4{S.voff, S.toff, S.nv, S.t};
#else
		O.meshlets[S.nm] = crthip_meshlet{S.voff, S.toff, S.nv, S.t};
#endif
	}
}
MLT_HD void mlt_emitted(MltState &S) {
	S.voff += S.nv; S.toff += (3*S.t + 3) & ~3u; S.nm++; S.t = S.nv = 0; S.m = ++S.ctr;
}

// A segment by one wave.  X is the wave: each(f) runs f(lane, MltLane &) for every lane (the kernel: its own; the host: all 64 in a shuffled
// order), window(J, pos, end, nwin) gives every lane its face of the window at pos (in, v), sync() orders the lanes' LDS traffic, scan() turns every lane's cnt into incl, first(pred) is the lowest lane pred(lane, L) holds
// for or 64, incl_of(lane) that lane's incl.  W must start out zeroed (serial 0 is nobody's).
template <class X> MLT_HD MltCount mlt_segment(X &x, MLT_LDS MltWaveMem &W, const MltIn &J, const MltSeg &sg, const MltOut &O) {
	MltState S;
	S.pos = sg.f0; S.end = sg.f1; S.t = S.nv = 0; S.ctr = 1; S.m = 1; S.w = 0; S.nm = S.voff = S.toff = 0;
	auto emit = [&]() {
		x.each([&](uint32_t lane, MltLane &) { mlt_emit_pad(W, S, lane); });
		x.sync();
		x.each([&](uint32_t lane, MltLane &) { mlt_emit_store(W, S, O, lane); });
		x.sync();
		mlt_emitted(S);
	};
	while(S.pos < S.end) {
		const uint32_t nwin = S.end - S.pos < MLT_WAVE ? S.end - S.pos : MLT_WAVE;
		S.w = ++S.ctr;
		x.window(J, S.pos, S.end, nwin);
		x.each([&](uint32_t lane, MltLane &L) { mlt_probe(W, S, lane, L); });
		x.sync();
		x.each([&](uint32_t lane, MltLane &L) { mlt_count(W, S, lane, L); });
		x.scan();
		uint32_t cut = x.first([&](uint32_t lane, const MltLane &L) { return mlt_breaks(J, S, lane, L); });
		if(cut > nwin) cut = nwin;
		if(cut == 0) { emit(); continue; }                                   // (the meshlet is not empty: a lone face fits)
		const uint32_t added = x.incl_of(cut - 1);
		x.each([&](uint32_t lane, MltLane &L) { mlt_publish(W, lane, L); });
		x.sync();
		x.each([&](uint32_t lane, MltLane &L) { mlt_commit(W, S, O, lane, cut, L); });
		x.sync();
		S.t += cut; S.nv += added; S.pos += cut;
		if(cut < nwin || S.pos == S.end) emit();
	}
	return MltCount{S.nm, S.voff, S.toff, 0};
}

// ---- placement ----------------------------------------------------------------------------------------------------------------------------

// a blob's scratch: the provisional arrays and a count a segment
struct MltScratch { MLT_MEM crthip_meshlet *meshlets; MLT_MEM uint32_t *vertices; MLT_MEM uint32_t *triangles; MLT_MEM MltCount *counts; };
MLT_HD MltOut mlt_provisional(const MltScratch &P, const MltSeg &sg) { return MltOut{P.meshlets + sg.mbase, P.vertices + (size_t)3*sg.f0, P.triangles + (sg.tbase >> 2)}; }
// bytes of a blob's scratch for a bound and a number of segments, and where its parts start
struct MltScratchLayout { uint64_t vertices, triangles, counts, total; };
MLT_HD MltScratchLayout mlt_scratch_layout(uint32_t nface, const crthip_meshlet_counts &bound) {
	MltScratchLayout l;
	l.vertices = (uint64_t)bound.meshlets*16;
	l.triangles = l.vertices + (((uint64_t)nface*12 + 15) & ~15ull);
	l.counts = l.triangles + (((uint64_t)bound.triangle_bytes + 4 + 15) & ~15ull);
	l.total = l.counts + (uint64_t)bound.segments*16;
	return l;
}
// thread tid of nthr moves its share of a segment's pieces behind `before`, the sum of the segments in front of it
MLT_HD void mlt_place(const MltScratch &P, const MltOut &F, const MltSeg &sg, const MltCount &before, const MltCount &own, uint32_t tid, uint32_t nthr) {
	const MltOut src = mlt_provisional(P, sg);
	for(uint32_t i = tid; i < own.meshlets; i += nthr) {
#if MLT_DEVICE_PASS
		mlt_u32x4 r = *(MLT_MEM const mlt_u32x4 *)&src.meshlets[i];
		r.x += before.vertices; r.y += before.triangle_bytes;
		*(MLT_MEM mlt_u32x4 *)&F.meshlets[before.meshlets + i] = r;
#else
		crthip_meshlet r = src.meshlets[i];
		r.vertex_offset += before.vertices; r.triangle_offset += before.triangle_bytes;
		F.meshlets[before.meshlets + i] = r;
#endif
	}
	for(uint32_t i = tid; i < own.vertices; i += nthr) F.vertices[before.vertices + i] = src.vertices[i];
	for(uint32_t i = tid; i < own.triangle_bytes >> 2; i += nthr) F.triangles[(before.triangle_bytes >> 2) + i] = src.triangles[i];
}
MLT_HD MltCount mlt_add(const MltCount &a, const MltCount &b) { return MltCount{a.meshlets + b.meshlets, a.vertices + b.vertices, a.triangle_bytes + b.triangle_bytes, 0}; }

// (meshlet_host.cpp) the host's part: a blob's segment table with the provisional bases, and the capacity bound with the exact segment count.
// false: a parameter outside its range, or a bound beyond 32 bits
bool mlt_plan(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t max_vertices, uint32_t max_triangles, uint32_t segment_faces,
              std::vector<MltSeg> *segs, crthip_meshlet_counts &bound);

} // namespace corto_hip
