// bvh_check.cpp — both partitions of csrc/bvh.h on the host under AddressSanitizer and UBSan (tests/test_bvh_sanitize_cpu.py): a stand-alone
// program, host code only.  nodes, parent, order and the record are heap blocks of their own: nodes ENDS exactly at 2F - 1 records, parent at
// 2F - 1 words, order at F words and the record is a block of exactly 16 bytes, so a store one byte past what the contract allows is reported.
// (The hook's own scratch - what stands for the workgroup's LDS, the pairs, the sort's table, the arrival counters - is made at exactly the
// kernels' sizes: a step past an end is reported too.)  The positions and the index end at their last byte as well.  The two partitions must
// leave the same bytes under every seed, and those bytes must be a tree: every face in one leaf, every internal id once, boxes the unions.
// Built with csrc/bvh_host.cpp, whose one dependency on the library (ctx_fail) is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/corto_hip.h"
#include "bvh.h"

using namespace corto_hip;

namespace corto_hip {
int ctx_fail(int code, const char *) { return code; }
}

static int failures = 0;
#define CHECK(cond, ...) do { if(!(cond)) { failures++; printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while(0)

static uint64_t rng_state;
static uint64_t rng() { rng_state = rng_state*6364136223846793005ull + 1442695040888963407ull; return rng_state >> 16; }

// a block that ENDS at its last byte (aligned_alloc rounds a block to 16 bytes): the bytes, and the block to free
static uint8_t *ending_block(size_t sz, uint8_t **blk) {
	const size_t cap = sz ? (sz + 15)/16*16 : 16;
	*blk = (uint8_t *)aligned_alloc(16, cap);
	memset(*blk, 0xCD, cap);
	return *blk + (cap - sz);
}

// every face in one leaf, every internal id once, parent agrees, boxes are unions, the height is the longest path
static void check_tree(const crthip_bvh_node *nodes, const uint32_t *parent, const uint32_t *order, const crthip_bvh_counts &rec, uint32_t F, const char *tag) {
	std::vector<uint32_t> faces(F, 0), seen(2*(size_t)F - 1, 0), depth(2*(size_t)F - 1, 0), stack{0};
	uint32_t longest = 0;
	CHECK(parent[0] == CRTHIP_NO_NODE, "%s", tag);
	while(!stack.empty()) {
		const uint32_t n = stack.back(); stack.pop_back();
		CHECK(n < 2*F - 1 && !seen[n], "%s node %u", tag, n);
		if(n >= 2*F - 1 || seen[n]) return;
		seen[n] = 1;
		if(depth[n] > longest) longest = depth[n];
		const crthip_bvh_node &d = nodes[n];
		if(d.right == CRTHIP_BVH_LEAF) {
			CHECK(n >= F - 1 && d.left < F && order[n - (F - 1)] == d.left, "%s leaf %u", tag, n);
			if(d.left < F) faces[d.left]++;
			continue;
		}
		CHECK(n < F - 1 && d.left < 2*F - 1 && d.right < 2*F - 1, "%s node %u", tag, n);
		if(d.left >= 2*F - 1 || d.right >= 2*F - 1) return;
		const crthip_bvh_node &l = nodes[d.left], &r = nodes[d.right];
		for(int c = 0; c < 3; c++)
			CHECK(d.min[c] == (l.min[c] < r.min[c] ? l.min[c] : r.min[c]) && d.max[c] == (l.max[c] > r.max[c] ? l.max[c] : r.max[c]), "%s box of node %u", tag, n);
		CHECK(parent[d.left] == n && parent[d.right] == n, "%s parents of node %u", tag, n);
		depth[d.left] = depth[d.right] = depth[n] + 1;
		stack.push_back(d.left); stack.push_back(d.right);
	}
	for(uint32_t f = 0; f < F; f++) CHECK(faces[f] == 1, "%s face %u is in %u leaves", tag, f, faces[f]);
	for(size_t n = 0; n < 2*(size_t)F - 1; n++) CHECK(seen[n] == 1, "%s node %zu not reached", tag, n);
	CHECK(rec.nodes == 2*F - 1 && rec.faces == F && rec.height == longest && longest <= 64, "%s record {%u %u %u %u}, longest %u", tag, rec.nodes, rec.faces, rec.absent, rec.height, longest);
}

// kind 0: a strip over random vertices; 1: few cells (long runs of equal keys); 2: with ids >= nvert among them; 3: every face absent
static void one(uint32_t F, int kind, int u16) {
	rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)F*131u + kind*7u + u16);
	const uint32_t nvert = F + 2 > 60000 ? 60000 : F + 2;
	uint8_t *pblk, *iblk;
	int32_t *pos = (int32_t *)ending_block((size_t)nvert*12, &pblk);
	const uint32_t spread = kind == 1 ? 40 : 1u << 20;
	for(size_t k = 0; k < (size_t)nvert*3; k++) pos[k] = (int32_t)(rng() % spread) - (int32_t)(spread/2);
	uint8_t *index = ending_block((size_t)F*3*(u16 ? 2 : 4), &iblk);
	uint32_t absent = 0;
	for(uint32_t f = 0; f < F; f++) {
		uint32_t id[3] = {f % nvert, (f + 1) % nvert, (f + 2) % nvert};
		if(kind == 3 || (kind == 2 && f % 5 == 1)) { id[f % 3] = u16 ? 0xFFFFu : nvert + (uint32_t)(rng() % 1000); absent++; }
		for(int c = 0; c < 3; c++) { if(u16) ((uint16_t *)index)[(size_t)f*3 + c] = (uint16_t)id[c]; else ((uint32_t *)index)[(size_t)f*3 + c] = id[c]; }
	}
	const size_t nn = 2*(size_t)F - 1;
	std::vector<uint8_t> first;
	for(int which = 0; which < 2; which++) {
		if(which == 0 && !bvh_in_blob(F)) continue;
		for(uint32_t seed = 0; seed < 3; seed++) {
			uint8_t *nblk, *qblk, *oblk, *rblk;
			crthip_bvh_node *nodes = (crthip_bvh_node *)ending_block(nn*32, &nblk);
			uint32_t *parent = (uint32_t *)ending_block(nn*4, &qblk);
			uint32_t *order = (uint32_t *)ending_block((size_t)F*4, &oblk);
			crthip_bvh_counts *rec = (crthip_bvh_counts *)ending_block(16, &rblk);
			char tag[96];
			snprintf(tag, sizeof tag, "F %u kind %d u16 %d which %d seed %u", F, kind, u16, which, seed);
			// (a seed in three runs without the optional arrays: the hook's own parent array, no order)
			const bool bare = seed == 2;
			const int err = crthip_bvh_model(pos, nvert, index, (uint32_t)u16, F, nodes, bare ? nullptr : parent, bare ? nullptr : order, rec, which, seed*977u + 1);
			CHECK(err == CRTHIP_OK, "%s: %d", tag, err);
			CHECK(rec->absent == absent, "%s: absent %u, expected %u", tag, rec->absent, absent);
			std::vector<uint8_t> all(nn*32 + (bare ? 0 : nn*4 + (size_t)F*4) + 16);
			memcpy(all.data(), nodes, nn*32);
			if(!bare) { memcpy(all.data() + nn*32, parent, nn*4); memcpy(all.data() + nn*36, order, (size_t)F*4); }
			memcpy(all.data() + all.size() - 16, rec, 16);
			if(!bare) {
				check_tree(nodes, parent, order, *rec, F, tag);
				if(first.empty()) first = all;
				CHECK(all == first, "%s: the bytes differ from the first run's", tag);
			} else if(!first.empty())
				CHECK(memcmp(all.data(), first.data(), nn*32) == 0 && memcmp(all.data() + nn*32, first.data() + first.size() - 16, 16) == 0, "%s: the bare run's bytes differ", tag);
			free(nblk); free(qblk); free(oblk); free(rblk);
		}
	}
	free(pblk); free(iblk);
}

int main() {
	const uint32_t sizes[] = {1, 2, 3, 17, 255, 256, 257, BVH_TILE - 1, BVH_TILE, BVH_TILE + 1, BVH_BLOB_FACES - 1, BVH_BLOB_FACES, BVH_BLOB_FACES + 1, 2*BVH_TILE + 77};
	for(uint32_t F : sizes)
		for(int kind = 0; kind < 4; kind++) one(F, kind, (F + kind) & 1);
	// which 0 refuses a blob beyond its limit, before it touches anything
	{
		int32_t p[9] = {0};
		std::vector<uint32_t> idx(3*(BVH_BLOB_FACES + 1), 0);
		crthip_bvh_node *n = (crthip_bvh_node *)aligned_alloc(16, 32);
		CHECK(crthip_bvh_model(p, 3, idx.data(), 0, BVH_BLOB_FACES + 1, n, nullptr, nullptr, nullptr, 0, 0) == CRTHIP_E_LIMIT, "the limit");
		CHECK(crthip_bvh_model(p, 3, idx.data(), 0, 0, n, nullptr, nullptr, nullptr, 0, 0) == CRTHIP_E_ARGUMENT, "no faces");
		free(n);
	}
	if(failures) { printf("bvh_check: %d failures\n", failures); return 1; }
	printf("bvh_check ok\n");
	return 0;
}
