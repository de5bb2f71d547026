// plan_feedback_check.cpp — the trajectories of the decode contexts' two learning loops (corto_amd/csrc/plan_feedback.h), on the host:
// K-DELTA's narrow / wide layout with its back-off, K-TOPO's ring, pool and cap with theirs.  Built with AddressSanitizer and UBSan by
// tests/test_plan_feedback_cpu.py; prints "plan_feedback_check ok" and returns 0, or says which expectation failed.
#include <cstdio>
#include <vector>

#include "plan_feedback.h"

using namespace corto_hip;

static int failures = 0;
#define EXPECT(cond) do { if(!(cond)) { printf("line %d: %s\n", __LINE__, #cond); failures++; } } while(0)

static void delta() {
	DeltaFeedback d;
	EXPECT(!d.wide && d.calm == 0 && d.patience == 256 && !d.just_narrowed);
	d.update(false, 1, false);                                    // a context's first overflow
	EXPECT(d.wide && d.patience == 256 && !d.just_narrowed);
	for(int i = 0; i < 255; i++) { d.update(true, 0, false); EXPECT(d.wide); }
	d.update(true, 0, false);                                     // the 256th
	EXPECT(!d.wide && d.just_narrowed && d.calm == 0);
	d.update(false, 3, false);                                    // overflowed right after narrowing
	EXPECT(d.wide && d.patience == 512 && !d.just_narrowed);
	for(int i = 0; i < 511; i++) { d.update(true, 0, false); EXPECT(d.wide); }
	d.update(true, 0, false);
	EXPECT(!d.wide && d.just_narrowed);
	d.update(false, 0, false);                                    // narrow and fine
	EXPECT(!d.wide && !d.just_narrowed && d.patience == 512);
	d.update(false, 1, false);                                    // a later overflow
	EXPECT(d.wide && d.patience == 512);

	DeltaFeedback f;                                              // $CORTO_DELTA_WIDE=1: as the context sets it up
	f.wide = true;
	for(int i = 0; i < 3000; i++) f.update(true, 0, true);
	EXPECT(f.wide && !f.just_narrowed && f.patience == 256);

	DeltaFeedback g;                                              // wide spell, narrow, overflow at once - until the patience stops growing
	g.update(false, 1, false);
	for(int round = 0; round < 16; round++) {
		const uint32_t p = g.patience;
		for(uint32_t i = 0; i + 1 < p; i++) g.update(true, 0, false);
		EXPECT(g.wide);
		g.update(true, 0, false);
		EXPECT(!g.wide && g.just_narrowed);
		g.update(false, 1, false);
		EXPECT(g.wide && g.patience == (p < (1u << 20) ? 2*p : p));
	}
	EXPECT(g.patience == (1u << 20));
}

// every blob has 4 096 faces; a faller's flags word: bit 0, the ring slots it needed above it, the pool slots from bit 16
static TopoBlob clean() { return TopoBlob{4096, 2100, 0, 0}; }
static TopoBlob faller(uint32_t ring, uint32_t pool, int32_t status = 0) { return TopoBlob{4096, 2100, 1u | ring << 1 | pool << 16, status}; }
static void batch(TopoFeedback &t, size_t n, size_t nfall, TopoBlob f) {
	std::vector<TopoBlob> v(n, clean());
	for(size_t i = 0; i < nfall; i++) v[3*i + 1] = f;
	t.update(n, [&](size_t i) { return v[i]; });
}
static bool is(const TopoFeedback &t, uint32_t scale, uint32_t pool_q8, uint32_t pool_cap, uint32_t calm, uint32_t patience) {
	const bool ok = t.scale == scale && t.pool_q8 == pool_q8 && t.pool_cap == pool_cap && t.calm == calm && t.patience == patience;
	if(!ok) printf("  scale %u pool_q8 %u pool_cap %u calm %u patience %u\n", t.scale, t.pool_q8, t.pool_cap, t.calm, t.patience);
	return ok;
}

static void topo() {
	EXPECT(topo_slots(31) == 8 && topo_slots(32) == 4);
	TopoFeedback fresh;
	EXPECT(is(fresh, 1, 8, 0, 0, 64));
	// 1: three of forty
	TopoFeedback t1;
	batch(t1, 40, 3, faller(300, 200));
	EXPECT(is(t1, 2, 14, 225, 0, 128));
	// 2: two of forty is one in twenty, not more
	TopoFeedback t2 = t1;
	t2.calm = 5;
	batch(t2, 40, 2, faller(300, 200));
	EXPECT(is(t2, 2, 14, 225, 5, 128));
	TopoFeedback t2f;
	batch(t2f, 40, 2, faller(300, 200));
	EXPECT(is(t2f, 1, 8, 0, 0, 64));
	// 3: the same needs again - nothing grew, so everything doubles
	TopoFeedback t3 = t1;
	batch(t3, 40, 3, faller(300, 200));
	EXPECT(t3.scale == 4 && t3.pool_q8 == 28 && t3.pool_cap == 450 && t3.calm == 0);
	// 4: a calm run as long as the patience scales down, a second one reaches the floor, and the count stops there
	TopoFeedback t4 = t1;
	for(int i = 0; i < 127; i++) batch(t4, 40, 0, clean());
	EXPECT(is(t4, 2, 14, 225, 127, 128));
	batch(t4, 40, 0, clean());
	EXPECT(is(t4, 1, 10, 168, 0, 128));
	// 5: a fallback on the very next call
	TopoFeedback t5 = t4;
	batch(t5, 40, 3, faller(300, 200));
	EXPECT(t5.patience == 256 && t5.calm == 0);
	for(int i = 0; i < 127; i++) batch(t4, 40, 0, clean());
	EXPECT(is(t4, 1, 10, 168, 127, 128));
	batch(t4, 40, 0, clean());
	EXPECT(is(t4, 1, 8, 126, 0, 128));
	for(int i = 0; i < 300; i++) batch(t4, 40, 0, clean());
	EXPECT(is(t4, 1, 8, 126, 0, 128));
	// 6: fallers that teach nothing - an error, a ring or a pool beyond the LDS form
	const TopoBlob mute[3] = {faller(300, 200, -5), faller(5000, 200), faller(300, 5000)};
	for(const TopoBlob &f : mute) {
		TopoFeedback t6;
		batch(t6, 40, 3, f);
		EXPECT(is(t6, 1, 8, 0, 0, 128));
	}
	// 7: the cap's bound
	TopoFeedback t7;
	batch(t7, 40, 3, faller(300, 4096));
	EXPECT(t7.pool_cap == 4608);
	for(int i = 0; i < 40; i++) { batch(t7, 40, 3, faller(300, 4096)); EXPECT(t7.pool_cap == 4608 && t7.scale <= 16 && t7.pool_q8 <= 128); }
}

int main() {
	delta();
	topo();
	if(failures) { printf("plan_feedback_check: %d expectation(s) failed\n", failures); return 1; }
	printf("plan_feedback_check ok\n");
	return 0;
}
