// draw_host.cpp -- nte_probe_draw.h on the CPU: the probe stage's draw coordinates enumerated, and the order of events of
// probe_claim_try played with simulated workgroups on two XCD ids, one call at a time in a seeded random order, the
// stores that publish an XCD's pair landing late.
//
//   draw_host selftest      prints one line per case and a tally; exit status 0 iff nothing differs
//
// Built by tests/test_draw_cpu.py with a plain host compiler (and once more under -fsanitize=address,undefined).
#include "../../ntedit_amd/csrc/nte_probe_draw.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace nte;

static unsigned long long g_mismatches = 0, g_waits = 0;

static void
expect(bool ok, const char* what, unsigned a, unsigned b, unsigned c)
{
	if (!ok) {
		if (g_mismatches < 20) {
			std::fprintf(stderr, "MISMATCH %s (%u, %u, %u)\n", what, a, b, c);
		}
		g_mismatches++;
	}
}

// every (run, step below the bound) exactly once, nothing beyond, one closing draw: the last
static void
coords_case(u32 n_wg, u32 longest)
{
	const unsigned long long before = g_mismatches;
	const u32 steps = longest ? (longest + PROBE_STEP - 1) / PROBE_STEP : 1;
	const u32 total = draw_total(n_wg, longest);
	expect(total == n_wg * steps * (u32)PROBE_STEP && total >= (u32)PROBE_STEP, "total", n_wg, longest, total);
	std::vector<u32> seen((size_t)n_wg * steps, 0);
	u32 draws = 0, closing = 0, units = 0;
	for (u32 p = 0; p < total; p += PROBE_DRAW, draws++) {
		if (total - p <= PROBE_DRAW) {
			closing++;
			expect(p + PROBE_DRAW >= total, "the closing draw is the last", n_wg, longest, p);
		}
		for (u32 wave = 0; wave < (u32)PROBE_WAVES; wave++) {
			const u32 at = p + wave * PROBE_STEP;
			if (at >= total) {
				continue; // (the kernel's wavefront skips it)
			}
			u32 run = ~0u, i0 = ~0u;
			draw_unit(at, n_wg, run, i0);
			expect(run < n_wg && i0 % PROBE_STEP == 0 && i0 / PROBE_STEP < steps, "unit in range", at, run, i0);
			if (run < n_wg && i0 / PROBE_STEP < steps) {
				seen[(size_t)(i0 / PROBE_STEP) * n_wg + run]++;
				units++;
			}
			// the eight wavefronts of a draw: the same step, or the next one where the draw wraps round the runs
			u32 run0 = 0, i00 = 0;
			draw_unit(p, n_wg, run0, i00);
			expect(i0 >= i00 && i0 - i00 <= ((u32)PROBE_WAVES + n_wg - 1) / n_wg * PROBE_STEP, "a draw's steps are neighbours", at, i0, i00);
		}
	}
	for (size_t i = 0; i < seen.size(); i++) {
		expect(seen[i] == 1, "every unit once", (unsigned)i, seen[i], n_wg);
	}
	expect(closing == 1 && draws >= 1, "one closing draw", n_wg, longest, closing);
	std::printf("coords n_wg %u longest %u: draws %u units %u mismatches %llu\n", n_wg, longest, draws, units, g_mismatches - before);
}

// The control words on the host: plain words, one simulated thread at a time.  Atomics take effect at once; a store is
// DELAYED: it waits in `pending` until the scheduler lets it land or its owner touches the control words again (program
// order), so other workgroups run inside the windows between a claim's compare-and-swap or its bump of the slice counter
// and the store that publishes the XCD's new pair -- they see "being claimed" or the pair that has run out, and wait.
struct HostCtl
{
	struct Store
	{
		u32 owner, i, v;
	};
	std::vector<u32> ctl;
	std::vector<u32> lng;
	std::vector<Store> pending;
	u32 owner = 0;

	void
	land(size_t at)
	{
		ctl.at(pending[at].i) = pending[at].v;
		pending.erase(pending.begin() + (long)at);
	}
	void
	land_own()
	{
		for (size_t at = 0; at < pending.size();) {
			if (pending[at].owner == owner) {
				land(at);
			} else {
				at++;
			}
		}
	}

	u32
	add(u32 i, u32 v)
	{
		land_own();
		const u32 old = ctl.at(i);
		ctl.at(i) = old + v;
		return old;
	}
	u32
	cas(u32 i, u32 expect_, u32 v)
	{
		land_own();
		const u32 old = ctl.at(i);
		if (old == expect_) {
			ctl.at(i) = v;
		}
		return old;
	}
	u32
	load(u32 i)
	{
		land_own();
		return ctl.at(i);
	}
	void
	store(u32 i, u32 v)
	{
		pending.push_back(Store{ owner, i, v });
	}
	u32
	longest(u32 slice)
	{
		return lng.at(slice);
	}
};

struct Workgroup
{
	u32 xcd, sl, p, total;
	bool done;
};

// k_bin_probe's thread 0, one call of probe_claim_try per event, its stores delayed (HostCtl); a draw's units are tallied
// as the wavefronts would probe them.  The atomics of ONE call are not interleaved with other workgroups' (each is a
// single read-modify-write on the device too); what the play varies is who runs between them and the stores.
static void
claim_case(const std::vector<u32>& longest, u32 n_wg, u32 plog, u32 n_workgroups, u32 seed)
{
	const unsigned long long before = g_mismatches;
	const u32 n_slices = (u32)longest.size(), n_units = n_slices << plog;
	HostCtl c;
	c.ctl.assign(CTL_WORK + n_units + 1, 0);
	c.lng = longest;
	std::vector<std::vector<u32>> seen(n_units);
	unsigned long long want = 0;
	for (u32 u = 0; u < n_units; u++) {
		seen[u].assign(draw_total(n_wg, longest[u >> plog]) / PROBE_STEP, 0);
		want += seen[u].size();
	}
	std::vector<Workgroup> wg(n_workgroups);
	for (u32 i = 0; i < n_workgroups; i++) {
		wg[i] = Workgroup{ i % 3 == 0 ? 5u : 2u, DRAW_NONE, 0, 0, false }; // two XCD ids, unevenly manned
	}
	u32 left = n_workgroups;
	unsigned long long events = 0, handed = 0, waits = 0;
	const unsigned long long limit = 64 * (want + n_units + n_workgroups) + 100000; // far beyond what a terminating play takes
	u32 rng = seed;
	while (left && events < limit) {
		rng = rng * 1664525u + 1013904223u;
		if (!c.pending.empty() && (rng >> 28) < 3) {
			c.land((rng >> 8) % c.pending.size()); // (a delayed store reaches the control words)
			continue;
		}
		Workgroup& w = wg[(rng >> 8) % n_workgroups];
		if (w.done) {
			continue;
		}
		events++;
		c.owner = (u32)(&w - wg.data());
		const u32 r = probe_claim_try(c, w.xcd, n_units, plog, n_wg, w.sl, w.p, w.total);
		if (r == CLAIM_WAIT) {
			waits++;
			continue;
		}
		if (r == CLAIM_DONE) {
			w.done = true;
			left--;
			continue;
		}
		expect(w.sl < n_units && w.p < w.total && w.total == draw_total(n_wg, longest[w.sl >> plog]), "a draw inside its pair", w.sl, w.p, w.total);
		if (w.sl < n_units) {
			for (u32 wave = 0; wave < (u32)PROBE_WAVES; wave++) {
				const u32 at = w.p + wave * PROBE_STEP;
				if (at < w.total && at / PROBE_STEP < seen[w.sl].size()) {
					seen[w.sl][at / PROBE_STEP]++;
					handed++;
				}
			}
			w.p = c.add(CTL_WORK + w.sl, PROBE_DRAW); // (the draw made ahead; program order: the claim's store lands first)
		}
	}
	expect(left == 0, "termination", left, (unsigned)events, n_workgroups);
	g_waits += waits;
	for (u32 u = 0; u < n_units; u++) {
		for (size_t i = 0; i < seen[u].size(); i++) {
			expect(seen[u][i] == 1, "every unit of every pair once", u, (unsigned)i, seen[u][i]);
		}
	}
	std::printf("claim slices %u parts %u n_wg %u workgroups %u: units %llu handed %llu events %llu waits %llu mismatches %llu\n", n_slices,
	            1u << plog, n_wg, n_workgroups, want, handed, events, waits, g_mismatches - before);
}

static int
selftest()
{
	const u32 n_wgs[] = { 1, 7, 11, 256 };
	const u32 longests[] = { 0, 1, 511, 512, 513, 17184 };
	for (u32 n_wg : n_wgs) {
		for (u32 l : longests) {
			coords_case(n_wg, l);
		}
	}
	// slices that got no record at all among short and long ones, at the list's ends and in a row
	const std::vector<u32> mixed = { 0, 513, 0, 0, 17184, 1, 512, 0, 0, 511, 8, 0 };
	const std::vector<u32> empty(9, 0);
	const std::vector<u32> one = { 0 };
	u32 seed = 1;
	for (u32 n_wg : { 1u, 7u, 11u, 256u }) {
		for (u32 plog : { 0u, 1u, 2u }) {
			for (u32 n_workgroups : { 1u, 2u, 5u, 64u }) {
				claim_case(mixed, n_wg, plog, n_workgroups, seed++);
			}
		}
		claim_case(empty, n_wg, 0, 7, seed++);
		claim_case(one, n_wg, 1, 3, seed++);
	}
	expect(g_waits > 0, "the wait path ran", (unsigned)g_waits, 0, 0);
	std::printf("waits %llu\n", g_waits);
	std::printf("mismatches %llu\n", g_mismatches);
	return g_mismatches ? 1 : 0;
}

int
main(int argc, char** argv)
{
	if (argc == 2 && !std::strcmp(argv[1], "selftest")) {
		return selftest();
	}
	std::fprintf(stderr, "usage: draw_host selftest\n");
	return 2;
}
