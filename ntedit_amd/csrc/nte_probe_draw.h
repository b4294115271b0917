// nte_probe_draw.h -- how the probe stage (k_bin_probe, nte_kernels.hip) hands out a slice's records: the coordinates of
// a draw and the order of events by which the workgroups of an XCD move from slice to slice, each stated once.
//
//   the step    PROBE_STEP = 512 records of ONE run: what a wavefront probes at a time
//   the draw    PROBE_DRAW = 8 steps: what a workgroup takes from its slice's counter at a time, one step per wavefront
//   the order   step-major: a slice's counter enumerates steps with the RUN index fastest -- unit u is step u / n_wg of
//               run u % n_wg -- and ends behind the last step of the slice's LONGEST run (the partition kernel's drain
//               leaves it in longest[slice]).  The eight wavefronts of a draw work on the same step of eight runs and are
//               equally full; steps are empty only where a run is shorter than the longest of its slice.  (Run-major, over
//               runs of `cap` records rounded up to whole steps, left the steps between a run's fill and its cap -- four
//               of 38 at 3 Gbp -- next to each other: every tenth draw was empty and four in ten were half empty.)
//   the claim   probe_claim_try: one thread's next draw from its XCD's current slice; the workgroup whose draw reaches the
//               end of a slice opens the next one.  A slice therefore hands out at least ONE draw, however short its runs:
//               a slice without a draw would never be closed and its XCD would wait for ever (draw_total's max(1, ..)).
//
// Includes nte_common.h and nothing of the context; compiles under hipcc and under a plain host compiler
// (tests/draw/draw_host.cpp plays the workgroups of two XCDs one event at a time).  The control words are reached
// through a policy class (add, cas, load, store on ctl[], longest(slice)): device atomics in nte_kernels.hip, plain
// words on the host.
#pragma once
#include "nte_common.h"

#if defined(__HIPCC__)
#define NTE_DEV __device__ __forceinline__
#else
#define NTE_DEV inline
#endif

namespace nte {

#ifndef NTE_PROBE_TPB
#define NTE_PROBE_TPB 512
#endif
constexpr int PROBE_TPB = NTE_PROBE_TPB;
constexpr int PROBE_WAVES = PROBE_TPB / 64;
#ifndef NTE_PROBE_PER
#define NTE_PROBE_PER 8
#endif
constexpr int PROBE_PER = NTE_PROBE_PER;      // records per lane and step, all in flight together
constexpr int PROBE_STEP = 64 * PROBE_PER;    // records per step of a wavefront
constexpr u32 PROBE_DRAW = PROBE_STEP * PROBE_WAVES; // records per draw of a workgroup
// ctl[] (zeroed before every record chunk): [0] next unclaimed slice, [1..16] current slice of XCD x (0 = none yet,
// 1 = being claimed, s + 2 = slice s), [32 + s] records of slice s handed out so far, in the counter's coordinates
constexpr u32 CTL_NEXT = 0, CTL_CUR = 1, CTL_WORK = 32;
constexpr u32 DRAW_NONE = 0xFFFFFFFFu;

// the end of a slice's counter: n_wg runs x the steps of its longest run, at least one
NTE_HD u32
draw_total(u32 n_wg, u32 longest)
{
	const u32 steps = (longest + PROBE_STEP - 1) / PROBE_STEP;
	return n_wg * (u32)PROBE_STEP * (steps ? steps : 1u);
}

// counter coordinate `at` (a multiple of PROBE_STEP below the slice's total) -> the run and the first record in it
NTE_HD void
draw_unit(u32 at, u32 n_wg, u32& run, u32& i0)
{
	const u32 u = at / PROBE_STEP;
	const u32 step = u / n_wg;
	run = u - step * n_wg;
	i0 = step * PROBE_STEP;
}

// One thread: the next stretch [p, p + PROBE_DRAW) of the XCD's current (slice, part) pair, moving on to further pairs
// as they run out.  On entry {sl, p, total} is a draw already made from pair `sl`, whose counter ends at `total` (or
// sl == DRAW_NONE: none yet).  CLAIM_WAIT: another workgroup is switching the XCD's pair right now -- call again.
constexpr u32 CLAIM_DRAW = 0, CLAIM_DONE = 1, CLAIM_WAIT = 2;
template<class Ctl>
NTE_DEV u32
probe_claim_try(Ctl& c, u32 xcd, u32 n_units, u32 plog, u32 n_wg, u32& sl, u32& p, u32& total)
{
	const u32 cur = CTL_CUR + xcd;
	for (;;) {
		if (sl != DRAW_NONE && p < total) {
			if (total - p <= PROBE_DRAW) {
				// this draw reaches the end of the pair: open the next one for the whole XCD
				const u32 nx = c.add(CTL_NEXT, 1u);
				c.store(cur, nx + 2);
			}
			return CLAIM_DRAW;
		}
		// the XCD's current pair (another workgroup may be switching it right now)
		const u32 v = c.load(cur);
		if (v == 0) {
			if (c.cas(cur, 0u, 1u) == 0u) {
				const u32 nx = c.add(CTL_NEXT, 1u);
				c.store(cur, nx + 2);
			}
			continue;
		}
		if (v == 1 || v - 2 == sl) {
			return CLAIM_WAIT;
		}
		sl = v - 2;
		if (sl >= n_units) {
			return CLAIM_DONE;
		}
		total = draw_total(n_wg, c.longest(sl >> plog)); // (every part of a slice walks the slice's runs)
		p = c.add(CTL_WORK + sl, PROBE_DRAW);
	}
}

} // namespace nte

#undef NTE_DEV
