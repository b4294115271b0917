// nte_settle.h -- settle_event(): the whole outcome of a plain substitution event, as a fixed function.
//
// Most events of a draft with scattered errors are the same thing: one wrong base in otherwise clean sequence (the
// shares measured on the bench drafts: DESIGN.md 8, experiment 65).
// The machine (nte_machine.h) confirms the k-mer on the subset (step 2), finds the one candidate base whose k-mers are
// there, applies it, rolls through the k - 1 k-mers that hold the new base -- all present -- and stops, clean again, at
// the first position behind them.  What it leaves is one arena chunk of four items.  settle_event() computes exactly
// that from 2k draft bytes, a few bitmap words and the filter, without rope, overlay or cursors, and only where the
// machine's walk is that fixed function: it accepts an event iff (s = start + k - 1)
//   a. room        start + 2k + max_deletions + 2 <= len: the windows of the failing position and of the look-ahead
//                  behind its edit are full (Machine::fill_window, clean and general form); the contig-end paths
//                  stay the machine's
//   b. characters  seq[s] is exactly A, C, G or T (the revert of a lower-case or IUPAC base writes the UPPER-cased
//                  draft base back: extra TAG_MOD items), and no byte of seq[start .. start + 2k - 1] is a
//                  non-accepted one (step 2 gives the position up; the advance skips over such k-mers)
//   c. step 2      absent_count_stride(bitmap, gbase + start + 1, k, jump) >= thr_missing
//   d. candidates  in candidate_bases order: a candidate whose own k-mer is there is counted on the rolls
//                  kk = 0, jump, 2 jump, ... <= k - 1 (the roll kk == k - 1 drops the new base, process_missing);
//                  support >= thr_edit -> note_candidate; a present candidate below the bar declines the event when
//                  none has been accepted before it (the machine starts an indel sweep there) and is ignored
//                  otherwise; afterwards edit_type == 1
//   e. look-ahead  the k - 1 k-mers start + 1 .. start + k - 1 with the winning base are all present (else the machine
//                  assesses a failing position in a state that is not clean)
//   f. end         at g = gbase + start + k: !bit_absent(runmap, g) || is_event_start(runmap, g, start_grid): the
//                  machine, clean again, stops there; cover end = start + k
// and declines -- writing nothing -- everywhere else: a declined event goes through the machine, which stays the
// reference (tests/settle/settle_host.cpp runs every event through both).
// Configurations: settle_applicable().  The arithmetic is the machine's own (hash_roll, hash_changelast, the grouped
// level-by-level probe, candidate_bases, note_candidate); only make_edit's packing of the TAG_SUB item, a member that
// works on the rope, is restated.
#pragma once
#include "nte_machine.h"

namespace nte {

// plain primary filter, no secondary one, no -s 1, -m 0 without -a: the machine that configuration runs
typedef MachineT<CFG_MODE0 | CFG_PLAIN | CFG_NOSEC> SettleMachine;

constexpr u32 SETTLE_MAX_K = 64; // the presence of a candidate's k rolls is one 64-bit mask

// the configurations settle_event() restates the machine for
inline bool
settle_applicable(const DevParams& p, const Filter& bloom)
{
	return !bloom.counting && !p.counting && !p.secbf && !p.snv && p.mode == 0 && !p.mask && p.debug_stop == 0 && p.k >= 2 && p.k <= SETTLE_MAX_K &&
	       (p.event_budget == 0 || p.event_budget > p.k + 2);
}

struct SettleOut
{
	Item item[4];  // link, header, TAG_MOD, TAG_SUB: the event's arena chunk as emit / make_edit case 1 / finish leave it
	u32 cover_end; // start + k
};

// e.win / e.win_stride: 2k bytes of window storage (the codes of seq[start .. start + 2k - 1]); G: k-mers probed together
template<int G>
NTE_HD bool
settle_event_on(SettleMachine& m, u32 start, SettleOut& out)
{
	const EventEnv& e = m.e;
	const DevParams& p = m.p;
	const u32 k = p.k;
	const u32 s = start + k - 1;
	// a. room
	if ((u64)start + 2 * (u64)k + p.max_deletions + 2 > e.len) {
		return false;
	}
	// c. step 2, f. end: bitmap words only
	if (absent_count_stride(e.bitmap, e.gbase + start + 1, k, p.jump) < p.thr_missing) {
		return false;
	}
	const u64 g_end = e.gbase + start + k;
	if (bit_absent(e.runmap, g_end) && !is_event_start(e.runmap, g_end, p.start_grid)) {
		return false;
	}
	// b. characters: the window in aligned 8-byte words, as fill_window reads it
	const u8 draft_char = e.seq[s];
	if (draft_char != 'A' && draft_char != 'C' && draft_char != 'G' && draft_char != 'T') {
		return false;
	}
	{
		const u32 want = 2 * k;
		const u64 g0 = e.gbase + start;
		const u8* base = e.seq - e.gbase; // batch buffer start (16-byte aligned)
		const u64 a0 = g0 & ~7ULL;
		u32 filled = 0;
		u32 skip = (u32)(g0 - a0);
		bool bad = false;
		for (u64 a = a0; filled < want; a += 8) {
			u64 w = 0;
			if (base + a + 8 <= e.batch_end) {
				w = *reinterpret_cast<const u64*>(base + a);
			} else {
				for (u32 b = 0; b < 8 && base + a + b < e.batch_end; b++) {
					w |= (u64)base[a + b] << (8 * b);
				}
			}
			w >>= 8 * skip;
			for (u32 b = skip; b < 8 && filled < want; b++) {
				const u8 code = char_code((u8)(w & 0xFF));
				bad |= code == CODE_BAD;
				e.win[(u64)filled * e.win_stride] = code;
				w >>= 8;
				filled++;
			}
			skip = 0;
		}
		if (bad) {
			return false;
		}
	}
	m.win_off = 0;
	const HashState hs = m.seed_from_window();
	const u8 draft_code = char_code(draft_char);

	// d. candidates: their own k-mers first, together
	u8 cand[MAX_CANDIDATES];
	const u32 n_cand = SettleMachine::candidate_bases(draft_char, false, cand);
	u64 cb[MAX_CANDIDATES];
	NTE_UNROLL
	for (int ci = 0; ci < (int)MAX_CANDIDATES; ci++) {
		cb[ci] = 0;
		if ((u32)ci < n_cand) {
			HashState t = hs;
			hash_changelast(t, e.tab, draft_code, char_code(cand[ci]));
			cb[ci] = t.fh + t.rh;
		}
	}
	const u32 there = m.template probe_group<(int)MAX_CANDIDATES>(e.bloom, cb, n_cand);
	if (!there) {
		return false;
	}
	u64 subset = 0; // rolls that count for the support
	for (u32 kk = 0; kk < k; kk += p.jump) {
		subset |= 1ULL << kk;
	}
	Best b;
	b.edit_type = 0;
	b.n_indel = 0;
	b.sub_base = 0;
	b.num_support = 0;
	b.altbase1 = b.altbase2 = b.altbase3 = 0;
	b.altsupp1 = b.altsupp2 = b.altsupp3 = 0;
	u64 best_pm = 0; // presence of the winning candidate's rolls 0 .. k - 1
	NTE_UNROLL
	for (int ci = 0; ci < (int)MAX_CANDIDATES; ci++) {
		if ((u32)ci >= n_cand || !((there >> ci) & 1)) {
			continue;
		}
		const u8 sub_code = char_code(cand[ci]);
		HashState t = hs;
		hash_changelast(t, e.tab, draft_code, sub_code);
		u64 pm = 0;
		u32 kk = 0, support = 0;
		bool short_of_bar = false;
		while (kk < k) {
			u64 hb[G];
			const u32 kk0 = kk;
			NTE_UNROLL
			for (int u = 0; u < G; u++) {
				hb[u] = 0;
				if (kk0 + (u32)u < k) {
					// (the substituted base is the last one to leave the window)
					hash_roll(t, e.tab, kk == k - 1 ? sub_code : m.win_o(kk), m.win_i(kk));
					hb[u] = t.fh + t.rh;
					kk++;
				}
			}
			pm |= (u64)m.template probe_group<G>(e.bloom, hb, kk - kk0) << kk0;
			const u64 counted = pm & subset;
			support = SettleMachine::popc32((u32)counted) + SettleMachine::popc32((u32)(counted >> 32));
			const u64 ahead = kk < 64 ? subset >> kk : 0;
			if (support + SettleMachine::popc32((u32)ahead) + SettleMachine::popc32((u32)(ahead >> 32)) < p.thr_edit) {
				short_of_bar = true; // the bar is out of reach (subset_scan gives up the same way: support counts as 0)
				break;
			}
		}
		if (!short_of_bar && support >= p.thr_edit) {
			SettleMachine::note_candidate(b, cand[ci], support);
			if (b.sub_base == cand[ci]) {
				best_pm = pm;
			}
		} else if (b.edit_type != 1) {
			return false; // the machine sweeps indel candidates here
		}
	}
	if (b.edit_type != 1) {
		return false;
	}
	// e. look-ahead
	const u64 la = (1ULL << (k - 1)) - 1;
	if ((best_pm & la) != la) {
		return false;
	}

	// the outcome: emit (first chunk: link + header), make_edit case 1 (set_seq -> TAG_MOD, then TAG_SUB), finish
	out.item[0].w[0] = NONE32;
	out.item[0].w[1] = 4;
	out.item[0].w[2] = out.item[0].w[3] = 0;
	out.item[1].w[0] = e.contig;
	out.item[1].w[1] = start;
	out.item[1].w[2] = start + k;
	out.item[1].w[3] = 0;
	out.item[2].w[0] = TAG_MOD | ((u32)b.sub_base << 8);
	out.item[2].w[1] = s;
	out.item[2].w[2] = out.item[2].w[3] = 0;
	u8 a1 = 0, a2 = 0, a3 = 0;
	u32 s1 = 0, s2 = 0, s3 = 0;
	if (b.altsupp1 && b.altbase1 != b.sub_base) {
		a1 = b.altbase1;
		s1 = b.altsupp1;
	}
	if (b.altsupp2 && b.altbase2 != b.altbase1) {
		a2 = b.altbase2;
		s2 = b.altsupp2;
	}
	if (b.altsupp3 && b.altbase3 != b.altbase2) {
		a3 = b.altbase3;
		s3 = b.altsupp3;
	}
	out.item[3].w[0] = TAG_SUB | ((u32)draft_char << 8) | ((u32)b.sub_base << 16) | ((b.num_support & 0xFF) << 24);
	out.item[3].w[1] = s;
	out.item[3].w[2] = (u32)a1 | ((s1 & 0xFF) << 8) | ((u32)a2 << 16) | ((s2 & 0xFF) << 24);
	out.item[3].w[3] = (u32)a3 | ((s3 & 0xFF) << 8);
	out.cover_end = start + k;
	return true;
}

// inputs: the event's seq, len, gbase, contig, bitmap, runmap, tab, p, bloom (and the window storage) of e, and start
template<int G = 8>
NTE_HD bool
settle_event(const EventEnv& e, u32 start, SettleOut& out)
{
	SettleMachine m(e);
	return settle_event_on<G>(m, start, out);
}

} // namespace nte
