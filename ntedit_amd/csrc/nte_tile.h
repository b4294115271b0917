// nte_tile.h -- "every k-mer of a batch, tile by tile": the rules the per-k-mer kernels share, each stated once.
//
//   the tile       256 threads x 64 consecutive k-mer starts; its bytes (+ k - 1 halo) parked in LDS as one code per byte,
//                  rows of 64 codes padded to 68 bytes (tile_phys)
//   the prologue   seed tables and the byte -> code look-up table into LDS (tile_load_tabs, tile_fill_lut)
//   the staging    16-byte loads, bytes past the batch as '\n', the table applied (tile_stage)
//   the walk       a thread's rolling hash over its stream: prime from k codes, roll one start, fh + rh, "k good codes"
//                  (TileWalk), fed a byte at a time (roll_bytes) or four starts per LDS word (TileQuad)
//   the packed tile  two 4-bit codes per byte: twice the starts in the same LDS (tile_stage_packed, tile_prime_packed, and
//                  TileOct, eight starts per LDS word), for the partition kernel's 1,024 threads x 32 starts
//   the entries    of a batch: the first entry whose end lies behind a position (entry_behind), a stream's cursor along
//                  them (EntryCursor), the bits of a word (bit_range)
//   byte_sat_inc   saturating +1 of a byte counter
//
// Users: k_screen, k_mark, k_spectrum (nte_kernels.hip), k_cn_count, k_spectrum_cn (nte_cn.hip), the reads passes
// (nte_reads.hip), the entries alone in nte_apply.hip and nte_track.hip, the packed tile in nte_bin_wc.inc.
// What a kernel gathers, its histograms and row flushes, and every barrier stay in the kernel: nothing here synchronises
// or reads threadIdx, and all state is a handful of registers (no array indexed by a run-time value).
// Includes nte_common.h and nothing of the context; compiles under hipcc and under a plain host compiler
// (tests/tile/tile_host.cpp and tile_packed_host.cpp play a workgroup's threads one after the other).
#pragma once
#include "nte_common.h"

#if defined(__HIPCC__)
#define NTE_DEV __device__ __forceinline__
#else
#define NTE_DEV inline
#endif

namespace nte {

// ---------------------------------------------------------------- the tile
// Rows of 64 codes are padded to 68 bytes so that the per-thread streams (lane stride = one row) hit 32 different banks.
// The halo is sized for k <= TILE_MAXK whatever limit a caller's API sets below that: one LDS size for every kernel.
constexpr int TILE_TPB = 256;
constexpr int TILE_L = 64;
constexpr int TILE_STARTS = TILE_TPB * TILE_L;
constexpr int TILE_MAXK = 256;
constexpr int TILE_LDS_BYTES = ((TILE_STARTS + TILE_MAXK + 63) / 64) * 68 + 16;

// 16 bytes of the batch: one load
struct __attribute__((aligned(16))) TileChunk
{
	u32 w[4];
};

NTE_DEV u32
tile_phys(u32 x)
{
	return x + ((x >> 6) << 2);
}

// the look-up table's entry of a byte: all IUPAC codes (the screening), or -- acgt_only -- a code above 3 ends a k-mer
// (the filter builds, marks, spectra, reads)
NTE_DEV u8
tile_lut_code(u8 byte, bool acgt_only)
{
	const u8 code = char_code(byte);
	return acgt_only && code > 3 ? CODE_BAD : code;
}

// ---------------------------------------------------------------- prologue (a barrier follows in the kernel)
NTE_DEV void
tile_load_tabs(const u64* __restrict__ tabs, u64* s_tab, u32 tid)
{
	if (tid < TAB_WORDS) {
		s_tab[tid] = tabs[tid];
	}
}

// one entry per thread: a workgroup of TILE_TPB = 256 threads fills the table
NTE_DEV void
tile_fill_lut(u8* s_lut, bool acgt_only, u32 tid)
{
	s_lut[tid] = tile_lut_code((u8)tid, acgt_only);
}

// ---------------------------------------------------------------- staging (a barrier follows in the kernel)
// tile_len starts from tile_base (a multiple of 16) + the k - 1 halo, as codes in s_codes; seq is 16-byte aligned
NTE_DEV void
tile_stage(const u8* __restrict__ seq, u64 n, u64 tile_base, u32 tile_len, u32 k, const u8* s_lut, u8* s_codes, u32 tid, u32 tpb)
{
	const u32 n_chunks = (tile_len + k - 1 + 15) / 16;
	for (u32 c = tid; c < n_chunks; c += tpb) {
		const u64 g = tile_base + (u64)c * 16;
		u32 w[4];
		if (g + 16 <= n) {
			const TileChunk v = *reinterpret_cast<const TileChunk*>(seq + g);
			w[0] = v.w[0];
			w[1] = v.w[1];
			w[2] = v.w[2];
			w[3] = v.w[3];
		} else {
			NTE_UNROLL
			for (int q = 0; q < 4; q++) {
				u32 x = 0;
				NTE_UNROLL
				for (int b = 0; b < 4; b++) {
					const u64 gg = g + q * 4 + b;
					const u32 ch = gg < n ? seq[gg] : (u32)'\n';
					x |= ch << (8 * b);
				}
				w[q] = x;
			}
		}
		NTE_UNROLL
		for (int q = 0; q < 4; q++) {
			const u32 x = w[q];
			const u32 codes = (u32)s_lut[x & 0xFF] | ((u32)s_lut[(x >> 8) & 0xFF] << 8) |
			                  ((u32)s_lut[(x >> 16) & 0xFF] << 16) | ((u32)s_lut[x >> 24] << 24);
			*reinterpret_cast<u32*>(&s_codes[tile_phys(c * 16 + q * 4)]) = codes;
		}
	}
}

// ---------------------------------------------------------------- the walk
// The hash state is exact once k good codes have entered since the last CODE_BAD (a CODE_BAD has zero seeds both ways, so
// it leaves nothing behind).  After prime() the state is that of the start x0; every roll moves one start on.
struct TileWalk
{
	HashState hs;
	u32 good, x0, k;

	NTE_DEV void
	prime(const u8* s_codes, const u64* s_tab, u32 x0_, u32 k_)
	{
		hs = HashState{ 0, 0 };
		good = 0;
		x0 = x0_;
		k = k_;
		for (u32 i = 0; i < k; i++) {
			roll(s_tab, CODE_BAD, s_codes[tile_phys(x0 + i)]);
		}
	}

	NTE_DEV void
	roll(const u64* s_tab, u8 out, u8 in)
	{
		hash_roll(hs, s_tab, out, in);
		good = in == CODE_BAD ? 0 : good + 1;
	}

	// the byte reader: from start x0 + j to the next
	NTE_DEV void
	roll_bytes(const u8* s_codes, const u64* s_tab, u32 j)
	{
		roll(s_tab, s_codes[tile_phys(x0 + j)], s_codes[tile_phys(x0 + j + k)]);
	}

	// start u of the four a TileQuad read
	NTE_DEV void
	roll_quad(const u64* s_tab, u32 outw, u32 inw, int u)
	{
		roll(s_tab, (u8)((outw >> (8 * u)) & 0xFF), (u8)((inw >> (8 * u)) & 0xFF));
	}

	NTE_DEV u64
	base() const // the canonical hash every probe is extended from
	{
		return hs.fh + hs.rh;
	}

	NTE_DEV bool
	valid() const // k codes of the table's alphabet under the cursor
	{
		return good >= k;
	}
};

// The four-start reader: one LDS word per four starts for each of the two streams.  The codes that enter at starts
// j0 .. j0 + 3 are bytes x0 + j0 + k .. + 3: funnelled out of two aligned words, the upper of which is carried into the
// next read.  (With k % 4 == 0 the upper word is read and not used; at k = TILE_MAXK the last one lies behind what the
// staging wrote, inside TILE_LDS_BYTES.  So does, with either reader and k = 1 mod 16, the code the last thread's last
// roll takes in: that roll's state is never read.)
// The guard of the funnel is written on k & 3, not on ksh: tested on ksh the compiler folds select and shifts into one
// v_alignbit_b32, which moves every user's register allocation.
struct TileQuad
{
	u32 in_lo, ksh;

	NTE_DEV void
	begin(const u8* s_codes, const TileWalk& w) // (w primed: the stream and k are the walk's)
	{
		ksh = (w.k & 3) * 8;
		in_lo = *reinterpret_cast<const u32*>(&s_codes[tile_phys((w.x0 + w.k) & ~3u)]);
	}

	NTE_DEV void
	read(const u8* s_codes, const TileWalk& w, u32 j0, u32& outw, u32& inw)
	{
		outw = *reinterpret_cast<const u32*>(&s_codes[tile_phys(w.x0 + j0)]);
		const u32 in_hi = *reinterpret_cast<const u32*>(&s_codes[tile_phys(((w.x0 + j0 + w.k) & ~3u) + 4)]);
		inw = (w.k & 3) ? ((in_lo >> ksh) | (in_hi << (32 - ksh))) : in_lo;
		in_lo = in_hi;
	}
};

// ---------------------------------------------------------------- the packed tile
// Codes are 4 bits (CODE_BAD = 15): two per byte, the even start in the low nibble, hold twice the starts in the same
// LDS -- TILE_PACKED_STARTS + the TILE_MAXK halo are 16,512 bytes, 17,560 with the row padding, inside TILE_LDS_BYTES.
// A thread of 32 consecutive starts begins 16 bytes behind its neighbour, as a thread of 16 starts does in the byte
// form, so tile_phys and its bank pattern stay.  User: k_wc_scatter_b (nte_bin_wc.inc); tests/tile/tile_packed_host.cpp
// plays it against the byte walk.
constexpr int TILE_PACKED_STARTS = 2 * TILE_STARTS;
constexpr int TILE_PACKED_BYTES = (TILE_PACKED_STARTS + 8 + TILE_MAXK + 15) / 16 * 8; // staged, before the row padding
static_assert(TILE_PACKED_BYTES + TILE_PACKED_BYTES / 64 * 4 + 8 <= TILE_LDS_BYTES, "the packed tile (and the word the last read takes) fits the byte tile's LDS");

NTE_DEV u32
tile_pack4(const u8* s_lut, u32 x) // the codes of four bytes, 16 bits
{
	return (u32)s_lut[x & 0xFF] | ((u32)s_lut[(x >> 8) & 0xFF] << 4) | ((u32)s_lut[(x >> 16) & 0xFF] << 8) | ((u32)s_lut[x >> 24] << 12);
}

// tile_stage in the packed form: code x of the tile is nibble x & 1 of byte tile_phys(x >> 1)
NTE_DEV void
tile_stage_packed(const u8* __restrict__ seq, u64 n, u64 tile_base, u32 tile_len, u32 k, const u8* s_lut, u8* s_codes, u32 tid, u32 tpb)
{
	const u32 n_chunks = (tile_len + k - 1 + 15) / 16;
	for (u32 c = tid; c < n_chunks; c += tpb) {
		const u64 g = tile_base + (u64)c * 16;
		u32 w[4];
		if (g + 16 <= n) {
			const TileChunk v = *reinterpret_cast<const TileChunk*>(seq + g);
			w[0] = v.w[0];
			w[1] = v.w[1];
			w[2] = v.w[2];
			w[3] = v.w[3];
		} else {
			NTE_UNROLL
			for (int q = 0; q < 4; q++) {
				u32 x = 0;
				NTE_UNROLL
				for (int b = 0; b < 4; b++) {
					const u64 gg = g + q * 4 + b;
					const u32 ch = gg < n ? seq[gg] : (u32)'\n';
					x |= ch << (8 * b);
				}
				w[q] = x;
			}
		}
		NTE_UNROLL
		for (int q = 0; q < 2; q++) {
			*reinterpret_cast<u32*>(&s_codes[tile_phys(c * 8 + q * 4)]) = tile_pack4(s_lut, w[2 * q]) | (tile_pack4(s_lut, w[2 * q + 1]) << 16);
		}
	}
}

NTE_DEV u32
tile_packed_word(const u8* s_codes, u32 x) // the eight codes x .. x + 7 (x a multiple of 8)
{
	return *reinterpret_cast<const u32*>(&s_codes[tile_phys(x >> 1)]);
}

// prime a walk from the packed tile (x0 a multiple of 8): as TileWalk::prime, eight codes per LDS word
NTE_DEV void
tile_prime_packed(TileWalk& w, const u8* s_codes, const u64* s_tab, u32 x0, u32 k)
{
	w.hs = HashState{ 0, 0 };
	w.good = 0;
	w.x0 = x0;
	w.k = k;
	for (u32 i = 0; i < k; i += 8) {
		const u32 w8 = tile_packed_word(s_codes, x0 + i);
		NTE_UNROLL
		for (u32 b = 0; b < 8; b++) {
			if (i + b < k) {
				w.roll(s_tab, CODE_BAD, (u8)((w8 >> (4 * b)) & 15u));
			}
		}
	}
}

// The eight-start reader: TileQuad on nibbles.  The codes that enter at starts j0 .. j0 + 7 (x0 and j0 multiples of 8) are
// nibbles x0 + j0 + k .. + 7: funnelled out of two aligned words by k & 7 nibbles, the upper word carried into the next
// read.  (With k % 8 == 0 the upper word is read and not used; at k = TILE_MAXK the last one lies behind what the staging
// wrote, inside TILE_LDS_BYTES.)
struct TileOct
{
	u32 in_lo, ksh;

	NTE_DEV void
	begin(const u8* s_codes, const TileWalk& w)
	{
		ksh = (w.k & 7) * 4;
		in_lo = tile_packed_word(s_codes, (w.x0 + w.k) & ~7u);
	}

	NTE_DEV void
	read(const u8* s_codes, const TileWalk& w, u32 j0, u32& outw, u32& inw)
	{
		outw = tile_packed_word(s_codes, w.x0 + j0);
		const u32 in_hi = tile_packed_word(s_codes, ((w.x0 + j0 + w.k) & ~7u) + 8);
		inw = (w.k & 7) ? ((in_lo >> ksh) | (in_hi << (32 - ksh))) : in_lo;
		in_lo = in_hi;
	}

	// start u of the eight that were read
	static NTE_DEV void
	roll(TileWalk& w, const u64* s_tab, u32 outw, u32 inw, u32 u)
	{
		w.roll(s_tab, (u8)((outw >> (4 * u)) & 15u), (u8)((inw >> (4 * u)) & 15u));
	}
};

// ---------------------------------------------------------------- the entries of a batch
// bits [lo, hi) of a word, 0 <= lo <= hi <= 64
NTE_DEV u64
bit_range(u32 lo, u32 hi)
{
	if (hi <= lo) {
		return 0;
	}
	const u64 upto = hi >= 64 ? ~0ULL : (1ULL << hi) - 1;
	return upto & ~((1ULL << lo) - 1);
}

// the first entry whose end lies behind position x (entries are in batch order)
NTE_DEV u32
entry_behind(const u64* __restrict__ offs, const u32* __restrict__ lens, u32 n, u64 x)
{
	u32 lo = 0, hi = n;
	while (lo < hi) {
		const u32 mid = (lo + hi) >> 1;
		if (offs[mid] + lens[mid] <= x) {
			lo = mid + 1;
		} else {
			hi = mid;
		}
	}
	return lo;
}

// The entry of a stream's position: [eb, ee), both ~0 behind the last entry (then nothing is a k-mer).  Entries may abut
// (no separator: the entry's bounds end a k-mer, not the byte) and may be shorter than k or empty.
struct EntryCursor
{
	u32 e;
	u64 eb, ee;

	NTE_DEV void
	load(const u64* __restrict__ offs, const u32* __restrict__ lens, u32 n_entries)
	{
		eb = ee = ~0ULL;
		if (e < n_entries) {
			eb = offs[e];
			ee = eb + lens[e];
		}
	}

	NTE_DEV void
	start(const u64* __restrict__ offs, const u32* __restrict__ lens, u32 n_entries, u64 pos)
	{
		e = entry_behind(offs, lens, n_entries, pos);
		load(offs, lens, n_entries);
	}

	// positions only grow along a stream
	NTE_DEV void
	advance(const u64* __restrict__ offs, const u32* __restrict__ lens, u32 n_entries, u64 pos)
	{
		while (pos >= ee) { // (ee = ~0 behind the last entry: the loop ends there)
			e++;
			load(offs, lens, n_entries);
		}
	}

	// does a k-mer that starts at pos lie inside the entry
	NTE_DEV bool
	holds(u64 pos, u32 k) const
	{
		return pos >= eb && pos + k <= ee;
	}
};

// ---------------------------------------------------------------- byte_sat_inc
// Saturating +1 of byte s of a counter array: a plain read of the containing word, the compare-and-swap only while the
// byte is below 255 (gfx950 has no byte atomics).  Counters only grow, so a stale read costs at most one more round; a
// satellite k-mer repeated a million times is answered from L2 after its 255th occurrence instead of serialising on one
// line.  (On the host, one thread: the compare-and-swap is a plain compare.)
NTE_DEV void
byte_sat_inc(u32* words, u64 s)
{
	u32* w = words + (s >> 2);
	const u32 sh = (u32)(s & 3) * 8;
#if defined(__HIPCC__)
	u32 old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	while (((old >> sh) & 0xFFu) != 0xFFu) {
		const u32 prev = atomicCAS(w, old, old + (1u << sh));
		if (prev == old) {
			break;
		}
		old = prev;
	}
#else
	if (((*w >> sh) & 0xFFu) != 0xFFu) {
		*w += 1u << sh;
	}
#endif
}

} // namespace nte

#undef NTE_DEV
