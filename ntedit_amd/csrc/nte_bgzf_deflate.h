// nte_bgzf_deflate.h -- one BGZF member written on the device, written once: a block of 1 to 65,280 plain bytes into
// one complete member (gzip header with the 'BC' subfield, one final DEFLATE block, CRC-32, ISIZE).  The deflate
// kernel (nte_bgzf_deflate.hip) and the serial host model (ntedit_hip_bgzf_deflate_model, same unit) are both built
// from these functions, as nte_bgzf_inflate.h serves the inflate kernel and its model.
//
// The DEFLATE block is literal-only: a dynamic Huffman code over the block's byte values and the end-of-block symbol,
// no matches, an empty distance set (HDIST names one code of length 0).  A draft is four letters, so such a block
// holds it at a little over two bits per base and needs no LZ77 search.  Where the dynamic block is not smaller than
// a stored one (random bytes, uniform byte values) the stored block is written: a member is at most 31 + 65,280 bytes.
//
// Every function takes (lane, lanes); the kernel calls them with (lane, 64), the model with (0, 1).  What steers the
// encoder -- histogram, code lengths, codes, header, sizes -- is integer work on the block's bytes alone, with ties
// broken by symbol value: the member is a function of the block's bytes, whatever the lanes and the order in which
// LDS atomics land (they only add counts and OR bits, both commutative).  The stages:
//   histogram   four bytes per lane and step; per byte position of the step up to DZ_BALLOTS rounds of "the first
//               pending lane's value, a ballot of the lanes that hold it, one add of its popcount", so the four letters
//               of a draft cost four adds per 64 bytes and no two lanes meet on an address; lanes still pending after
//               those rounds (text, random bytes: many distinct values) add 1 each with an LDS atomic
//   lengths     symbols ranked by (count, symbol) in parallel, each lane its share of the symbols; then one lane: the
//               Huffman tree by the two-queue method over the ranked leaves, the leaves counted per depth, depths over the
//               limit folded into it and the Kraft sum brought back to exactly 1 by moving one code a level down per unit
//               of excess (integer counts only), lengths handed out by rank.  Limit 15 for the literals, 7 for the
//               code-length code.  A set with one used symbol gets a second code of length 1: always complete.
//   header      the 258 lengths (257 literal/length + 1 distance) run-length coded with 16 / 17 / 18, their code built
//               by the same function, HCLEN by the format's order
//   payload     steps of four bytes per lane (at most 60 bits); an exclusive wave scan of the lanes' bit counts places
//               each lane's bits; they are ORed into a zeroed ring of 256 words in LDS, whose complete words leave for
//               the member's slot as aligned 32-bit stores, 64 words or more at a time
//   trailer     CRC-32 (bz_crc_term of nte_bgzf_inflate.h, the lanes' terms XORed) and ISIZE through the same writer
// The slot is DZ_SLOT bytes at a 4-byte aligned address; the last, partial word is stored whole (the bytes behind the
// member inside its slot are of no meaning).
#pragma once

#include "nte_bgzf_inflate.h"

#include <stdint.h>
#include <string.h>

namespace nte_bgzf {

constexpr uint32_t DZ_BLOCK = 65280; // plain bytes of a member (bgzip's own block size)
constexpr uint32_t DZ_SLOT = 65536;  // bytes a member may take
constexpr uint32_t DZ_HEAD = 18;     // the gzip header with its one extra subfield
constexpr uint32_t DZ_TAIL = 8;      // CRC-32, ISIZE
constexpr uint32_t DZ_STORED = 5;    // a stored block's own bytes: BFINAL / BTYPE, LEN, NLEN
constexpr int DZ_NSYM = 257;         // byte values and end-of-block
constexpr int DZ_NLEN = 258;         // lengths the header holds: DZ_NSYM + one distance code
constexpr int DZ_BALLOTS = 6;        // distinct values a histogram step settles by ballot
constexpr uint32_t DZ_RING = 256;    // words of the bit writer's ring

// One wave's tables (8.1 KiB; 4 waves a workgroup).
struct DzTables
{
	uint32_t hist[DZ_NSYM + 3]; // symbol counts; the code-length code's counts in its first 19 words afterwards
	uint32_t lc[DZ_NSYM + 3];   // per symbol: code (bit-reversed: first bit lowest) | length << 16
	uint32_t sw[DZ_NSYM + 3];   // the used symbols' counts by rank ...
	uint32_t iw[DZ_NSYM + 3];   // ... and the inner nodes' weights in the order they are made
	uint16_t ssym[DZ_NSYM + 3]; // the used symbols by rank
	uint16_t lpar[DZ_NSYM + 3]; // a ranked leaf's parent (index of an inner node)
	uint16_t ipar[DZ_NSYM + 3]; // an inner node's parent
	uint16_t idep[DZ_NSYM + 3]; // an inner node's depth
	uint8_t lens[DZ_NLEN + 2];  // the literal/length lengths and the one distance length (0)
	uint8_t rsym[DZ_NLEN + 2];  // the lengths as code-length symbols 0 .. 18
	uint8_t rext[DZ_NLEN + 2];  // ... and the value of a symbol's extra bits
	uint8_t clen[20];           // the code-length code's lengths
	uint32_t clc[20];           // ... and its codes, as lc
	uint32_t cnt[16], next[17]; // codes of each length; the next canonical code of each length
	uint32_t n_used, n_rle, hclen, head_bits, pay_bits;
	uint32_t ring[DZ_RING];
};

// the bit writer: wave-uniform position, the ring in LDS, complete words to the slot
struct DzBits
{
	uint32_t* slot;   // the member's slot as words
	uint32_t* ring;
	uint32_t bitpos;  // bits written
	uint32_t flushed; // words stored to the slot
};

#if defined(__HIP_DEVICE_COMPILE__)
#define DZ_OR32(p, v) atomicOr((p), (v))
#else
#define DZ_OR32(p, v) (*(p) |= (v))
#endif

// the timing build (make bgzf_phases) stamps the stages of dz_member; nothing of it is in the shipped library
#ifndef DZ_PHASE
#define DZ_PHASE_BEGIN() ((void)0)
#define DZ_PHASE(i) ((void)0)
#endif

// the XOR of v over the wave's lanes, in every lane
BZ_HD uint32_t
dz_wave_xor(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	for (int d = 1; d < 64; d <<= 1) {
		v ^= __shfl_xor(v, d, 64);
	}
#endif
	return v;
}

// the sum of v over the lanes below this one; *total: over all lanes, in every lane
BZ_HD uint32_t
dz_wave_scan(uint32_t v, uint32_t lane, uint32_t* total)
{
#if defined(__HIP_DEVICE_COMPILE__)
	uint32_t incl = v;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t up = __shfl_up(incl, d, 64);
		if (lane >= (uint32_t)d) {
			incl += up;
		}
	}
	*total = __shfl(incl, 63, 64);
	return incl - v;
#else
	(void)lane;
	*total = v;
	return 0;
#endif
}

// this lane's four bytes of a step: src[at .. at + 4) clipped to n; *nb: how many are there
BZ_HD uint32_t
dz_load4(const uint8_t* src, uint32_t n, uint32_t at, uint32_t* nb)
{
	uint32_t w = 0;
	if (at + 4 <= n) {
		memcpy(&w, src + at, 4);
		*nb = 4;
		return w;
	}
	uint32_t have = 0;
	for (; at + have < n && have < 4; have++) {
		w |= (uint32_t)src[at + have] << (8 * have);
	}
	*nb = have;
	return w;
}

BZ_HD void
dz_histogram(const uint8_t* src, uint32_t n, uint32_t* hist, uint32_t lane, uint32_t lanes)
{
	for (uint32_t s = lane; s < (uint32_t)DZ_NSYM; s += lanes) {
		hist[s] = s == 256 ? 1u : 0u; // one end-of-block
	}
	BZ_SYNC();
	for (uint32_t base = 0; base < n; base += 4 * lanes) {
		uint32_t nb;
		const uint32_t w = dz_load4(src, n, base + 4 * lane, &nb);
		for (uint32_t j = 0; j < 4; j++) {
			const uint32_t b = (w >> (8 * j)) & 255;
			const bool valid = j < nb;
#if defined(__HIP_DEVICE_COMPILE__)
			bool mine = valid;
			unsigned long long pending = __ballot(mine);
			for (int it = 0; it < DZ_BALLOTS && pending; it++) {
				const int leader = __ffsll((long long)pending) - 1;
				const uint32_t v = __shfl(b, leader, 64);
				const unsigned long long same = __ballot(mine && b == v);
				if (lane == (uint32_t)leader) {
					atomicAdd(&hist[v], (uint32_t)__popcll(same));
				}
				mine = mine && b != v;
				pending &= ~same;
			}
			if (mine) {
				atomicAdd(&hist[b], 1u);
			}
#else
			if (valid) {
				hist[b]++;
			}
#endif
		}
	}
	BZ_SYNC();
}

BZ_HD uint32_t
dz_bitrev(uint32_t code, uint32_t len)
{
	uint32_t r = 0;
	for (uint32_t i = 0; i < len; i++) {
		r = r << 1 | ((code >> i) & 1);
	}
	return r;
}

// freq[0 .. nsym) to a complete prefix code of lengths <= maxlen in lens[0 .. nsym) (0: unused) and its canonical
// codes, bit-reversed, in code_of(s) = code | length << 16 written to lc[s].  At least one freq is not 0.
BZ_HD void
dz_build_code(const uint32_t* freq, int nsym, int maxlen, uint8_t* lens, uint32_t* lc, DzTables* t, uint32_t lane, uint32_t lanes)
{
	// ranks: symbol s stands behind every used symbol of a smaller count, and of the same count and a smaller value
	for (int s = (int)lane; s < nsym; s += (int)lanes) {
		lens[s] = 0;
		lc[s] = 0;
		const uint32_t f = freq[s];
		if (f) {
			uint32_t rank = 0;
			for (int o = 0; o < nsym; o++) {
				const uint32_t g = freq[o];
				rank += (g != 0 && (g < f || (g == f && o < s))) ? 1u : 0u;
			}
			t->ssym[rank] = (uint16_t)s;
			t->sw[rank] = f;
		}
	}
	BZ_SYNC();
	if (lane == 0) {
		int n = 0;
		for (int s = 0; s < nsym; s++) {
			n += freq[s] != 0;
		}
		uint32_t* cnt = t->cnt;
		for (int l = 0; l < 16; l++) {
			cnt[l] = 0;
		}
		if (n == 1) { // a second code beside the only one: the set is complete
			t->ssym[1] = t->ssym[0];
			t->ssym[0] = (uint16_t)(t->ssym[1] == 0 ? 1 : 0);
			n = 2;
			cnt[1] = 2;
		} else {
			// the tree: inner node k joins the two lightest of the leaves and inner nodes not yet joined; a leaf goes first
			// where the weights are equal
			int li = 0, ii = 0;
			for (int k = 0; k < n - 1; k++) {
				uint32_t w = 0;
				for (int pick = 0; pick < 2; pick++) {
					if (li < n && (ii >= k || t->sw[li] <= t->iw[ii])) {
						w += t->sw[li];
						t->lpar[li++] = (uint16_t)k;
					} else {
						w += t->iw[ii];
						t->ipar[ii++] = (uint16_t)k;
					}
				}
				t->iw[k] = w;
			}
			t->idep[n - 2] = 0;
			for (int k = n - 3; k >= 0; k--) {
				t->idep[k] = (uint16_t)(t->idep[t->ipar[k]] + 1);
			}
			for (int i = 0; i < n; i++) {
				const int d = t->idep[t->lpar[i]] + 1;
				cnt[d < maxlen ? d : maxlen]++;
			}
			// the Kraft sum in units of 2^-maxlen; over-long codes folded to maxlen made it too large by less than one
			// unit each: at most n passes
			uint32_t total = 0;
			for (int l = 1; l <= maxlen; l++) {
				total += cnt[l] << (maxlen - l);
			}
			for (int pass = 0; pass < nsym && total > (1u << maxlen); pass++) {
				cnt[maxlen]--;
				for (int l = maxlen - 1; l >= 1; l--) {
					if (cnt[l]) {
						cnt[l]--;
						cnt[l + 1] += 2;
						break;
					}
				}
				total--;
			}
		}
		// lengths by rank: the heaviest symbols take the shortest codes
		int j = n;
		for (int l = 1; l <= maxlen; l++) {
			for (uint32_t q = 0; q < cnt[l]; q++) {
				lens[t->ssym[--j]] = (uint8_t)l;
			}
		}
		// canonical codes (RFC 1951, 3.2.2)
		uint32_t* next = t->next;
		next[0] = next[1] = 0;
		for (int l = 1; l <= maxlen; l++) {
			next[l + 1] = (next[l] + cnt[l]) << 1;
		}
		for (int s = 0; s < nsym; s++) {
			const uint32_t l = lens[s];
			if (l) {
				lc[s] = dz_bitrev(next[l]++, l) | l << 16;
			}
		}
		t->n_used = (uint32_t)n;
	}
	BZ_SYNC();
}

// t->lens[0 .. DZ_NLEN) to code-length symbols with their counts in t->hist[0 .. 19), the code over them, HCLEN and
// the header's bits (BFINAL and BTYPE included)
BZ_HD void
dz_build_header(DzTables* t, uint32_t lane, uint32_t lanes)
{
	if (lane == 0) {
		for (int s = 0; s < 19; s++) {
			t->hist[s] = 0;
		}
		uint32_t m = 0, extra = 0;
		for (int i = 0; i < DZ_NLEN;) {
			const uint8_t v = t->lens[i];
			int run = 1;
			while (i + run < DZ_NLEN && t->lens[i + run] == v) {
				run++;
			}
			i += run;
			if (v == 0) {
				while (run >= 11) {
					const int r = run < 138 ? run : 138;
					t->rsym[m] = 18;
					t->rext[m++] = (uint8_t)(r - 11);
					extra += 7;
					run -= r;
				}
				if (run >= 3) {
					t->rsym[m] = 17;
					t->rext[m++] = (uint8_t)(run - 3);
					extra += 3;
					run = 0;
				}
			} else {
				t->rsym[m] = v;
				t->rext[m++] = 0;
				run--;
				while (run >= 3) {
					const int r = run < 6 ? run : 6;
					t->rsym[m] = 16;
					t->rext[m++] = (uint8_t)(r - 3);
					extra += 2;
					run -= r;
				}
			}
			for (; run > 0; run--) {
				t->rsym[m] = v;
				t->rext[m++] = 0;
			}
		}
		for (uint32_t i = 0; i < m; i++) {
			t->hist[t->rsym[i]]++;
		}
		t->n_rle = m;
		t->head_bits = 3 + 14 + extra;
	}
	BZ_SYNC();
	dz_build_code(t->hist, 19, 7, t->clen, t->clc, t, lane, lanes);
	if (lane == 0) {
		uint32_t bits = 0;
		for (int s = 0; s < 19; s++) {
			bits += t->hist[s] * t->clen[s];
		}
		uint32_t hclen = 4;
		for (int i = 0; i < 19; i++) {
			const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
			if (t->clen[at] && (uint32_t)i + 1 > hclen) {
				hclen = (uint32_t)i + 1;
			}
		}
		t->hclen = hclen;
		t->head_bits += 3 * hclen + bits;
	}
	BZ_SYNC();
}

// complete words of the ring to the slot, once there are min_words of them
BZ_HD void
dz_flush(DzBits& b, uint32_t min_words, uint32_t lane, uint32_t lanes)
{
	const uint32_t upto = b.bitpos >> 5;
	if (upto - b.flushed < min_words || upto == b.flushed) {
		return;
	}
	BZ_SYNC(); // the ring's bits were set by all lanes
	for (uint32_t w = b.flushed + lane; w < upto; w += lanes) {
		b.slot[w] = b.ring[w & (DZ_RING - 1)];
		b.ring[w & (DZ_RING - 1)] = 0;
	}
	BZ_SYNC();
	b.flushed = upto;
}

// n <= 32 bits at the writer's position, by one lane; every lane moves the position
BZ_HD void
dz_put(DzBits& b, uint32_t v, uint32_t n, uint32_t lane)
{
	if (lane == 0 && n) {
		const uint32_t w = b.bitpos >> 5, sh = b.bitpos & 31;
		const uint64_t x = (uint64_t)(n < 32 ? v & ((1u << n) - 1) : v) << sh;
		b.ring[w & (DZ_RING - 1)] |= (uint32_t)x;
		if (x >> 32) {
			b.ring[(w + 1) & (DZ_RING - 1)] |= (uint32_t)(x >> 32);
		}
	}
	b.bitpos += n;
}

BZ_HD uint8_t
dz_head_byte(uint32_t i, uint32_t member)
{
	// ID1 ID2 CM FLG=FEXTRA | MTIME 0 | XFL 0 | OS 255 | XLEN 6 | 'B' 'C' 2 0 | BSIZE = member - 1
	const uint32_t bsize = member - 1;
	return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xff : i == 10 ? 6 : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2
	     : i == 16 ? (uint8_t)(bsize & 255) : i == 17 ? (uint8_t)(bsize >> 8) : 0;
}

// The block src[0 .. n), 1 <= n <= DZ_BLOCK, into one member at slot (4-byte aligned, DZ_SLOT bytes, whatever they
// hold).  Returns the member's bytes; *stored: 1 when it holds a stored block.
//
// Bounds: the histogram indexes hist by a byte value or 256; dz_build_code indexes its tables by rank < used symbols
// <= nsym <= 257 and by inner node < used - 1; the run-length code of 258 lengths is at most 258 symbols; the ring is
// indexed modulo its size, and between two flushes at most 63 words + one step's 64 x 60 bits (120 words) + one partial
// word wait in it; the slot is written at words below ceil(member / 4) <= 16,328, the stored form at bytes below
// 31 + n <= 65,311.  Every loop is counted by n, by the symbols or by the lengths.
BZ_HD uint32_t
dz_member(const uint8_t* src, uint32_t n, uint8_t* slot, DzTables* t, uint32_t lane, uint32_t lanes, uint32_t* stored)
{
	DZ_PHASE_BEGIN();
	dz_histogram(src, n, t->hist, lane, lanes);
	DZ_PHASE(0);
	dz_build_code(t->hist, DZ_NSYM, 15, t->lens, t->lc, t, lane, lanes);
	if (lane == 0) {
		uint32_t bits = 0;
		for (int s = 0; s < DZ_NSYM; s++) {
			bits += t->hist[s] * (t->lc[s] >> 16);
		}
		t->pay_bits = bits;
		t->lens[DZ_NSYM] = 0; // HDIST: one code, of length 0
	}
	BZ_SYNC();
	dz_build_header(t, lane, lanes);
	const uint32_t dyn_bytes = (t->head_bits + t->pay_bits + 7) >> 3;
	DZ_PHASE(1);
	uint32_t crc = dz_wave_xor(bz_crc_term(src, n, lane, lanes));
	crc = ~crc;
	DZ_PHASE(2);
	if (dyn_bytes >= DZ_STORED + n) {
		const uint32_t member = DZ_HEAD + DZ_STORED + n + DZ_TAIL;
		for (uint32_t i = lane; i < DZ_HEAD; i += lanes) {
			slot[i] = dz_head_byte(i, member);
		}
		if (lane == 0) {
			uint8_t* p = slot + DZ_HEAD;
			p[0] = 1; // BFINAL, BTYPE 00
			p[1] = (uint8_t)(n & 255);
			p[2] = (uint8_t)(n >> 8);
			p[3] = (uint8_t)(~n & 255);
			p[4] = (uint8_t)((~n >> 8) & 255);
			p += DZ_STORED + n;
			for (int i = 0; i < 4; i++) {
				p[i] = (uint8_t)(crc >> (8 * i));
				p[4 + i] = (uint8_t)(n >> (8 * i));
			}
		}
		for (uint32_t i = lane; i < n; i += lanes) {
			slot[DZ_HEAD + DZ_STORED + i] = src[i];
		}
		*stored = 1;
		return member;
	}
	const uint32_t member = DZ_HEAD + dyn_bytes + DZ_TAIL;
	for (uint32_t w = lane; w < DZ_RING; w += lanes) {
		t->ring[w] = 0;
	}
	BZ_SYNC();
	DzBits b = { (uint32_t*)slot, t->ring, 0, 0 };
	for (uint32_t i = 0; i < DZ_HEAD; i++) {
		dz_put(b, dz_head_byte(i, member), 8, lane);
	}
	dz_put(b, 1 | 2 << 1, 3, lane);                                  // BFINAL, BTYPE 10
	dz_put(b, 0 | 0 << 5 | (t->hclen - 4) << 10, 14, lane);          // HLIT 257, HDIST 1, HCLEN
	for (uint32_t i = 0; i < t->hclen; i++) {
		const int at = i < 3 ? 16 + (int)i : i == 3 ? 0 : (i & 1) ? 8 - (((int)i - 3) >> 1) : 8 + (((int)i - 4) >> 1);
		dz_put(b, t->clen[at], 3, lane);
	}
	dz_flush(b, 1, lane, lanes);
	for (uint32_t i = 0; i < t->n_rle; i++) {
		const uint32_t s = t->rsym[i];
		dz_put(b, t->clc[s] & 0xFFFF, t->clen[s], lane);
		dz_put(b, t->rext[i], s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u, lane);
		if ((i & 63) == 63) {
			dz_flush(b, 1, lane, lanes); // (64 symbols are at most 64 x 14 bits: 28 words)
		}
	}
	dz_flush(b, 1, lane, lanes);
	BZ_SYNC(); // (one lane wrote the header's last, partial word: all lanes OR into it next)
	DZ_PHASE(3);
	// the payload
	for (uint32_t base = 0; base < n; base += 4 * lanes) {
		uint32_t nb;
		const uint32_t w = dz_load4(src, n, base + 4 * lane, &nb);
		uint64_t acc = 0;
		uint32_t bits = 0;
		for (uint32_t j = 0; j < nb; j++) {
			const uint32_t e = t->lc[(w >> (8 * j)) & 255];
			acc |= (uint64_t)(e & 0xFFFF) << bits;
			bits += e >> 16;
		}
		uint32_t total;
		const uint32_t pos = b.bitpos + dz_wave_scan(bits, lane, &total);
		if (bits) {
			const uint32_t at = pos >> 5, sh = pos & 31;
			const uint64_t lo = acc << sh;
			const uint32_t w2 = sh ? (uint32_t)(acc >> (64 - sh)) : 0u;
			if ((uint32_t)lo) {
				DZ_OR32(&b.ring[at & (DZ_RING - 1)], (uint32_t)lo);
			}
			if ((uint32_t)(lo >> 32)) {
				DZ_OR32(&b.ring[(at + 1) & (DZ_RING - 1)], (uint32_t)(lo >> 32));
			}
			if (w2) {
				DZ_OR32(&b.ring[(at + 2) & (DZ_RING - 1)], w2);
			}
		}
		b.bitpos += total;
		dz_flush(b, 64, lane, lanes);
	}
	BZ_SYNC();
	DZ_PHASE(4);
	dz_put(b, t->lc[256] & 0xFFFF, t->lc[256] >> 16, lane); // end-of-block
	dz_put(b, 0, (8 - (b.bitpos & 7)) & 7, lane);           // to the byte boundary
	dz_put(b, crc, 32, lane);
	dz_put(b, n, 32, lane);
	dz_put(b, 0, (32 - (b.bitpos & 31)) & 31, lane); // the last word whole
	dz_flush(b, 1, lane, lanes);
	DZ_PHASE(5);
	*stored = 0;
	return member;
}

// the 28 bytes that end a BGZF file: a member of no bytes (a fixed-code block of the end-of-block code alone)
constexpr uint8_t DZ_EOF[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };

} // namespace nte_bgzf
