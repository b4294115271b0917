// nte_bgzf_inflate.h -- one BGZF member on the device, written once: the raw DEFLATE stream (RFC 1951) of the member
// into its ISIZE bytes, and the CRC-32 of those bytes.  The inflate kernel (nte_reads_inflate.hip) and the serial host
// model (ntedit_hip_reads_inflate_model, same unit) are both built from these functions, as nte_reads_grammar.h serves
// the parse kernels.
//
// Every function takes (lane, lanes).  The kernel calls them from all 64 lanes of a wavefront with (lane, 64); the
// model calls them with (0, 1).  Whatever steers the decode -- the bit buffer, the tables, the output position -- is
// computed from the member's bytes alone, so it is the same in every lane (wave-uniform): the decode of a symbol is
// one lane's work done in lockstep, table reads are one LDS address per wave (a broadcast, no bank conflict), and no
// value has to travel between lanes.  Only the loops that touch many bytes are split by lane: table fills, stored-block
// and match copies (byte i of a match from src[i mod dist]), and the CRC (each lane a contiguous piece, combined by
// multiplication with x^(8 len) mod P).  BZ_SYNC() stands where one lane reads what another has stored.
//
// Verdicts follow zlib's inflate: over-subscribed code sets are refused, incomplete ones too unless the set (literal /
// length or distance) holds a single code of length 1, a set without any code is legal until it is used, a block
// without an end-of-block code is refused, as are literal/length symbols 286-287 and distance symbols 30-31.
#pragma once

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define BZ_HD __host__ __device__ __forceinline__
#else
#define BZ_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define BZ_SYNC() __threadfence_block() // workgroup scope: LDS and global stores of this wave's lanes, before its later loads
#else
#define BZ_SYNC() ((void)0) // (one lane: program order)
#endif

namespace nte_bgzf {

// a member's status (NTEDIT_INFLATE_* in ntedit_hip.h)
enum : uint32_t {
	BZ_OK = 0,
	BZ_BAD_BLOCK = 1,   // block type 3
	BZ_BAD_CODES = 2,   // a code set that is over-subscribed, incomplete, too large, or without end-of-block
	BZ_BAD_DIST = 3,    // a distance that reaches before the member's first byte
	BZ_OUT_OVER = 4,    // more output than ISIZE
	BZ_IN_OVER = 5,     // the stream needs bits past the member's compressed bytes
	BZ_SHORT_OUT = 6,   // the final block ends short of ISIZE
	BZ_LEFT_IN = 7,     // compressed bytes left behind the final block
	BZ_BAD_CRC = 8,     // the CRC-32 of the inflated bytes is not the trailer's
	BZ_BAD_STORED = 9,  // a stored block whose LEN is not the complement of NLEN
	BZ_BAD_SYMBOL = 10, // bits that are no code of the set, or a symbol zlib refuses (286, 287; distance 30, 31)
};

constexpr int BZ_LFAST = 10; // bits the literal/length look-up resolves at once
constexpr int BZ_DFAST = 8;  // ... the distance look-up

// One wave's tables (3.6 KiB; 4 waves a workgroup).  A fast entry is (symbol << 4 | code length), 0 for bits whose
// code is longer than the look-up: those go through the canonical walk over cnt / sym.
struct BzTables
{
	uint16_t lfast[1 << BZ_LFAST];
	uint16_t dfast[1 << BZ_DFAST];
	uint16_t lsym[288], dsym[32], csym[20];
	uint16_t lcnt[16], dcnt[16], ccnt[16]; // codes of each length
	uint16_t offs[16];
	uint8_t lens[288 + 32];
	uint32_t err;
};

struct BzBits
{
	const uint8_t* in;
	uint32_t n_in, pos; // pos: bytes taken into buf
	uint64_t buf;
	uint32_t bits; // valid bits of buf (the rest are 0)
};

// buf up to more than 56 bits, or to the end of the input: never a byte at or past in + n_in
BZ_HD void
bz_refill(BzBits& b)
{
	if (b.bits > 56) {
		return;
	}
	if (b.n_in - b.pos >= 8) {
		uint64_t w = 0;
		for (int i = 0; i < 8; i++) {
			w |= (uint64_t)b.in[b.pos + i] << (8 * i);
		}
		const uint32_t n = (64 - b.bits) >> 3; // 1 .. 8
		if (n < 8) {
			w &= (1ull << (8 * n)) - 1;
		}
		b.buf |= w << b.bits;
		b.pos += n;
		b.bits += 8 * n;
		return;
	}
	while (b.bits <= 56 && b.pos < b.n_in) {
		b.buf |= (uint64_t)b.in[b.pos++] << b.bits;
		b.bits += 8;
	}
}

BZ_HD void
bz_drop(BzBits& b, uint32_t n) // n <= b.bits, n < 64
{
	b.buf >>= n;
	b.bits -= n;
}

// The canonical walk: the code in the low bits of v (first bit of the code lowest), over a set with cnt[l] codes of
// length l <= maxlen and its symbols sorted by (length, symbol).  *len = the code's length, or 0 when the bits are no
// code of the set.
BZ_HD uint32_t
bz_walk(uint64_t v, const uint16_t* cnt, const uint16_t* sym, int maxlen, uint32_t* len)
{
	int32_t code = 0, first = 0, index = 0;
	for (int l = 1; l <= maxlen; l++) {
		code |= (int32_t)(v & 1);
		v >>= 1;
		const int32_t count = cnt[l];
		if (code - count < first) {
			*len = (uint32_t)l;
			return sym[index + (code - first)];
		}
		index += count;
		first += count;
		first <<= 1;
		code <<= 1;
	}
	*len = 0;
	return 0;
}

// one symbol; *err set (and 0 returned) when the bits are no code or lie past the input
BZ_HD uint32_t
bz_symbol(BzBits& b, const uint16_t* fast, int fast_bits, const uint16_t* cnt, const uint16_t* sym, uint32_t* err)
{
	uint32_t len, s;
	const uint32_t e = fast[b.buf & ((1u << fast_bits) - 1)];
	if (e) {
		len = e & 15;
		s = e >> 4;
	} else {
		s = bz_walk(b.buf, cnt, sym, 15, &len);
		if (len == 0) {
			*err = b.bits < 15 ? (uint32_t)BZ_IN_OVER : (uint32_t)BZ_BAD_SYMBOL;
			return 0;
		}
	}
	if (len > b.bits) {
		*err = BZ_IN_OVER;
		return 0;
	}
	bz_drop(b, len);
	return s;
}

// lens[0 .. n) to cnt / sym (one lane's work); codes: the code-length alphabet, which may not be incomplete at all
BZ_HD uint32_t
bz_count_sort(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* offs, uint16_t* sym, bool codes)
{
	for (int l = 0; l < 16; l++) {
		cnt[l] = 0;
	}
	for (int s = 0; s < n; s++) {
		cnt[lens[s] & 15]++;
	}
	cnt[0] = 0;
	int32_t left = 1, max = 0;
	for (int l = 1; l < 16; l++) {
		left <<= 1;
		left -= (int32_t)cnt[l];
		if (left < 0) {
			return BZ_BAD_CODES; // over-subscribed
		}
		if (cnt[l]) {
			max = l;
		}
	}
	if (left > 0 && (codes || max > 1)) {
		return BZ_BAD_CODES; // incomplete (a code-length alphabet without a code ends in a refusal in zlib as well)
	}
	offs[1] = 0;
	for (int l = 1; l < 15; l++) {
		offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
	}
	for (int s = 0; s < n; s++) {
		const int l = lens[s] & 15;
		if (l) {
			sym[offs[l]++] = (uint16_t)s;
		}
	}
	return BZ_OK;
}

// the look-up of a set: entry e from the walk over e's own bits (each lane its share of the entries)
BZ_HD void
bz_fill_fast(uint16_t* fast, int fast_bits, const uint16_t* cnt, const uint16_t* sym, uint32_t lane, uint32_t lanes)
{
	for (uint32_t e = lane; e < (1u << fast_bits); e += lanes) {
		uint32_t len;
		const uint32_t s = bz_walk(e, cnt, sym, fast_bits, &len);
		fast[e] = len ? (uint16_t)(s << 4 | len) : (uint16_t)0;
	}
}

// t->lens[0 .. nlen) and t->lens[nlen .. nlen + ndist) to the two sets' tables
BZ_HD uint32_t
bz_build_sets(BzTables* t, int nlen, int ndist, uint32_t lane, uint32_t lanes)
{
	BZ_SYNC();
	if (lane == 0) {
		uint32_t err = t->lens[256] == 0 ? (uint32_t)BZ_BAD_CODES : (uint32_t)BZ_OK; // no end-of-block code
		if (!err) {
			err = bz_count_sort(t->lens, nlen, t->lcnt, t->offs, t->lsym, false);
		}
		if (!err) {
			err = bz_count_sort(t->lens + nlen, ndist, t->dcnt, t->offs, t->dsym, false);
		}
		t->err = err;
	}
	BZ_SYNC();
	if (t->err) {
		return t->err;
	}
	bz_fill_fast(t->lfast, BZ_LFAST, t->lcnt, t->lsym, lane, lanes);
	bz_fill_fast(t->dfast, BZ_DFAST, t->dcnt, t->dsym, lane, lanes);
	BZ_SYNC();
	return BZ_OK;
}

BZ_HD uint32_t
bz_build_fixed(BzTables* t, uint32_t lane, uint32_t lanes)
{
	BZ_SYNC(); // (no lane still reads the tables of the block before)
	for (uint32_t s = lane; s < 288 + 32; s += lanes) {
		t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
	}
	return bz_build_sets(t, 288, 32, lane, lanes);
}

// the header of a dynamic block: HLIT, HDIST, HCLEN, the code-length alphabet, the two sets' lengths
BZ_HD uint32_t
bz_build_dynamic(BzBits& b, BzTables* t, uint32_t lane, uint32_t lanes)
{
	bz_refill(b);
	if (b.bits < 14) {
		return BZ_IN_OVER;
	}
	const int nlen = (int)(b.buf & 31) + 257, ndist = (int)((b.buf >> 5) & 31) + 1, ncode = (int)((b.buf >> 10) & 15) + 4;
	bz_drop(b, 14);
	if (nlen > 286 || ndist > 30) {
		return BZ_BAD_CODES;
	}
	BZ_SYNC(); // (no lane still reads the tables of the block before)
	// the 19 code lengths' lengths, in the format's order; every lane reads the bits, lane 0 stores
	uint32_t err = BZ_OK;
	for (int i = 0; i < 19; i++) {
		// 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
		const int at = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - ((i - 3) >> 1) : 8 + ((i - 4) >> 1);
		uint32_t v = 0;
		if (i < ncode) {
			bz_refill(b);
			if (b.bits < 3) {
				err = BZ_IN_OVER;
				break;
			}
			v = (uint32_t)(b.buf & 7);
			bz_drop(b, 3);
		}
		if (lane == 0) {
			t->lens[at] = (uint8_t)v;
		}
	}
	if (err) {
		return err;
	}
	BZ_SYNC();
	if (lane == 0) {
		t->err = bz_count_sort(t->lens, 19, t->ccnt, t->offs, t->csym, true);
	}
	BZ_SYNC();
	if (t->err) {
		return t->err;
	}
	// (the walk reads ccnt / csym only; lens is free for the two sets from here)
	BZ_SYNC();
	int have = 0;
	uint32_t prev = 0;
	while (have < nlen + ndist) {
		bz_refill(b);
		uint32_t len;
		const uint32_t s = bz_walk(b.buf, t->ccnt, t->csym, 7, &len);
		if (len == 0) {
			return b.bits < 7 ? (uint32_t)BZ_IN_OVER : (uint32_t)BZ_BAD_SYMBOL;
		}
		const uint32_t extra = s < 16 ? 0u : s == 16 ? 2u : s == 17 ? 3u : 7u;
		if (len + extra > b.bits) {
			return BZ_IN_OVER;
		}
		bz_drop(b, len);
		uint32_t rep = 1, val = s;
		if (s >= 16) {
			if (s == 16 && have == 0) {
				return BZ_BAD_CODES; // a repeat with nothing to repeat
			}
			rep = (s == 16 ? 3u : s == 17 ? 3u : 11u) + (uint32_t)(b.buf & ((1u << extra) - 1));
			val = s == 16 ? prev : 0u;
			bz_drop(b, extra);
		}
		if ((uint32_t)have + rep > (uint32_t)(nlen + ndist)) {
			return BZ_BAD_CODES; // a repeat past the last length
		}
		if (lane == 0) {
			for (uint32_t r = 0; r < rep; r++) {
				t->lens[have + r] = (uint8_t)val;
			}
		}
		have += (int)rep;
		prev = val;
	}
	return bz_build_sets(t, nlen, ndist, lane, lanes);
}

// The member's DEFLATE stream in[0 .. n_in) into out[0 .. n_out); n_out is the trailer's ISIZE.
//
// Why this ends and stays in bounds on any bytes whatever:
//   * Bits come from bz_refill alone, which reads in[pos] only for pos < n_in, and are spent by bz_drop alone, whose
//     every call is preceded by a check that the buffer holds that many; so over the whole call at most 8 n_in bits
//     are dropped.  Every pass of the block loop drops the 3 header bits, every pass of the symbol loop the 1 to 15
//     bits of a literal/length code, every pass of the code-length loop 1 to 7, or returns; the 19-step loop is
//     counted.  So the loops make at most 8 n_in + 1 passes between them (`budget` states the same bound once more,
//     for a reader who would rather not follow the argument).
//   * A stored block copies len bytes only after len <= n_in - pos and len <= n_out - done have been checked.
//   * A literal is stored only at done < n_out; a match only after dist <= done (no read before out) and
//     len <= n_out - done (no write past out + n_out), its sources all below out + done.
//   * Table indices: a look-up index is masked to the table's size; the walk indexes cnt[1 .. 15] and
//     sym[index + code - first] with that sum below the number of codes counted, at most the set's size; lens is
//     written at have + r < nlen + ndist <= 316 and at the 19 code-length places.
//   * After the final block the whole bytes still in the buffer go back to the input; a byte left over refuses the
//     member (BZ_LEFT_IN), as does an output short of n_out (BZ_SHORT_OUT).
BZ_HD uint32_t
bz_inflate(const uint8_t* in, uint32_t n_in, uint8_t* out, uint32_t n_out, BzTables* t, uint32_t lane, uint32_t lanes)
{
	BzBits b = { in, n_in, 0, 0, 0 };
	uint32_t done = 0;
	uint64_t budget = 8ull * n_in + 1;
	bool fixed_built = false;
	for (;;) {
		bz_refill(b);
		if (b.bits < 3) {
			return BZ_IN_OVER;
		}
		const uint32_t last = (uint32_t)(b.buf & 1), type = (uint32_t)((b.buf >> 1) & 3);
		bz_drop(b, 3);
		if (budget-- == 0) {
			return BZ_IN_OVER;
		}
		if (type == 3) {
			return BZ_BAD_BLOCK;
		}
		if (type == 0) {
			bz_drop(b, b.bits & 7); // to the byte boundary: the buffer holds whole bytes
			bz_refill(b);
			if (b.bits < 32) {
				return BZ_IN_OVER;
			}
			const uint32_t len = (uint32_t)(b.buf & 0xFFFF), nlen = (uint32_t)((b.buf >> 16) & 0xFFFF);
			if (len != (nlen ^ 0xFFFF)) {
				return BZ_BAD_STORED;
			}
			bz_drop(b, 32);
			b.pos -= b.bits >> 3; // the buffered bytes go back: the block's bytes are copied from the input
			b.buf = 0;
			b.bits = 0;
			if (len > n_in - b.pos) {
				return BZ_IN_OVER;
			}
			if (len > n_out - done) {
				return BZ_OUT_OVER;
			}
			for (uint32_t i = lane; i < len; i += lanes) {
				out[done + i] = in[b.pos + i];
			}
			done += len;
			b.pos += len;
		} else {
			uint32_t err;
			if (type == 1) {
				err = fixed_built ? (uint32_t)BZ_OK : bz_build_fixed(t, lane, lanes);
				fixed_built = true;
			} else {
				err = bz_build_dynamic(b, t, lane, lanes);
				fixed_built = false;
			}
			if (err) {
				return err;
			}
			for (;;) {
				if (b.bits < 48) {
					bz_refill(b); // a literal/length code, its extra bits, a distance code and its: at most 48
				}
				if (budget-- == 0) {
					return BZ_IN_OVER;
				}
				err = BZ_OK;
				uint32_t s = bz_symbol(b, t->lfast, BZ_LFAST, t->lcnt, t->lsym, &err);
				if (err) {
					return err;
				}
				if (s < 256) {
					if (done >= n_out) {
						return BZ_OUT_OVER;
					}
					if (lane == 0) {
						out[done] = (uint8_t)s;
					}
					done++;
					continue;
				}
				if (s == 256) {
					break;
				}
				if (s >= 286) {
					return BZ_BAD_SYMBOL;
				}
				s -= 257;
				// lengths 3 .. 258: 0 extra bits up to 10, then four codes per extra bit; 258 has its own code
				uint32_t extra = s < 8 || s == 28 ? 0u : (s >> 2) - 1;
				uint32_t len = s < 8 ? 3 + s : s == 28 ? 258u : 3 + ((4 + (s & 3)) << extra);
				if (extra > b.bits) {
					return BZ_IN_OVER;
				}
				len += (uint32_t)(b.buf & ((1u << extra) - 1));
				bz_drop(b, extra);
				const uint32_t d = bz_symbol(b, t->dfast, BZ_DFAST, t->dcnt, t->dsym, &err);
				if (err) {
					return err;
				}
				if (d >= 30) {
					return BZ_BAD_SYMBOL;
				}
				// distances 1 .. 32768: 0 extra bits up to 4, then two codes per extra bit
				extra = d < 4 ? 0u : (d >> 1) - 1;
				uint32_t dist = d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << extra);
				if (extra > b.bits) {
					return BZ_IN_OVER;
				}
				dist += (uint32_t)(b.buf & ((1u << extra) - 1));
				bz_drop(b, extra);
				if (dist > done) {
					return BZ_BAD_DIST;
				}
				if (len > n_out - done) {
					return BZ_OUT_OVER;
				}
				BZ_SYNC(); // the bytes before `done` were stored by other lanes
				const uint8_t* src = out + done - dist;
				if (dist >= len) {
					for (uint32_t i = lane; i < len; i += lanes) {
						out[done + i] = src[i];
					}
				} else {
					for (uint32_t i = lane; i < len; i += lanes) {
						out[done + i] = src[i % dist];
					}
				}
				done += len;
			}
		}
		if (last) {
			break;
		}
	}
	b.pos -= b.bits >> 3;
	if (b.pos != n_in) {
		return BZ_LEFT_IN;
	}
	if (done != n_out) {
		return BZ_SHORT_OUT;
	}
	return BZ_OK;
}

// ------------------------------------------------------------------ CRC-32 (the gzip polynomial, reflected)
constexpr uint32_t BZ_POLY = 0xEDB88320u;

// the register after p[0 .. n) from a register of 0, without the final complement: linear in the bytes
BZ_HD uint32_t
bz_crc_raw(const uint8_t* p, uint32_t n)
{
	uint32_t c = 0;
	for (uint32_t i = 0; i < n; i++) {
		c ^= p[i];
		for (int k = 0; k < 8; k++) {
			c = (c >> 1) ^ (BZ_POLY & (0u - (c & 1)));
		}
	}
	return c;
}

// a * b mod P in GF(2), reflected (bit 31 is x^0): 32 shift / xor steps
BZ_HD uint32_t
bz_mulmod(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; i++) {
		p ^= b & (0u - ((a >> (31 - i)) & 1));
		b = (b >> 1) ^ (BZ_POLY & (0u - (b & 1)));
	}
	return p;
}

// x^(8 n) mod P: square and multiply
BZ_HD uint32_t
bz_xpow8(uint32_t n)
{
	uint32_t r = 0x80000000u, base = 0x00800000u; // x^0, x^8
	for (; n; n >>= 1) {
		if (n & 1) {
			r = bz_mulmod(r, base);
		}
		base = bz_mulmod(base, base);
	}
	return r;
}

// This lane's term of the CRC-32 of p[0 .. n): the XOR of the terms of all lanes, complemented, is the CRC.  Lane i
// takes the i-th contiguous piece; its raw register moves to its place by x^(8 (bytes behind the piece)); lane 0
// adds the initial register of all ones moved over the whole length.
BZ_HD uint32_t
bz_crc_term(const uint8_t* p, uint32_t n, uint32_t lane, uint32_t lanes)
{
	const uint32_t per = (n + lanes - 1) / lanes;
	const uint32_t a = lane * per < n ? lane * per : n, e = a + per < n ? a + per : n;
	uint32_t r = bz_mulmod(bz_crc_raw(p + a, e - a), bz_xpow8(n - e));
	if (lane == 0) {
		r ^= bz_mulmod(0xFFFFFFFFu, bz_xpow8(n));
	}
	return r;
}

} // namespace nte_bgzf
