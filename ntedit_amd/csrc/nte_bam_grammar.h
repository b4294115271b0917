// nte_bam_grammar.h -- the BAM grammar of --gpu_parse, written once (SAM specification 4.2, little-endian): what a clean
// header is, what a clean record is, which records are kept, and what their text is.  The kernels (nte_reads_bam.hip)
// and the serial host model (bam_model below: ntedit_hip_reads_bam_model) are both built from these functions, as
// nte_reads_grammar.h serves the text parser.  No length from the file is trusted: every read is checked against the
// bytes at hand before it is made.
//
// A chunk is a run of inflated bytes that starts at the file's first byte (at_header) or at a record start.
//   header   "BAM\1", l_text (i32), the text, n_ref (i32), n_ref x { l_name (i32), the name, l_ref (i32) }; clean when
//            the magic matches, l_text >= 0, n_ref >= 0 and every l_name >= 1.  A header that ends behind the bytes at
//            hand is not unclean: the chunk's cut is 0 and it grows.
//   record   block_size (i32), 32 fixed bytes (refID, pos, l_read_name u8, mapq, bin, n_cigar_op u16, flag u16, l_seq
//            u32, next_refID, next_pos, tlen), read_name, cigar (4 bytes each), seq ((l_seq + 1) / 2 bytes, the high
//            nibble first), qual (l_seq bytes), aux up to block_size (not interpreted).  Clean when block_size < 2^30,
//            l_read_name >= 1 and 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq <= block_size.
//   the cut  the offset of the first record that does not lie completely inside the chunk; a record is judged as soon
//            as its fields are inside (block_size alone: its range; the fixed bytes: the rest), so an unclean record
//            makes the chunk unclean even when its end is not.
//   kept     (flag & 0x900) == 0 (neither secondary nor supplementary) and l_seq >= min_len.  The strand flag 0x10 is not
//            applied: the sketch and the filter hash canonical k-mers (nte_reads.hip).
//            With a read filter (--min_read_len, --min_rq, --min_mean_qual: bam_reason) also by its rq:f aux field and
//            the mean of its qualities, which are the only reads this grammar makes of the aux fields.
//   text     every kept record's bases (codes "=ACMGRSVTWYHKDBN") followed by '\n', in file order.
#pragma once

#include <stdint.h>

#include "nte_bgzf_inflate.h"
#include "nte_reads_grammar.h"

#if defined(__HIP__) || defined(__HIPCC__)
#define BAM_HD __host__ __device__ __forceinline__
#else
#define BAM_HD inline
#endif

namespace nte_bam {

// the rules, as bits of `broken` (NTEDIT_BAM_BAD_* in ntedit_hip.h)
enum : uint32_t {
	BAM_BAD_MAGIC = 1,  // the first bytes are not "BAM\1"
	BAM_BAD_HEADER = 2, // l_text < 0, n_ref < 0 or an l_name < 1
	BAM_BAD_RECORD = 4, // l_read_name < 1, or the record's parts do not fit its block_size
	BAM_BAD_SIZE = 8,   // block_size < 0 or >= 2^30, or a chunk of 2^31 bytes or more
};
// what a hop or a header ends with, besides the bits above
enum : uint32_t {
	BAM_NEXT = 0,     // a whole clean record (header): go on behind it
	BAM_END = 1u << 8 // it ends behind the bytes at hand
};

constexpr uint64_t BAM_MAX_RAW = 1ull << 31;
constexpr uint32_t BAM_MAX_BLOCK = 1u << 30;
constexpr uint32_t BAM_MIN_RECORD = 4 + 32 + 1; // block_size, the fixed bytes, a read name of one byte
constexpr uint32_t BAM_NO_GUESS = ~0u;
constexpr int BAM_GUESS_HOPS = 3;               // records a guess's chain has to stay clean for behind its first

BAM_HD uint32_t
bam_ld16(const uint8_t* p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8;
}

BAM_HD uint32_t
bam_ld32(const uint8_t* p)
{
	return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the header of raw[0 .. n): BAM_NEXT and its length and n_ref, BAM_END, or the rule it breaks
BAM_HD uint32_t
bam_header(const uint8_t* raw, uint64_t n, uint64_t* header_len, uint32_t* n_ref)
{
	const uint8_t magic[4] = { 'B', 'A', 'M', 1 };
	for (uint64_t i = 0; i < 4 && i < n; i++) {
		if (raw[i] != magic[i]) {
			return BAM_BAD_MAGIC;
		}
	}
	if (n < 8) {
		return BAM_END;
	}
	const uint32_t l_text = bam_ld32(raw + 4);
	if (l_text >> 31) {
		return BAM_BAD_HEADER;
	}
	uint64_t p = 8 + (uint64_t)l_text;
	if (n < p + 4) {
		return BAM_END;
	}
	const uint32_t refs = bam_ld32(raw + p);
	if (refs >> 31) {
		return BAM_BAD_HEADER;
	}
	p += 4;
	for (uint32_t i = 0; i < refs; i++) {
		if (n < p + 4) {
			return BAM_END;
		}
		const uint32_t l_name = bam_ld32(raw + p);
		if (l_name >> 31 || l_name < 1) {
			return BAM_BAD_HEADER;
		}
		p += 4 + (uint64_t)l_name + 4; // the name and l_ref
		if (n < p) {
			return BAM_END;
		}
	}
	*header_len = p;
	*n_ref = refs;
	return BAM_NEXT;
}

struct BamRecord
{
	uint32_t next;    // the offset behind the record
	uint32_t flag;
	uint32_t l_seq;
	uint32_t seq_off; // of its packed bases
};

// the record at raw[p], p <= n < 2^31: BAM_NEXT and its fields, BAM_END (it does not lie completely inside), or the rule
// it breaks
BAM_HD uint32_t
bam_hop(const uint8_t* raw, uint32_t n, uint32_t p, BamRecord* r)
{
	const uint32_t left = n - p;
	if (left < 4) {
		return BAM_END;
	}
	const uint32_t block = bam_ld32(raw + p);
	if (block >= BAM_MAX_BLOCK) {
		return BAM_BAD_SIZE;
	}
	if (block < 32) {
		return BAM_BAD_RECORD;
	}
	if (left < 36) {
		return BAM_END;
	}
	const uint32_t l_read_name = raw[p + 12], n_cigar = bam_ld16(raw + p + 16), l_seq = bam_ld32(raw + p + 20);
	const uint64_t head = 32ull + l_read_name + 4ull * n_cigar;
	if (l_read_name < 1 || head + ((uint64_t)l_seq + 1) / 2 + l_seq > block) {
		return BAM_BAD_RECORD;
	}
	if (left - 4 < block) {
		return BAM_END;
	}
	r->next = p + 4 + block;
	r->flag = bam_ld16(raw + p + 18);
	r->l_seq = l_seq;
	r->seq_off = p + 4 + (uint32_t)head;
	return BAM_NEXT;
}

BAM_HD bool
bam_kept(uint32_t flag, uint32_t l_seq, uint32_t min_len)
{
	return (flag & 0x900u) == 0 && l_seq >= min_len;
}

// base j of the packed bases at seq_off
BAM_HD char
bam_base(const uint8_t* raw, uint32_t seq_off, uint32_t j)
{
	const uint32_t b = raw[seq_off + (j >> 1)];
	return "=ACMGRSVTWYHKDBN"[(j & 1) ? (b & 15u) : (b >> 4)];
}

// --min_qual: the record's l_seq quality bytes (Phred, as stored) lie right behind its packed bases
BAM_HD uint32_t
bam_qual_off(uint32_t seq_off, uint32_t l_seq)
{
	return seq_off + (l_seq + 1) / 2;
}

// SAM specification 4.2.3: a first quality byte of 0xFF says the record has no qualities (qual_off: bam_qual_off of it)
BAM_HD bool
bam_has_qual(const uint8_t* raw, uint32_t qual_off, uint32_t l_seq)
{
	return l_seq > 0 && raw[qual_off] != 0xFFu;
}

// base j of a record that has qualities, as it enters the text under --min_qual: the one rule of nte_reads_grammar.h on
// the quality byte as stored; *n_masked += 1 when it is masked (whatever the base was)
BAM_HD char
bam_base_q(const uint8_t* raw, uint32_t seq_off, uint32_t qual_off, uint32_t j, uint32_t min_qual, uint32_t* n_masked)
{
	const bool low = nte_parse::rp_masked((int)raw[qual_off + j], min_qual);
	*n_masked += low;
	return (char)nte_parse::rp_mask_base((uint8_t)bam_base(raw, seq_off, j), low);
}

// --min_rq: the record's `rq` aux field of type f.  The aux fields lie in raw[aux_off .. rec_end), aux_off = qual_off +
// l_seq, and the walk reads no byte outside that range.  The SAM specification's types: A c C 1 byte, s S 2, i I f 4,
// Z H to a NUL, B a subtype, a count and count * size.  A field that does not fit, or of an unknown type, ends the walk:
// BAM_RQ_MALFORMED, and the record counts as having no tag.  An rq of another type than f is walked past like any field.
enum : uint32_t { BAM_RQ_FOUND = 0, BAM_RQ_ABSENT = 1, BAM_RQ_MALFORMED = 2 };

BAM_HD uint32_t
bam_aux_size(uint32_t type) // of a fixed-size value, 0: none
{
	switch (type) {
	case 'A': case 'c': case 'C': return 1;
	case 's': case 'S': return 2;
	case 'i': case 'I': case 'f': return 4;
	default: return 0;
	}
}

BAM_HD uint32_t
bam_aux_rq(const uint8_t* raw, uint32_t aux_off, uint32_t rec_end, uint32_t* value_bits)
{
	uint32_t p = aux_off;
	while (p < rec_end) {
		if (rec_end - p < 3) {
			return BAM_RQ_MALFORMED;
		}
		const uint32_t t0 = raw[p], t1 = raw[p + 1], type = raw[p + 2];
		p += 3;
		uint32_t size = bam_aux_size(type);
		if (size) {
			if (rec_end - p < size) {
				return BAM_RQ_MALFORMED;
			}
			if (type == 'f' && t0 == 'r' && t1 == 'q') {
				*value_bits = bam_ld32(raw + p);
				return BAM_RQ_FOUND;
			}
		} else if (type == 'Z' || type == 'H') {
			while (p + size < rec_end && raw[p + size] != 0) {
				size++;
			}
			if (p + size >= rec_end) {
				return BAM_RQ_MALFORMED; // no NUL inside the record
			}
			size++;
		} else if (type == 'B') {
			if (rec_end - p < 5) {
				return BAM_RQ_MALFORMED;
			}
			const uint32_t each = raw[p] == 'A' ? 0u : bam_aux_size(raw[p]); // (the subtypes are c C s S i I f)
			const uint64_t bytes = (uint64_t)each * bam_ld32(raw + p + 1);
			if (each == 0 || bytes > rec_end - p - 5) {
				return BAM_RQ_MALFORMED;
			}
			size = 5 + (uint32_t)bytes;
		} else {
			return BAM_RQ_MALFORMED;
		}
		p += size;
	}
	return BAM_RQ_ABSENT;
}

// `value` (the bits of an IEEE float) >= `min` (alike), as the floats compare: a NaN is below everything
BAM_HD bool
bam_rq_kept(uint32_t value_bits, uint32_t min_bits)
{
	union { uint32_t u; float f; } v, m;
	v.u = value_bits;
	m.u = min_bits;
	return v.f >= m.f;
}

// what the filter needs to know of a record besides its flag and length
struct BamFacts
{
	uint32_t rq_status; // bam_aux_rq's
	uint32_t rq_bits;
	bool has_qual;      // bam_has_qual
	uint64_t qual_sum;  // of rp_qual_weight over its quality bytes
};

// RP_KEPT, or the first rule that drops the record: flag, length, rq, mean quality
BAM_HD uint32_t
bam_reason(uint32_t flag, uint32_t l_seq, uint32_t min_len, const nte_parse::ReadFilter& f, const BamFacts& x)
{
	if (flag & 0x900u) {
		return nte_parse::RP_DROP_FLAG;
	}
	if (l_seq < nte_parse::rp_min_len(f, min_len)) {
		return nte_parse::RP_DROP_LENGTH;
	}
	if (f.rq_bits && x.rq_status == BAM_RQ_FOUND && !bam_rq_kept(x.rq_bits, f.rq_bits)) {
		return nte_parse::RP_DROP_RQ;
	}
	if (f.min_mean_qual && x.has_qual && !nte_parse::rp_mean_qual_kept(x.qual_sum, l_seq, f.min_mean_qual)) {
		return nte_parse::RP_DROP_MEAN_QUAL;
	}
	return nte_parse::RP_KEPT;
}

BAM_HD bool
bam_kept(uint32_t flag, uint32_t l_seq, uint32_t min_len, const nte_parse::ReadFilter& f, const BamFacts& x)
{
	return bam_reason(flag, l_seq, min_len, f, x) == nte_parse::RP_KEPT;
}

// ... and for a caller that holds the reason k_bam_facts stored for the record's table slot (RP_KEPT, RP_DROP_RQ or
// RP_DROP_MEAN_QUAL: the rules that need the record's bytes), the flag and length rules in front of it as above
BAM_HD uint32_t
bam_reason(uint32_t flag, uint32_t l_seq, uint32_t min_len, const nte_parse::ReadFilter& f, uint32_t stored)
{
	if (flag & 0x900u) {
		return nte_parse::RP_DROP_FLAG;
	}
	if (l_seq < nte_parse::rp_min_len(f, min_len)) {
		return nte_parse::RP_DROP_LENGTH;
	}
	return stored;
}

// The chain from p (< end <= n) while it starts records below `end`: their offsets into table[0 .. cap), *count of them,
// *exit where the chain left [.., end) (BAM_NEXT), or where it stopped: the cut (BAM_END) or the unclean record.  The
// walk is a function of (raw, n, p, end): whoever enters at p writes the same table.
BAM_HD uint32_t
bam_walk(const uint8_t* raw, uint32_t n, uint32_t p, uint32_t end, uint32_t* table, uint32_t cap, uint32_t* count, uint32_t* exit)
{
	uint32_t c = 0, st = BAM_NEXT;
	while (p < end) {
		BamRecord r;
		st = bam_hop(raw, n, p, &r);
		if (st != BAM_NEXT) {
			break;
		}
		if (c < cap) {
			table[c] = p;
		}
		c++;
		p = r.next;
	}
	*count = c;
	*exit = p;
	return st;
}

// a guess: a whole clean record at q whose chain stays clean for BAM_GUESS_HOPS more whole records, or until fewer
// bytes are left than a record's fixed part.  A record whose fields are inside and whose end is not ends the guess: a
// block_size of hundreds of megabytes read from the middle of a sequence would pass as "cut by the chunk's end"
// otherwise, and the images of clean records it follows are common ("\xff\x09\x01\0" one byte before a true start is
// one).  The price is no guess in the last few records of a chunk, which the stitch then walks.
BAM_HD bool
bam_guess_ok(const uint8_t* raw, uint32_t n, uint32_t q)
{
	BamRecord r;
	if (bam_hop(raw, n, q, &r) != BAM_NEXT) {
		return false;
	}
	for (int h = 0; h < BAM_GUESS_HOPS && r.next < n; h++) {
		const uint32_t at = r.next, st = bam_hop(raw, n, at, &r);
		if (st == BAM_END) {
			return n - at < 36;
		}
		if (st != BAM_NEXT) {
			return false;
		}
	}
	return true;
}

// the slots a segment's slice of the offset table needs: no record is shorter than BAM_MIN_RECORD
BAM_HD uint32_t
bam_slice_cap(uint32_t segment)
{
	return segment / BAM_MIN_RECORD + 2;
}

struct BamResult // (ntedit_hip_reads_bam_result, field for field)
{
	int clean;
	uint32_t broken;
	uint64_t header_len;
	uint32_t n_ref, reserved;
	uint64_t cut, records, kept, skipped_flag, skipped_short, bases, text_len;
};

BAM_HD BamResult
bam_unclean(uint32_t broken, uint64_t at)
{
	BamResult r = BamResult();
	r.broken = broken;
	r.cut = at; // where the rule is broken
	return r;
}

// (host only from here on)
// The model: one chain from the true entry, one pass over its records.  The text into out[0 .. cap) as far as it fits;
// res->text_len is its whole length either way.
// With min_qual > 0 the bases of the records that have qualities are masked (bam_base_q); counts[0] += those bases,
// counts[1] += the masked ones (counts may be NULL).
// With a filter (bam_reason) a record dropped by rq or by its mean quality is in res->records and in no other field of
// res; fc (may be NULL) += what the records came to: those the flag rule let through, the drops per rule, the records
// that reached the rq rule and had an rq:f field, and those of them whose aux fields were malformed.  --min_qual's counts cover the records copied.
inline void
bam_model_f(const uint8_t* raw, uint64_t n, int at_header, uint32_t min_len, uint32_t min_qual, const nte_parse::ReadFilter& f, char* out,
            uint64_t cap, BamResult* res, uint64_t* counts, nte_parse::ReadFilterCounts* fc)
{
	*res = BamResult();
	if (n >= BAM_MAX_RAW) {
		*res = bam_unclean(BAM_BAD_SIZE, 0);
		return;
	}
	uint64_t entry = 0;
	if (at_header) {
		const uint32_t st = bam_header(raw, n, &res->header_len, &res->n_ref);
		if (st == BAM_END) {
			res->clean = 1; // cut 0: the chunk grows
			return;
		}
		if (st != BAM_NEXT) {
			*res = bam_unclean(st, 0);
			return;
		}
		entry = res->header_len;
	}
	uint32_t p = (uint32_t)entry;
	uint64_t text = 0;
	while (p < n) {
		BamRecord r;
		const uint32_t st = bam_hop(raw, (uint32_t)n, p, &r);
		if (st == BAM_END) {
			break;
		}
		if (st != BAM_NEXT) {
			*res = bam_unclean(st, p);
			return;
		}
		res->records++;
		const uint32_t qual_off = bam_qual_off(r.seq_off, r.l_seq);
		BamFacts x = BamFacts();
		x.rq_status = BAM_RQ_ABSENT;
		const bool filtered = nte_parse::rp_filter_on(f) && !(r.flag & 0x900u);
		// (a record the length rule drops is not looked into: its tag and its qualities decide nothing)
		const bool look = filtered && bam_reason(r.flag, r.l_seq, min_len, f, (uint32_t)nte_parse::RP_KEPT) == nte_parse::RP_KEPT;
		if (look && f.rq_bits) {
			x.rq_status = bam_aux_rq(raw, qual_off + r.l_seq, r.next, &x.rq_bits);
		}
		if (look && f.min_mean_qual && (x.has_qual = bam_has_qual(raw, qual_off, r.l_seq))) {
			for (uint32_t j = 0; j < r.l_seq; j++) {
				x.qual_sum += nte_parse::rp_qual_weight((int)raw[qual_off + j]);
			}
		}
		const uint32_t why = bam_reason(r.flag, r.l_seq, min_len, f, x);
		if (filtered && fc) {
			fc->records++;
			fc->by_length += why == nte_parse::RP_DROP_LENGTH;
			fc->by_rq += why == nte_parse::RP_DROP_RQ;
			fc->by_mean_qual += why == nte_parse::RP_DROP_MEAN_QUAL;
			fc->rq_tagged += x.rq_status == BAM_RQ_FOUND;
			fc->aux_malformed += x.rq_status == BAM_RQ_MALFORMED;
		}
		if (why == nte_parse::RP_DROP_FLAG) {
			res->skipped_flag++;
		} else if (why == nte_parse::RP_DROP_LENGTH) {
			res->skipped_short++;
		} else if (why == nte_parse::RP_KEPT) {
			res->kept++;
			res->bases += r.l_seq;
			const bool mask = min_qual && bam_has_qual(raw, qual_off, r.l_seq);
			uint32_t masked = 0;
			for (uint32_t j = 0; j <= r.l_seq; j++, text++) {
				char ch = '\n';
				if (j < r.l_seq) {
					ch = mask ? bam_base_q(raw, r.seq_off, qual_off, j, min_qual, &masked) : bam_base(raw, r.seq_off, j);
				}
				if (text < cap) {
					out[text] = ch;
				}
			}
			if (mask && counts) {
				counts[0] += r.l_seq;
				counts[1] += masked;
			}
		}
		p = r.next;
	}
	res->clean = 1;
	res->cut = p;
	res->text_len = text;
}

inline void
bam_model_q(const uint8_t* raw, uint64_t n, int at_header, uint32_t min_len, uint32_t min_qual, char* out, uint64_t cap, BamResult* res,
            uint64_t* counts)
{
	bam_model_f(raw, n, at_header, min_len, min_qual, nte_parse::ReadFilter(), out, cap, res, counts, nullptr);
}

inline void
bam_model(const uint8_t* raw, uint64_t n, int at_header, uint32_t min_len, char* out, uint64_t cap, BamResult* res)
{
	bam_model_q(raw, n, at_header, min_len, 0, out, cap, res, nullptr);
}

// The first BGZF member of buf[0 .. n) (a gzip member with FEXTRA and a 'B','C' subfield of the member's size - 1): where
// its DEFLATE data lies, its ISIZE and CRC-32; false when there is none that lies completely inside.
inline bool
bam_first_member(const uint8_t* buf, uint64_t n, uint64_t* in_off, uint32_t* n_in, uint32_t* n_out, uint32_t* crc)
{
	if (n < 12 + 8 || buf[0] != 0x1f || buf[1] != 0x8b || buf[2] != 8 || buf[3] != 4) {
		return false;
	}
	const uint64_t xlen = bam_ld16(buf + 10);
	if (n < 12 + xlen) {
		return false;
	}
	uint64_t member = 0;
	for (uint64_t x = 12; x + 4 <= 12 + xlen;) {
		const uint64_t slen = bam_ld16(buf + x + 2);
		if (buf[x] == 'B' && buf[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) {
			member = (uint64_t)bam_ld16(buf + x + 4) + 1;
		}
		x += 4 + slen;
	}
	if (member < 12 + xlen + 8 || member > n) {
		return false;
	}
	*in_off = 12 + xlen;
	*n_in = (uint32_t)(member - 12 - xlen - 8);
	*crc = bam_ld32(buf + member - 8);
	*n_out = bam_ld32(buf + member - 4);
	return *n_out <= 65536;
}

// whether buf[0 .. n), the start of a file, begins with BGZF members that inflate to "BAM\1" (the inflate model, one
// lane; the members' CRCs are not looked at: the pass checks them on the device).  Members are inflated, one after the
// other, until four bytes are at hand: a first member of one to three bytes, or of none, is legal BGZF.  The members that
// hold those four bytes have to lie completely inside buf.
inline bool
bam_starts_bam(const uint8_t* buf, uint64_t n)
{
	const uint8_t magic[4] = { 'B', 'A', 'M', 1 };
	nte_bgzf::BzTables* t = new nte_bgzf::BzTables();
	uint64_t at = 0;
	uint32_t have = 0;
	bool bam = true;
	while (bam && have < 4) {
		uint64_t in_off = 0;
		uint32_t n_in = 0, n_out = 0, crc = 0;
		if (!bam_first_member(buf + at, n - at, &in_off, &n_in, &n_out, &crc)) {
			bam = false;
			break;
		}
		if (n_out) {
			uint8_t* out = new uint8_t[n_out];
			bam = nte_bgzf::bz_inflate(buf + at + in_off, n_in, out, n_out, t, 0, 1) == nte_bgzf::BZ_OK;
			for (uint32_t i = 0; bam && i < n_out && have < 4; i++, have++) {
				bam = out[i] == magic[have];
			}
			delete[] out;
		}
		at += in_off + n_in + 8;
	}
	delete t;
	return bam;
}

} // namespace nte_bam
