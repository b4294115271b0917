// nte_reads_bam.hip -- gfx950 kernels and C ABI of --gpu_parse on BAM reads: in an inflated chunk (nte_reads_inflate.hip)
// the records are found and the kept ones' 4-bit bases unpacked into the batch text the passes consume.  The grammar is
// nte_bam_grammar.h, written once for the kernels and for the serial host model (ntedit_hip_reads_bam_model, below).
//
// The chain of block_size fields is serial, so it is walked speculatively and stitched:
//   k_bam_header   one lane: the header's length and n_ref (once per file: the reference list is a chain of its own).
//   k_bam_walk     one wavefront per segment, four per workgroup.  The 64 lanes test 64 offsets at a time for a clean
//                  record (coalesced reads of the segment, which stays in the CU's L1 for what follows), the first whose
//                  chain stays clean for a few hops is the segment's guess, and lane 0 walks from it, writing record
//                  offsets to the segment's slice of the table and where the chain left the segment.  The segment that
//                  holds the true entry starts from it.
//   k_bam_stitch   one wavefront.  64 segments' guesses and exits at a time are loaded coalesced into LDS; lane 0 follows
//                  the true chain through them at LDS latency: exit == the next segment's guess keeps that segment's
//                  table (the walk is a function of its entry), anything else walks that segment again from the true
//                  entry.  It marks the segments on the chain, and ends with the cut or the rule a record broke.
//   k_bam_facts    (--min_rq, --min_mean_qual) one wavefront per segment on the chain, a group of 8, 16 or 64 lanes per
//                  record: the weights of its quality bytes summed over the group, its aux fields walked for rq by the
//                  group's first lane; one byte per table slot, the rule that drops the record or 0.
//   k_bam_sums     one wavefront per segment on the chain, a lane per record: kept records and text bytes of the segment
//                  (k_bam_sums<true>, k_bam_compact<true>: with the read filter, by bam_reason and the slot bytes).
//   k_bam_scan     one workgroup: the exclusive scan of those over the segments.
//   k_bam_compact  as k_bam_sums, with a wavefront scan: each kept record's packed-bases offset and text offset, dense.
//   k_bam_decode   one lane per 16 text bytes, whatever the records' lengths: a search in the text-offset table for the
//                  record its first byte lies in, then nibbles to bytes across record ends, one 16-byte store.
//                  k_bam_decode<true> (--min_qual) also masks each base by its quality byte, which lies behind the
//                  record's packed bases.
//
// Like nte_reads_inflate.hip this unit is outside KSRC and sees no context internals: its state hangs off the context
// pointer, its scratch grows only and goes with ntedit_hip_sketch_free.  It works on the parse unit's stream.
#include "nte_common.h"
#include "nte_bam_grammar.h"
#include "nte_bgzf_inflate.h"

#include "nte_reads_internal.h"
#include "nte_reads_unit.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace nte;
using namespace nte_bam;
using namespace nte_unit;

namespace {

constexpr int BAM_TPB = 256;
constexpr int BAM_WAVES = BAM_TPB / 64;
constexpr u32 BAM_WINDOW = 64; // segments the stitch resolves per load

static_assert(NTEDIT_BAM_BAD_MAGIC == BAM_BAD_MAGIC && NTEDIT_BAM_BAD_HEADER == BAM_BAD_HEADER && NTEDIT_BAM_BAD_RECORD == BAM_BAD_RECORD &&
                  NTEDIT_BAM_BAD_SIZE == BAM_BAD_SIZE,
              "the header names the grammar's rules");
static_assert(sizeof(ntedit_hip_reads_bam_result) == sizeof(BamResult), "the result is the grammar's, field for field");

struct BamInfo // the small result the device keeps per chunk
{
	u32 hdr_status, n_ref;
	u64 header_len;
	u32 broken, cut, rewalked, reserved;
	u64 records, kept, skipped_flag, skipped_short;
	u64 qual_bases, masked_bases; // --min_qual (k_bam_decode<true>): the bases decoded that had a quality, and those masked
	// --min_rq, --min_mean_qual (k_bam_facts, k_bam_sums<true>): the drops by those rules, the records that had an rq:f
	// field, and those whose aux fields were malformed
	u64 by_rq, by_mean_qual, rq_tagged, aux_malformed;
};

struct SegTables // per segment
{
	u32 *guess, *exit, *count, *status, *valid;
	u32* table; // cap offsets per segment
	u8* reason; // --min_rq, --min_mean_qual: one byte per table slot (k_bam_facts)
	u64* pack;  // (kept records << 32 | text bytes) of the segment, then their exclusive scan; [nseg]: the totals
};

__global__ void
k_bam_header(const u8* __restrict__ raw, u32 n, BamInfo* info)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		u64 len = 0;
		u32 refs = 0;
		info->hdr_status = bam_header(raw, n, &len, &refs);
		info->header_len = len;
		info->n_ref = refs;
	}
}

__global__ __launch_bounds__(BAM_TPB) void
k_bam_walk(const u8* __restrict__ raw, u32 n, u32 seg_bytes, u32 nseg, u32 entry, u32 cap, SegTables t)
{
	const u32 lane = threadIdx.x & 63, seg = blockIdx.x * BAM_WAVES + (threadIdx.x >> 6);
	if (seg >= nseg) {
		return;
	}
	const u64 a64 = (u64)seg * seg_bytes, b64 = a64 + seg_bytes;
	const u32 a = (u32)a64, b = b64 < n ? (u32)b64 : n;
	u32 g = BAM_NO_GUESS;
	if (entry >= b) {
		// in front of the true entry: nothing starts here
	} else if (entry >= a) {
		g = entry;
	} else {
		for (u32 base = a; base < b && g == BAM_NO_GUESS; base += 64) {
			const u32 q = base + lane;
			BamRecord r;
			const bool ok = q < b && bam_hop(raw, n, q, &r) == BAM_NEXT;
			u64 m = __ballot(ok);
			while (m) { // (uniform: every lane follows the same candidate)
				const u32 i = (u32)__ffsll((unsigned long long)m) - 1;
				m &= m - 1;
				if (bam_guess_ok(raw, n, base + i)) {
					g = base + i;
					break;
				}
			}
		}
	}
	if (lane == 0) {
		u32 count = 0, exit = 0, st = BAM_NEXT;
		if (g != BAM_NO_GUESS) {
			st = bam_walk(raw, n, g, b, t.table + (u64)seg * cap, cap, &count, &exit);
		}
		t.guess[seg] = g;
		t.exit[seg] = exit;
		t.count[seg] = count;
		t.status[seg] = st;
	}
}

__global__ __launch_bounds__(64) void
k_bam_stitch(const u8* __restrict__ raw, u32 n, u32 seg_bytes, u32 nseg, u32 entry, u32 cap, SegTables t, BamInfo* info)
{
	__shared__ u32 s_guess[BAM_WINDOW], s_exit[BAM_WINDOW], s_status[BAM_WINDOW];
	__shared__ u32 s_cur, s_done;
	const u32 lane = threadIdx.x;
	if (lane == 0) {
		s_cur = entry;
		s_done = 0;
	}
	__syncthreads();
	u32 rewalked = 0;
	for (;;) {
		const u32 cur = s_cur;
		if (s_done) {
			break;
		}
		if (cur >= n) { // the chain ends with the chunk
			if (lane == 0) {
				info->cut = n;
			}
			break;
		}
		const u32 w0 = cur / seg_bytes;
		if (w0 + lane < nseg) {
			s_guess[lane] = t.guess[w0 + lane];
			s_exit[lane] = t.exit[w0 + lane];
			s_status[lane] = t.status[w0 + lane];
		}
		__syncthreads();
		if (lane == 0) {
			u32 p = cur;
			while (p < n) {
				const u32 seg = p / seg_bytes;
				if (seg >= w0 + BAM_WINDOW) {
					break;
				}
				u32 st, next;
				if (s_guess[seg - w0] == p) {
					st = s_status[seg - w0];
					next = s_exit[seg - w0];
				} else {
					const u64 b64 = ((u64)seg + 1) * seg_bytes;
					u32 count = 0;
					st = bam_walk(raw, n, p, b64 < n ? (u32)b64 : n, t.table + (u64)seg * cap, cap, &count, &next);
					t.count[seg] = count;
					rewalked++;
				}
				t.valid[seg] = 1;
				p = next;
				if (st != BAM_NEXT) {
					info->cut = next; // the first record not completely inside, or the unclean one
					info->broken = st == BAM_END ? 0 : st;
					s_done = 1;
					break;
				}
			}
			s_cur = p;
		}
		__syncthreads();
	}
	if (lane == 0) {
		info->rewalked = rewalked;
	}
}

__device__ __forceinline__ u64
wave_sum(u64 v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		v += __shfl_xor(v, d, 64);
	}
	return v;
}

__device__ __forceinline__ u64
group_sum(u64 v, int width) // over each aligned group of `width` lanes (a power of two)
{
	for (int d = 1; d < width; d <<= 1) {
		const u32 lo = __shfl_xor((u32)v, d, 64), hi = __shfl_xor((u32)(v >> 32), d, 64);
		v += ((u64)hi << 32) | lo;
	}
	return v;
}

// --min_rq, --min_mean_qual: the rules that need a record's bytes, ahead of k_bam_sums.  One wavefront per segment on the
// chain, as k_bam_sums walks them; a group of WIDTH lanes (8, 16 or 64: the host chooses by the reads' mean length) per
// record, 64 / WIDTH records at a time.  The group's lanes share the record's l_seq quality bytes -- the unaligned head
// and tail a byte per lane, the body in aligned 16-byte loads -- and sum the weights over the
// group; the group's first lane walks the aux fields for rq (tens of bytes; arrays are skipped by their counts) and
// stores the slot's byte: RP_KEPT, RP_DROP_RQ or RP_DROP_MEAN_QUAL.  A record the flag or the length rule drops is not
// looked into (its byte is RP_KEPT; k_bam_sums and k_bam_compact apply those two rules in front of it: bam_reason).
// Every record in the tables passed bam_hop, so its quality bytes and r.next lie inside the chunk.
template <int WIDTH>
__global__ __launch_bounds__(BAM_TPB) void
k_bam_facts(const u8* __restrict__ raw, u32 n, u32 nseg, u32 cap, u32 min_len, nte_parse::ReadFilter f, SegTables t, BamInfo* info)
{
	__shared__ u32 s_weight[nte_parse::RP_MAX_QUAL + 1];
	if (threadIdx.x <= nte_parse::RP_MAX_QUAL) {
		s_weight[threadIdx.x] = nte_parse::RP_QUAL_WEIGHT[threadIdx.x];
	}
	__syncthreads();
	const u32 lane = threadIdx.x & 63, seg = blockIdx.x * BAM_WAVES + (threadIdx.x >> 6);
	if (seg >= nseg) { // (a whole wavefront: the shuffles below stay among lanes that are all here)
		return;
	}
	constexpr u32 GROUPS = 64 / WIDTH;
	const u32 g = lane / WIDTH, gl = lane % WIDTH;
	const u32 count = t.valid[seg] ? t.count[seg] : 0;
	u64 tagged = 0, malformed = 0;
	for (u32 j0 = 0; j0 < count; j0 += GROUPS) { // (uniform over the wavefront)
		const u32 j = j0 + g;
		BamRecord r = BamRecord();
		bool look = false;
		if (j < count) {
			(void)bam_hop(raw, n, t.table[(u64)seg * cap + j], &r); // (BAM_NEXT: the walk stored it)
			look = bam_reason(r.flag, r.l_seq, min_len, f, (u32)nte_parse::RP_KEPT) == nte_parse::RP_KEPT;
		}
		const u32 q0 = bam_qual_off(r.seq_off, r.l_seq), q1 = q0 + r.l_seq;
		BamFacts x = BamFacts();
		x.rq_status = BAM_RQ_ABSENT;
		x.has_qual = look && f.min_mean_qual && bam_has_qual(raw, q0, r.l_seq);
		u64 sum = 0;
		if (x.has_qual) {
			const u32 mis = (u32)((uintptr_t)raw & 15u); // (0 for a chunk that starts its buffer)
			u32 a0 = ((q0 + mis + 15u) & ~15u) - mis; // the aligned body is [a0, a1)
			a0 = a0 < q1 ? a0 : q1;
			const u32 a1 = a0 + ((q1 - a0) & ~15u);
			for (u32 p = q0 + gl; p < a0; p += WIDTH) {
				sum += s_weight[nte_parse::rp_qual_index((int)raw[p])];
			}
			for (u32 p = a0 + gl * 16; p < a1; p += WIDTH * 16) {
				const uint4 v = *reinterpret_cast<const uint4*>(raw + p);
				const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
				for (int b = 0; b < 16; b++) {
					sum += s_weight[nte_parse::rp_qual_index((int)((w[b >> 2] >> (8 * (b & 3))) & 0xFFu))];
				}
			}
			for (u32 p = a1 + gl; p < q1; p += WIDTH) {
				sum += s_weight[nte_parse::rp_qual_index((int)raw[p])];
			}
		}
		x.qual_sum = group_sum(sum, WIDTH);
		if (gl == 0 && j < count) {
			if (look && f.rq_bits) {
				x.rq_status = bam_aux_rq(raw, q1, r.next, &x.rq_bits);
				tagged += x.rq_status == BAM_RQ_FOUND;
				malformed += x.rq_status == BAM_RQ_MALFORMED;
			}
			t.reason[(u64)seg * cap + j] = look ? (u8)bam_reason(r.flag, r.l_seq, min_len, f, x) : (u8)nte_parse::RP_KEPT;
		}
	}
	tagged = wave_sum(tagged);
	malformed = wave_sum(malformed);
	if (lane == 0 && (tagged || malformed)) {
		atomicAdd((unsigned long long*)&info->rq_tagged, (unsigned long long)tagged);
		atomicAdd((unsigned long long*)&info->aux_malformed, (unsigned long long)malformed);
	}
}

// FILTER: the slot bytes of k_bam_facts behind the flag and the length rule (bam_reason); f.min_len alone needs no bytes
template <bool FILTER>
__global__ __launch_bounds__(BAM_TPB) void
k_bam_sums(const u8* __restrict__ raw, u32 n, u32 nseg, u32 cap, u32 min_len, SegTables t, BamInfo* info, nte_parse::ReadFilter f,
           const u8* __restrict__ reason)
{
	const u32 lane = threadIdx.x & 63, seg = blockIdx.x * BAM_WAVES + (threadIdx.x >> 6);
	if (seg >= nseg) {
		return;
	}
	const u32 count = t.valid[seg] ? t.count[seg] : 0;
	u64 kept = 0, text = 0, by_flag = 0, by_len = 0, by_rq = 0, by_mq = 0;
	for (u32 j = lane; j < count; j += 64) {
		BamRecord r;
		(void)bam_hop(raw, n, t.table[(u64)seg * cap + j], &r); // (BAM_NEXT: the walk stored it)
		if (FILTER) {
			const u32 why = bam_reason(r.flag, r.l_seq, min_len, f, reason ? (u32)reason[(u64)seg * cap + j] : (u32)nte_parse::RP_KEPT);
			by_flag += why == nte_parse::RP_DROP_FLAG;
			by_len += why == nte_parse::RP_DROP_LENGTH;
			by_rq += why == nte_parse::RP_DROP_RQ;
			by_mq += why == nte_parse::RP_DROP_MEAN_QUAL;
			if (why == nte_parse::RP_KEPT) {
				kept++;
				text += (u64)r.l_seq + 1;
			}
		} else if (r.flag & 0x900u) {
			by_flag++;
		} else if (r.l_seq < min_len) {
			by_len++;
		} else {
			kept++;
			text += (u64)r.l_seq + 1;
		}
	}
	kept = wave_sum(kept);
	text = wave_sum(text);
	by_flag = wave_sum(by_flag);
	by_len = wave_sum(by_len);
	if (FILTER) {
		by_rq = wave_sum(by_rq);
		by_mq = wave_sum(by_mq);
	}
	if (lane == 0) {
		t.pack[seg] = kept << 32 | text;
		if (count) {
			atomicAdd((unsigned long long*)&info->records, (unsigned long long)count);
			atomicAdd((unsigned long long*)&info->kept, (unsigned long long)kept);
			atomicAdd((unsigned long long*)&info->skipped_flag, (unsigned long long)by_flag);
			atomicAdd((unsigned long long*)&info->skipped_short, (unsigned long long)by_len);
			if (FILTER && (by_rq || by_mq)) {
				atomicAdd((unsigned long long*)&info->by_rq, (unsigned long long)by_rq);
				atomicAdd((unsigned long long*)&info->by_mean_qual, (unsigned long long)by_mq);
			}
		}
	}
}

// pack[0 .. nseg) to its exclusive scan in place, pack[nseg] = the totals; krec_text[kept] = the text's length
__global__ __launch_bounds__(BAM_TPB) void
k_bam_scan(u64* pack, u32 nseg, u32* krec_text)
{
	__shared__ u64 s[BAM_TPB];
	const u32 tid = threadIdx.x;
	u64 carry = 0;
	for (u32 base = 0; base < nseg; base += BAM_TPB) {
		const u64 v = base + tid < nseg ? pack[base + tid] : 0;
		s[tid] = v;
		__syncthreads();
		for (u32 d = 1; d < BAM_TPB; d <<= 1) {
			const u64 add = tid >= d ? s[tid - d] : 0;
			__syncthreads();
			s[tid] += add;
			__syncthreads();
		}
		if (base + tid < nseg) {
			pack[base + tid] = carry + s[tid] - v;
		}
		carry += s[BAM_TPB - 1];
		__syncthreads();
	}
	if (tid == 0) {
		pack[nseg] = carry;
		krec_text[carry >> 32] = (u32)carry;
	}
}

template <bool FILTER>
__global__ __launch_bounds__(BAM_TPB) void
k_bam_compact(const u8* __restrict__ raw, u32 n, u32 nseg, u32 cap, u32 min_len, SegTables t, u32* __restrict__ krec_seq,
              u32* __restrict__ krec_text, nte_parse::ReadFilter f, const u8* __restrict__ reason)
{
	const u32 lane = threadIdx.x & 63, seg = blockIdx.x * BAM_WAVES + (threadIdx.x >> 6);
	if (seg >= nseg) {
		return;
	}
	const u32 count = t.valid[seg] ? t.count[seg] : 0;
	u32 kb = (u32)(t.pack[seg] >> 32), tb = (u32)t.pack[seg];
	for (u32 j0 = 0; j0 < count; j0 += 64) {
		const u32 j = j0 + lane;
		BamRecord r = BamRecord();
		bool keep = false;
		if (j < count) {
			(void)bam_hop(raw, n, t.table[(u64)seg * cap + j], &r);
			if (FILTER) {
				keep = bam_reason(r.flag, r.l_seq, min_len, f, reason ? (u32)reason[(u64)seg * cap + j] : (u32)nte_parse::RP_KEPT) ==
				       nte_parse::RP_KEPT;
			} else {
				keep = bam_kept(r.flag, r.l_seq, min_len);
			}
		}
		const u32 len = keep ? r.l_seq + 1 : 0;
		u32 ik = keep ? 1 : 0, il = len; // inclusive scans over the lanes
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const u32 uk = __shfl_up(ik, d, 64), ul = __shfl_up(il, d, 64);
			if (lane >= (u32)d) {
				ik += uk;
				il += ul;
			}
		}
		if (keep) {
			krec_seq[kb + ik - 1] = r.seq_off;
			krec_text[kb + ik - 1] = tb + il - len;
		}
		kb += __shfl(ik, 63, 64);
		tb += __shfl(il, 63, 64);
	}
}

// MASK (--min_qual): base i of a record is masked by the quality byte at krec_seq[r] + (l_seq + 1) / 2 + i (bam_base_q),
// l_seq from the text offsets; a record whose first quality byte is 0xFF has none.  Every record in the tables passed
// bam_hop, so its quality bytes lie inside the chunk.  The counts are summed per wavefront, one atomic each per wavefront.
template <bool MASK>
__global__ __launch_bounds__(BAM_TPB) void
k_bam_decode(const u8* __restrict__ raw, const u32* __restrict__ krec_seq, const u32* __restrict__ krec_text, u32 kept, u8* text,
             u32 text_len, u32 min_qual, BamInfo* info)
{
	const u64 t0 = ((u64)blockIdx.x * BAM_TPB + threadIdx.x) * 16;
	u32 n_qual = 0, n_masked = 0;
	if (t0 < text_len) {
		// the last record whose text starts at or before t0 (text offsets rise strictly: every kept record has its '\n')
		u32 lo = 0, hi = kept;
		while (hi - lo > 1) {
			const u32 mid = lo + (hi - lo) / 2;
			if (krec_text[mid] <= (u32)t0) {
				lo = mid;
			} else {
				hi = mid;
			}
		}
		u32 rec = lo, start = krec_text[rec], end = krec_text[rec + 1], seq = krec_seq[rec];
		// the record's quality bytes and whether it has any: derived where the lane enters a record, not per base
		u32 qual = MASK ? bam_qual_off(seq, end - start - 1) : 0;
		bool has_qual = MASK && bam_has_qual(raw, qual, end - start - 1);
		const u32 todo = text_len - (u32)t0 < 16 ? text_len - (u32)t0 : 16;
		u32 w[4] = { 0, 0, 0, 0 };
		for (u32 i = 0; i < todo; i++) {
			const u32 at = (u32)t0 + i;
			if (at == end) {
				rec++;
				start = end;
				end = krec_text[rec + 1];
				seq = krec_seq[rec];
				if (MASK) {
					qual = bam_qual_off(seq, end - start - 1);
					has_qual = bam_has_qual(raw, qual, end - start - 1);
				}
			}
			u32 ch = (u32)'\n';
			if (at + 1 != end) {
				if (MASK && has_qual) {
					n_qual++;
					ch = (u32)(u8)bam_base_q(raw, seq, qual, at - start, min_qual, &n_masked);
				} else {
					ch = (u32)(u8)bam_base(raw, seq, at - start);
				}
			}
			w[i >> 2] |= ch << ((i & 3) * 8);
		}
		if (todo == 16) {
			*(uint4*)(text + t0) = make_uint4(w[0], w[1], w[2], w[3]);
		} else {
			for (u32 i = 0; i < todo; i++) {
				text[t0 + i] = (u8)(w[i >> 2] >> ((i & 3) * 8));
			}
		}
	}
	if (MASK) {
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			n_qual += __shfl_xor(n_qual, d, 64);
			n_masked += __shfl_xor(n_masked, d, 64);
		}
		if ((threadIdx.x & 63) == 0 && n_qual) {
			atomicAdd((unsigned long long*)&info->qual_bases, (unsigned long long)n_qual);
			atomicAdd((unsigned long long*)&info->masked_bases, (unsigned long long)n_masked);
		}
	}
}

// ------------------------------------------------------------------ host side
// what the calls set and the last pass counted: survives ntedit_hip_sketch_free
struct BamKeep
{
	ntedit_hip_reads_bam_stats info = {};
	u64 segment = 0;     // ntedit_hip_reads_bam_set_segment (0: the default)
	u32 group_width = 0; // ntedit_hip_reads_bam_set_group_width (0: by the reads' mean length)
};

// device scratch, grow-only, released by ntedit_hip_sketch_free
struct BamScratch
{
	u32 last_width = 0; // the width the last k_bam_facts ran at (ntedit_hip_reads_bam_group_width)
	u32 mean_l_seq = 0; // of the records the last chunk kept (0: no chunk yet): what the next chunk's width goes by
	int device = -1;
	hipStream_t stream = nullptr; // the parse unit's
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
	DevBuf seg; // the per-segment arrays and the table
	DevBuf rec; // the kept records' two arrays
	DevBuf in;  // a chunk given as host bytes
	BamInfo* d_info = nullptr;
	BamInfo* h_info = nullptr; // page-locked
	u64* h_total = nullptr;    // page-locked
};

typedef State<BamKeep, BamScratch> BamState;
Registry<BamState> g_bam;

int
ensure_device(const ntedit_hip_ctx* c, BamScratch* s)
{
	if (s->device >= 0) {
		NTE_TRY(c, hipSetDevice(s->device));
		return 0;
	}
	void *stream = nullptr, *copy_stream = nullptr;
	const int rc = nte_reads::parse_streams(c, &stream, &copy_stream);
	if (rc) {
		return rc;
	}
	int device = 0;
	NTE_TRY(c, hipGetDevice(&device));
	s->stream = (hipStream_t)stream;
	for (hipEvent_t& e : s->ev) {
		NTE_TRY(c, hipEventCreate(&e));
	}
	NTE_TRY(c, hipMalloc((void**)&s->d_info, sizeof(BamInfo)));
	NTE_TRY(c, hipHostMalloc((void**)&s->h_info, sizeof(BamInfo), hipHostMallocDefault));
	NTE_TRY(c, hipHostMalloc((void**)&s->h_total, sizeof(u64), hipHostMallocDefault));
	s->device = device;
	return 0;
}

// the entry of every call: the context's state, its device and the parse unit's stream
int
ready(const ntedit_hip_ctx* c, BamState** state)
{
	*state = g_bam.find(c, true);
	return ensure_device(c, &(*state)->scr);
}

// buf to at least `need` bytes, by this unit's sizing rule (a quarter and 64 KiB of slack)
int
room(const ntedit_hip_ctx* c, BamScratch* s, DevBuf* buf, u64 need)
{
	return grow(c, s->stream, buf, need, (need + need / 4 + (1u << 16)) / 256 * 256);
}

void
release_scratch(BamScratch* s)
{
	if (s->device < 0) {
		return;
	}
	(void)hipSetDevice(s->device);
	if (s->stream) {
		(void)hipStreamSynchronize(s->stream);
	}
	for (hipEvent_t e : s->ev) {
		if (e) {
			(void)hipEventDestroy(e);
		}
	}
	for (void* p : { (void*)s->seg.p, (void*)s->rec.p, (void*)s->in.p, (void*)s->d_info }) {
		if (p) {
			(void)hipFree(p);
		}
	}
	for (void* p : { (void*)s->h_info, (void*)s->h_total }) {
		if (p) {
			(void)hipHostFree(p);
		}
	}
	*s = BamScratch();
}

// the per-segment arrays of nseg segments with `cap` table slots each, carved from one allocation
SegTables
carve(u8* base, u64 nseg, u64 cap, u64* bytes)
{
	SegTables t;
	Carver cut(base);
	t.guess = (u32*)cut.take(nseg * 4);
	t.exit = (u32*)cut.take(nseg * 4);
	t.count = (u32*)cut.take(nseg * 4);
	t.status = (u32*)cut.take(nseg * 4);
	t.valid = (u32*)cut.take(nseg * 4);
	t.pack = (u64*)cut.take((nseg + 1) * 8);
	t.table = (u32*)cut.take(nseg * cap * 4);
	t.reason = cut.take(nseg * cap);
	*bytes = cut.at;
	return t;
}

void
to_result(const BamResult& r, ntedit_hip_reads_bam_result* res)
{
	memcpy(res, &r, sizeof r);
}

// one chunk of device bytes: the walk, then the decode of the records before the cut
int
bam_on_device(const ntedit_hip_ctx* c, BamState* state, const u8* d_raw, u64 n64, int at_header, u32 min_len, u8* d_text, u64 text_cap,
              ntedit_hip_reads_bam_result* res)
{
	BamKeep& keep = state->keep;
	BamScratch* s = &state->scr;
	BamResult out = BamResult();
	if (n64 >= BAM_MAX_RAW) {
		to_result(bam_unclean(BAM_BAD_SIZE, 0), res);
		return 0;
	}
	out.clean = 1;
	if (n64 == 0) {
		to_result(out, res);
		return 0;
	}
	const u32 n = (u32)n64;
	float ms = 0;
	NTE_TRY(c, hipMemsetAsync(s->d_info, 0, sizeof(BamInfo), s->stream));
	u32 entry = 0;
	if (at_header) {
		hipLaunchKernelGGL(k_bam_header, dim3(1), dim3(64), 0, s->stream, d_raw, n, s->d_info);
		NTE_TRY(c, hipGetLastError());
		NTE_TRY(c, hipMemcpyAsync(s->h_info, s->d_info, sizeof(BamInfo), hipMemcpyDeviceToHost, s->stream));
		NTE_TRY(c, hipStreamSynchronize(s->stream));
		const u32 st = s->h_info->hdr_status;
		if (st != BAM_NEXT) {
			to_result(st == BAM_END ? out : bam_unclean(st, 0), res); // (BAM_END: cut 0, the chunk grows)
			return 0;
		}
		out.header_len = s->h_info->header_len;
		out.n_ref = s->h_info->n_ref;
		entry = (u32)out.header_len; // (inside the chunk: at most n)
	}
	u64 seg_bytes = keep.segment ? keep.segment : (u64)NTEDIT_BAM_SEGMENT;
	seg_bytes = seg_bytes > n ? n : seg_bytes;
	seg_bytes = seg_bytes < 64 ? 64 : seg_bytes;
	const u32 nseg = (u32)((n + seg_bytes - 1) / seg_bytes), cap = bam_slice_cap((u32)seg_bytes);
	u64 bytes = 0;
	(void)carve(nullptr, nseg, cap, &bytes);
	int rc = room(c, s, &s->seg, bytes);
	if (rc) {
		return rc;
	}
	const SegTables t = carve(s->seg.p, nseg, cap, &bytes);
	const unsigned seg_blocks = (nseg + BAM_WAVES - 1) / BAM_WAVES;
	// ms_walk: the walk and the stitch (the header kernel, one lane once per file, and its round trip to the host are not in it)
	NTE_TRY(c, hipEventRecord(s->ev[0], s->stream));
	NTE_TRY(c, hipMemsetAsync(t.valid, 0, (u64)nseg * 4, s->stream));
	hipLaunchKernelGGL(k_bam_walk, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, (u32)seg_bytes, nseg, entry, cap, t);
	hipLaunchKernelGGL(k_bam_stitch, dim3(1), dim3(64), 0, s->stream, d_raw, n, (u32)seg_bytes, nseg, entry, cap, t, s->d_info);
	NTE_TRY(c, hipGetLastError());
	NTE_TRY(c, hipEventRecord(s->ev[1], s->stream));
	// the lengths of the records on the chain (a chunk that turns out unclean has paid for them: it fails the pass anyway)
	NTE_TRY(c, hipEventRecord(s->ev[2], s->stream));
	const u64 max_records = (u64)n / BAM_MIN_RECORD + 2;
	if ((rc = room(c, s, &s->rec, 2 * up256(max_records * 4))) != 0) {
		return rc;
	}
	u32 *krec_seq = (u32*)s->rec.p, *krec_text = (u32*)(s->rec.p + up256(max_records * 4));
	const nte_parse::ReadFilter f = nte_reads::read_filter(c);
	const bool filtered = nte_parse::rp_filter_on(f), facts = f.rq_bits || f.min_mean_qual;
	if (facts) {
		// the lanes per record: a whole wavefront for long reads, where one record's quality bytes are thousands and a
		// narrower group would leave a few lanes with a long loop; 16 for reads of hundreds of bases (a lane has one or two
		// 16-byte loads); 8 for short reads, where wider groups idle behind the aligned body
		const u32 width = keep.group_width ? keep.group_width : s->mean_l_seq >= 2048 ? 64u : s->mean_l_seq >= 256 ? 16u : s->mean_l_seq ? 8u : 16u;
		if (width == 64) {
			hipLaunchKernelGGL(k_bam_facts<64>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, f, t, s->d_info);
		} else if (width == 16) {
			hipLaunchKernelGGL(k_bam_facts<16>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, f, t, s->d_info);
		} else {
			hipLaunchKernelGGL(k_bam_facts<8>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, f, t, s->d_info);
		}
		s->last_width = width;
	}
	const u8* reason = facts ? t.reason : nullptr;
	if (filtered) {
		hipLaunchKernelGGL(k_bam_sums<true>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, t, s->d_info, f,
		                   reason);
	} else {
		hipLaunchKernelGGL(k_bam_sums<false>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, t, s->d_info, f,
		                   reason);
	}
	hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(BAM_TPB), 0, s->stream, t.pack, nseg, krec_text);
	NTE_TRY(c, hipGetLastError());
	NTE_TRY(c, hipMemcpyAsync(s->h_info, s->d_info, sizeof(BamInfo), hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipMemcpyAsync(s->h_total, t.pack + nseg, sizeof(u64), hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	NTE_TRY(c, hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
	keep.info.ms_walk += ms;
	keep.info.chunks++;
	keep.info.segments += nseg;
	keep.info.rewalked += s->h_info->rewalked;
	if (s->h_info->broken) {
		to_result(bam_unclean(s->h_info->broken, s->h_info->cut), res);
		return 0;
	}
	out.cut = s->h_info->cut;
	out.records = s->h_info->records;
	out.kept = s->h_info->kept;
	out.skipped_flag = s->h_info->skipped_flag;
	out.skipped_short = s->h_info->skipped_short;
	out.text_len = (u32)*s->h_total;
	out.bases = out.text_len - out.kept;
	if (out.kept) {
		s->mean_l_seq = (u32)(out.bases / out.kept);
	}
	if (filtered) {
		nte_parse::ReadFilterCounts fc = nte_parse::ReadFilterCounts();
		fc.records = out.records - out.skipped_flag;
		fc.by_length = out.skipped_short;
		fc.by_rq = s->h_info->by_rq;
		fc.by_mean_qual = s->h_info->by_mean_qual;
		fc.rq_tagged = s->h_info->rq_tagged;
		fc.aux_malformed = s->h_info->aux_malformed;
		nte_reads::read_filter_count(c, 0, &fc);
	}
	if (out.kept != *s->h_total >> 32 || out.text_len > text_cap) {
		return pfail(c, NTEDIT_E_DEVICE, "reads_bam: the text does not fit its buffer");
	}
	if (out.text_len) {
		if (filtered) {
			hipLaunchKernelGGL(k_bam_compact<true>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, t, krec_seq,
			                   krec_text, f, reason);
		} else {
			hipLaunchKernelGGL(k_bam_compact<false>, dim3(seg_blocks), dim3(BAM_TPB), 0, s->stream, d_raw, n, nseg, cap, min_len, t, krec_seq,
			                   krec_text, f, reason);
		}
		const unsigned blocks = (unsigned)((out.text_len + BAM_TPB * 16 - 1) / (BAM_TPB * 16));
		const u32 min_qual = nte_reads::min_qual(c);
		if (min_qual) {
			hipLaunchKernelGGL(k_bam_decode<true>, dim3(blocks), dim3(BAM_TPB), 0, s->stream, d_raw, krec_seq, krec_text, (u32)out.kept,
			                   d_text, (u32)out.text_len, min_qual, s->d_info);
		} else {
			hipLaunchKernelGGL(k_bam_decode<false>, dim3(blocks), dim3(BAM_TPB), 0, s->stream, d_raw, krec_seq, krec_text, (u32)out.kept,
			                   d_text, (u32)out.text_len, 0u, s->d_info);
		}
		NTE_TRY(c, hipGetLastError());
		if (min_qual) { // (the counts come back with the sync below)
			NTE_TRY(c, hipMemcpyAsync(&s->h_info->qual_bases, &s->d_info->qual_bases, 2 * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
		}
	}
	NTE_TRY(c, hipEventRecord(s->ev[3], s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	nte_reads::min_qual_count(c, 0, s->h_info->qual_bases, s->h_info->masked_bases); // (zero unless the mask ran: the info is zeroed per chunk)
	NTE_TRY(c, hipEventElapsedTime(&ms, s->ev[2], s->ev[3]));
	keep.info.ms_decode += ms;
	keep.info.records += out.records;
	keep.info.kept += out.kept;
	keep.info.skipped_flag += out.skipped_flag;
	keep.info.skipped_short += out.skipped_short;
	to_result(out, res);
	return 0;
}

} // namespace

// what the pass loop of reads_pass.cpp needs beyond the public calls
namespace nte_reads {

void
bam_release(const ntedit_hip_ctx* c)
{
	BamState* s = g_bam.find(c, false);
	if (s) {
		release_scratch(&s->scr);
	}
}

ntedit_hip_reads_bam_stats*
bam_info(const ntedit_hip_ctx* c)
{
	return &g_bam.find(c, true)->keep.info;
}

int
bam_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, int at_header, uint32_t min_len, const char** text,
           ntedit_hip_reads_bam_result* res)
{
	BamState* s;
	int rc = ready(c, &s);
	char* d_text = nullptr;
	uint64_t cap = 0;
	if (rc == 0) {
		rc = parse_text_buffer(c, n, &d_text, &cap);
	}
	if (rc) {
		return rc;
	}
	*text = d_text;
	return bam_on_device(c, s, (const u8*)d_raw, n, at_header, min_len, (u8*)d_text, cap, res);
}

} // namespace nte_reads

extern "C" {

int
ntedit_hip_reads_is_bam(const char* path)
{
	if (!path) {
		return 0;
	}
	std::vector<u8> buf(65536 + 4096); // (a member is at most 64 KiB)
	FILE* fp = fopen(path, "rb");
	const size_t got = fp ? fread(buf.data(), 1, buf.size(), fp) : 0;
	if (fp) {
		fclose(fp);
	}
	return bam_starts_bam(buf.data(), got) ? 1 : 0;
}

int
ntedit_hip_reads_bam_set_segment(ntedit_hip_ctx* c, uint64_t bytes)
{
	if (!c || (bytes && bytes < 64)) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_bam_set_segment: a segment has at least 64 bytes") : NTEDIT_E_ARG;
	}
	g_bam.find(c, true)->keep.segment = bytes;
	return 0;
}

int
ntedit_hip_reads_bam_set_group_width(ntedit_hip_ctx* c, uint32_t lanes)
{
	if (!c || (lanes != 0 && lanes != 8 && lanes != 16 && lanes != 64)) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_bam_set_group_width: 0 (by the reads' mean length), 8, 16 or 64 lanes per record") : NTEDIT_E_ARG;
	}
	g_bam.find(c, true)->keep.group_width = lanes;
	return 0;
}

int
ntedit_hip_reads_bam_group_width(ntedit_hip_ctx* c)
{
	return c ? (int)g_bam.find(c, true)->scr.last_width : NTEDIT_E_ARG;
}

int
ntedit_hip_reads_bam_info(ntedit_hip_ctx* c, ntedit_hip_reads_bam_stats* st)
{
	if (!c || !st) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_bam_info: bad argument") : NTEDIT_E_ARG;
	}
	*st = g_bam.find(c, true)->keep.info;
	return 0;
}

int
ntedit_hip_reads_bam_device(ntedit_hip_ctx* c, const void* raw, uint64_t n_raw, int on_device, int at_header, uint32_t min_len,
                            char* text_device, uint64_t text_cap, ntedit_hip_reads_bam_result* res)
{
	if (!c || !res || (n_raw && (!raw || !text_device)) || text_cap < n_raw || ((uintptr_t)text_device & 15) ||
	    (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) ||
	    (on_device == NTEDIT_HIP_BASES_DEVICE && ((uintptr_t)raw & 15))) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_bam_device: bad argument") : NTEDIT_E_ARG;
	}
	BamState* st;
	int rc = ready(c, &st);
	if (rc) {
		return rc;
	}
	BamScratch* s = &st->scr;
	const u8* d_raw = (const u8*)raw;
	if (on_device == NTEDIT_HIP_BASES_HOST && n_raw && n_raw < BAM_MAX_RAW) { // (its own buffer and sizing rule: not the parse unit's staging)
		if ((rc = room(c, s, &s->in, n_raw)) != 0) {
			return rc;
		}
		NTE_TRY(c, hipMemcpyAsync(s->in.p, raw, n_raw, hipMemcpyHostToDevice, s->stream));
		d_raw = s->in.p;
	}
	return bam_on_device(c, st, d_raw, n_raw, at_header, min_len, (u8*)text_device, text_cap, res);
}

int
ntedit_hip_reads_bam_model(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, char* out, uint64_t cap,
                           ntedit_hip_reads_bam_result* res)
{
	return ntedit_hip_reads_bam_model_q(raw, n_raw, at_header, min_len, 0, out, cap, res);
}

int
ntedit_hip_reads_bam_model_q(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, uint32_t min_qual, char* out, uint64_t cap,
                             ntedit_hip_reads_bam_result* res)
{
	if (!res || (n_raw && !raw) || (cap && !out) || min_qual > nte_parse::RP_MAX_MIN_QUAL) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_bam_model: bad argument");
	}
	return ntedit_hip_reads_bam_model_f(raw, n_raw, at_header, min_len, min_qual, 0, 0, 0.0f, out, cap, res, nullptr);
}

int
ntedit_hip_reads_bam_model_f(const void* raw, uint64_t n_raw, int at_header, uint32_t min_len, uint32_t min_qual, uint32_t min_read_len,
                             uint32_t min_mean_qual, float min_rq, char* out, uint64_t cap, ntedit_hip_reads_bam_result* res,
                             ntedit_hip_reads_read_filter_stats* st)
{
	nte_parse::ReadFilter f = nte_parse::ReadFilter();
	if (!res || (n_raw && !raw) || (cap && !out) || min_qual > nte_parse::RP_MAX_MIN_QUAL ||
	    !nte_parse::rp_make_filter(min_read_len, min_mean_qual, min_rq, &f)) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_bam_model: bad argument");
	}
	BamResult r;
	nte_parse::ReadFilterCounts fc = nte_parse::ReadFilterCounts();
	bam_model_f((const u8*)raw, n_raw, at_header, min_len, min_qual, f, out, cap, &r, nullptr, &fc);
	to_result(r, res);
	if (st) {
		memcpy(st, &fc, sizeof fc);
	}
	if (r.clean && r.text_len > cap) {
		return pfail(nullptr, NTEDIT_E_OVERFLOW, "reads_bam_model: the text does not fit the buffer");
	}
	return 0;
}

} // extern "C"
