// nte_reads_parse.hip -- gfx950 kernels and C ABI of --gpu_parse: raw FASTA / FASTQ bytes in HBM to the batch text the
// host parser (reads_pass.cpp) hands the reads kernels -- every read of k bases or more followed by '\n', in file order.
// The grammar (line class, clean predicate, kept rule) is nte_reads_grammar.h; a chunk that breaks it is reported
// unclean and left to the host parser.  ntedit_hip_reads_parse_model is the serial host model of the same functions
// (rp_model of nte_reads_model.h).
//
// Phases, ordered by kernel boundaries on one stream (no hand-off between workgroups inside a launch):
//   k_rp_tiles       per tile of 16 KiB (16-byte loads per lane): its number of '\n', and whether it holds a '\r'
//   scan             tile counts -> the line index at each tile start; their total is read back (the one host sync
//                    in the middle: it sizes the later grids, and a chunk over the line table's bound stops here)
//   k_rp_line_ends   the tiles again: a '\n' at p with line index L = tile base + rank in the tile -> line_end[L] = p
//   k_rp_classify    one lane per line: class and grammar checks (violations OR into one status word), and per line
//                    (record heads, sequence bytes) packed in 64 bits
//   scan             over the lines: each line's record and its offset in the record's sequence
//   k_rp_qsum        (--min_mean_qual, FASTQ chunks) byte-parallel over the raw tiles: the quality weights of each quality
//                    line summed into a table indexed by line, one atomic per (wavefront, line)
//   k_rp_heads / k_rp_records   each record's head line and length; kept records emit (1, length + 1).  k_rp_records<true>
//                    (--min_read_len, --min_mean_qual) keeps by rp_record_reason and counts the drops per rule
//   scan             over the records: each kept record's offset in the text
//   k_rp_line_out    each sequence line's offset in the text, and the '\n' behind each kept record
//   k_rp_copy        byte-parallel over the raw tiles: each lane finds the line of its 16 bytes from the tile base and
//                    the newline ranks, and writes them to that line's place (a line longer than a tile costs what
//                    its bytes cost).  k_rp_copy<true> (--min_qual, FASTQ chunks) also masks each base of a sequence
//                    line by the byte at the same offset of its quality line, two lines on
// The scans are count / scan / write over blocks of 2048 items (as k_count_starts / k_scan_counts / k_write_starts).
//
// Genome FASTA (nte_genome_grammar.h: chunks cut anywhere, entered in a state) shares the line table and the copy:
//   k_rp_tiles, scan, k_rp_line_ends   as above
//   k_gp_classify    one lane per line, line 0 by the entry state: class and grammar checks, the last header that
//                    begins in the chunk (an atomic max), and per line (headers begun, text bytes) packed in 64 bits
//   scan             over the lines: each line's place in the text
//   k_gp_line_out    the '\n' of each header that begins in the chunk, each sequence line's place, the exit state
//   k_rp_copy        as above
//
// Like nte_reads.hip this unit is outside KSRC and sees no context internals: its state hangs off the context pointer.
#include "nte_common.h"
#include "nte_reads_grammar.h"
#include "nte_reads_model.h"
#include "nte_genome_grammar.h"
#include "nte_reads_internal.h"
#include "nte_reads_unit.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

using namespace nte;
using namespace nte_parse;
using namespace nte_unit;

namespace {

constexpr int RP_TPB = 256;
constexpr int RP_TILE = 16384;
constexpr int RP_IT = RP_TILE / (RP_TPB * 16);
constexpr int SC_ITEMS = 8;
constexpr int SC_BLOCK = RP_TPB * SC_ITEMS;
constexpr u32 RP_NONE = 0xFFFFFFFFu; // line_out of a line that is not copied

static_assert(NTEDIT_PARSE_TILE == RP_TILE, "the header names the tile size");
static_assert(NTEDIT_PARSE_BAD_FIRST == RP_BAD_FIRST && NTEDIT_PARSE_BAD_CR == RP_BAD_CR && NTEDIT_PARSE_BAD_EMPTY == RP_BAD_EMPTY &&
                  NTEDIT_PARSE_BAD_SEQ_START == RP_BAD_SEQ_START && NTEDIT_PARSE_BAD_FQ_LINES == RP_BAD_FQ_LINES &&
                  NTEDIT_PARSE_BAD_FQ_HEADER == RP_BAD_FQ_HEADER && NTEDIT_PARSE_BAD_FQ_PLUS == RP_BAD_FQ_PLUS &&
                  NTEDIT_PARSE_BAD_FQ_QUAL == RP_BAD_FQ_QUAL && NTEDIT_PARSE_BAD_TABLE == RP_BAD_TABLE &&
                  NTEDIT_PARSE_BAD_SIZE == RP_BAD_SIZE,
              "the header names the grammar's rules");

struct RpInfo // the small result the device keeps per chunk
{
	u32 broken;
	u32 kind;
	u32 last_nl; // the chunk's last byte is '\n'
	u32 pad;
	u64 newlines;
	u64 records; // hi: kept records, lo: text bytes (a genome chunk: hi: headers begun)
	// genome chunks only
	u32 last_header1; // 1 + the raw offset of the last header line that begins in the chunk, 0: none
	u32 state_out;
	// --min_qual (k_rp_copy<true>): the bases copied that had a quality byte, and those of them masked
	u64 qual_bases, masked_bases;
	// --min_read_len, --min_mean_qual (k_rp_records<true>): the chunk's records and its drops per rule
	ReadFilterCounts filter;
};

__host__ __device__ __forceinline__ u32
lo32(u64 x)
{
	return (u32)x;
}

__host__ __device__ __forceinline__ u32
hi32(u64 x)
{
	return (u32)(x >> 32);
}

// the 16 raw bytes at `off` (a multiple of 16; raw is 16-byte aligned); bytes past n read as 0
__device__ __forceinline__ uint4
rp_load16(const u8* __restrict__ raw, u64 n, u64 off)
{
	if (off + 16 <= n) {
		return *reinterpret_cast<const uint4*>(raw + off);
	}
	u32 w[4] = { 0, 0, 0, 0 };
	for (int b = 0; b < 16; b++) {
		if (off + b < n) {
			w[b >> 2] |= (u32)raw[off + b] << (8 * (b & 3));
		}
	}
	return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit b set: byte b of the word equals ch (exact per byte: no carry crosses a byte)
__device__ __forceinline__ u32
rp_eq4(u32 w, u32 ch)
{
	const u32 x = w ^ (ch * 0x01010101u);
	const u32 t = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // 0x80 in every zero byte of x
	return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

__device__ __forceinline__ u32
rp_eq16(uint4 v, u32 ch)
{
	return rp_eq4(v.x, ch) | (rp_eq4(v.y, ch) << 4) | (rp_eq4(v.z, ch) << 8) | (rp_eq4(v.w, ch) << 12);
}

// bytes past n must not count as newlines: they read as 0, and '\n' != 0

// the newline masks of this lane's RP_IT pieces of the tile (piece j: bytes [j * 4096 + tid * 16, + 16) of the tile),
// and for each piece the number of newlines of the tile before it (byte order is (j, tid) order)
__device__ __forceinline__ void
rp_tile_ranks(const u8* __restrict__ raw, u64 n, u64 tile_off, u32 (&mask)[RP_IT], u32 (&before)[RP_IT], uint4 (&bytes)[RP_IT])
{
	__shared__ u32 s_seg[RP_IT * (RP_TPB / 64)];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	u32 in_wave[RP_IT];
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		bytes[j] = rp_load16(raw, n, tile_off + (u64)j * (RP_TPB * 16) + tid * 16);
		mask[j] = rp_eq16(bytes[j], '\n');
		const u32 c = __popc(mask[j]);
		u32 incl = c;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const u32 up = __shfl_up(incl, d, 64);
			if (lane >= (u32)d) {
				incl += up;
			}
		}
		in_wave[j] = incl - c;
		if (lane == 63) {
			s_seg[j * (RP_TPB / 64) + wave] = incl;
		}
	}
	__syncthreads();
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		u32 base = 0;
		const u32 me = j * (RP_TPB / 64) + wave;
		for (u32 q = 0; q < me; q++) {
			base += s_seg[q];
		}
		before[j] = base + in_wave[j];
	}
}

__global__ __launch_bounds__(RP_TPB) void
k_rp_tiles(const u8* __restrict__ raw, u64 n, u64* __restrict__ tile_nl, RpInfo* info)
{
	__shared__ u32 s_cnt;
	const u32 tid = threadIdx.x;
	if (tid == 0) {
		s_cnt = 0;
	}
	__syncthreads();
	const u64 tile_off = (u64)blockIdx.x * RP_TILE;
	u32 cnt = 0, cr = 0;
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		const uint4 v = rp_load16(raw, n, tile_off + (u64)j * (RP_TPB * 16) + tid * 16);
		cnt += __popc(rp_eq16(v, '\n'));
		cr |= rp_eq16(v, '\r');
	}
	if (cnt) {
		atomicAdd(&s_cnt, cnt);
	}
	if (cr) {
		atomicOr(&info->broken, (u32)RP_BAD_CR);
	}
	__syncthreads();
	if (tid == 0) {
		tile_nl[blockIdx.x] = s_cnt;
		if (blockIdx.x == 0) {
			info->kind = raw[0];
			info->last_nl = raw[n - 1] == '\n';
		}
	}
}

// ------------------------------------------------------------------ exclusive scan of 64-bit items
__device__ __forceinline__ u64
block_excl_scan(u64 v, u64* total)
{
	__shared__ u64 s_wave[RP_TPB / 64];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	u64 incl = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const u32 up_lo = __shfl_up((u32)incl, d, 64), up_hi = __shfl_up((u32)(incl >> 32), d, 64);
		if (lane >= (u32)d) {
			incl += ((u64)up_hi << 32) | up_lo;
		}
	}
	__syncthreads(); // (a caller's loop may still be reading s_wave of the round before)
	if (lane == 63) {
		s_wave[wave] = incl;
	}
	__syncthreads();
	u64 base = 0, all = 0;
#pragma unroll
	for (u32 w = 0; w < RP_TPB / 64; w++) {
		base += w < wave ? s_wave[w] : 0;
		all += s_wave[w];
	}
	*total = all;
	return base + incl - v;
}

__global__ __launch_bounds__(RP_TPB) void
k_scan_sums(const u64* __restrict__ in, u64 n, u64* __restrict__ bsum)
{
	const u64 at = (u64)blockIdx.x * SC_BLOCK + (u64)threadIdx.x * SC_ITEMS;
	u64 t = 0;
#pragma unroll
	for (int i = 0; i < SC_ITEMS; i++) {
		t += at + i < n ? in[at + i] : 0;
	}
	u64 total;
	(void)block_excl_scan(t, &total);
	if (threadIdx.x == 0) {
		bsum[blockIdx.x] = total;
	}
}

// one workgroup: bsum[0 .. nb) to its exclusive scan in place, the grand total to *total
__global__ __launch_bounds__(RP_TPB) void
k_scan_top(u64* __restrict__ bsum, u64 nb, u64* __restrict__ total)
{
	u64 carry = 0;
	for (u64 base = 0; base < nb; base += RP_TPB) {
		const u64 i = base + threadIdx.x;
		const u64 v = i < nb ? bsum[i] : 0;
		u64 all;
		const u64 ex = block_excl_scan(v, &all);
		if (i < nb) {
			bsum[i] = carry + ex;
		}
		carry += all;
	}
	if (threadIdx.x == 0) {
		*total = carry;
	}
}

// out may be in
__global__ __launch_bounds__(RP_TPB) void
k_scan_write(const u64* in, u64 n, const u64* __restrict__ bsum, u64* out)
{
	const u64 at = (u64)blockIdx.x * SC_BLOCK + (u64)threadIdx.x * SC_ITEMS;
	u64 v[SC_ITEMS], t = 0;
#pragma unroll
	for (int i = 0; i < SC_ITEMS; i++) {
		v[i] = at + i < n ? in[at + i] : 0;
		t += v[i];
	}
	u64 total;
	u64 run = block_excl_scan(t, &total) + bsum[blockIdx.x];
#pragma unroll
	for (int i = 0; i < SC_ITEMS; i++) {
		if (at + i < n) {
			out[at + i] = run;
		}
		run += v[i];
	}
}

// ------------------------------------------------------------------ lines
__global__ __launch_bounds__(RP_TPB) void
k_rp_line_ends(const u8* __restrict__ raw, u64 n, const u64* __restrict__ tile_base, u32* __restrict__ line_end, u64 n_lines,
               const RpInfo* __restrict__ info)
{
	u32 mask[RP_IT], before[RP_IT];
	uint4 bytes[RP_IT];
	const u64 tile_off = (u64)blockIdx.x * RP_TILE;
	rp_tile_ranks(raw, n, tile_off, mask, before, bytes);
	const u64 base = tile_base[blockIdx.x];
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		const u64 off = tile_off + (u64)j * (RP_TPB * 16) + threadIdx.x * 16;
		u64 line = base + before[j];
		for (u32 m = mask[j]; m; m &= m - 1) {
			if (line < n_lines) {
				line_end[line] = (u32)(off + (u32)__ffs(m) - 1);
			}
			line++;
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0 && !info->last_nl) {
		line_end[n_lines - 1] = (u32)n; // the last line's virtual end
	}
}

__device__ __forceinline__ u32
rp_line_start(const u32* __restrict__ line_end, u64 line)
{
	return line ? line_end[line - 1] + 1 : 0;
}

// per line: its class, and (record heads << 32 | sequence bytes) for the scan
__global__ __launch_bounds__(RP_TPB) void
k_rp_classify(const u8* __restrict__ raw, u64 n, const u32* __restrict__ line_end, u64 n_lines, u8* __restrict__ cls,
              u64* __restrict__ val, RpInfo* info)
{
	const u64 line = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	if (line >= n_lines) {
		return;
	}
	const int kind = (int)info->kind;
	const u32 s = rp_line_start(line_end, line), e = line_end[line];
	const u32 len = e - s;
	u32 broken = line == 0 ? rp_chunk_broken(kind, n, n_lines) : 0;
	const int c = rp_line_class(kind, line, len ? (int)raw[s] : -1, &broken);
	if (kind == '@' && line % 4 == 3) {
		const u32 seq_len = line_end[line - 2] - rp_line_start(line_end, line - 2);
		broken |= rp_quality_broken(seq_len, len);
	}
	cls[line] = (u8)c;
	val[line] = c == RP_HEADER ? 1ull << 32 : c == RP_SEQ ? (u64)len : 0ull;
	if (broken) {
		atomicOr(&info->broken, broken);
	}
}

// sr[L]: hi = record heads before line L, lo = sequence bytes before it; sr[n_lines] = (records, sequence bytes)
__global__ __launch_bounds__(RP_TPB) void
k_rp_heads(const u8* __restrict__ cls, const u64* __restrict__ sr, u64 n_lines, u32* __restrict__ head_line)
{
	const u64 line = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	if (line < n_lines && cls[line] == RP_HEADER) {
		head_line[hi32(sr[line])] = (u32)line;
	}
	if (line == 0) {
		head_line[hi32(sr[n_lines])] = (u32)n_lines;
	}
}

// --min_mean_qual on a FASTQ chunk: qsum[L] += the quality weights (rp_qual_weight) of the bytes of every line L with
// L % 4 == 3, the table indexed by line so that a chunk not yet known clean cannot index out of it (qsum is zeroed per
// chunk and has n_lines entries).  Byte-parallel over the raw tiles like k_rp_copy: a lane holds 16 bytes and the line
// each lies in.  The sums are integers, so atomics give the same result in any order, but not one per byte: a lane sums
// its bytes per line in registers, the lanes of a wavefront that hold pieces of one line combine by a segmented scan
// keyed on the line (a lane's piece opens a segment where it holds a '\n'), and one atomicAdd per (wavefront, line)
// reaches memory -- from the lane that holds the line's '\n', or from lane 63 for the line that runs on.
__device__ __forceinline__ u64
rp_shfl_up64(u64 v, int d)
{
	const u32 lo = __shfl_up((u32)v, d, 64), hi = __shfl_up((u32)(v >> 32), d, 64);
	return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(RP_TPB) void
k_rp_qsum(const u8* __restrict__ raw, u64 n, const u64* __restrict__ tile_base, u64 n_lines, u64* __restrict__ qsum)
{
	__shared__ u32 s_weight[RP_MAX_QUAL + 1];
	if (threadIdx.x <= RP_MAX_QUAL) {
		s_weight[threadIdx.x] = RP_QUAL_WEIGHT[threadIdx.x];
	}
	u32 mask[RP_IT], before[RP_IT];
	uint4 bytes[RP_IT];
	const u64 tile_off = (u64)blockIdx.x * RP_TILE;
	rp_tile_ranks(raw, n, tile_off, mask, before, bytes); // (its barrier also publishes s_weight)
	const u64 base = tile_base[blockIdx.x];
	const u32 lane = threadIdx.x & 63;
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		const u64 off = tile_off + (u64)j * (RP_TPB * 16) + threadIdx.x * 16;
		const u32 w[4] = { bytes[j].x, bytes[j].y, bytes[j].z, bytes[j].w };
		const u32 m = mask[j];
		const u64 line0 = base + before[j]; // the line of this lane's first byte
		u64 line = line0;
		u64 head = 0, run = 0; // the sum up to the first '\n' (the line that came in), and of the line being walked
		bool closed = false;   // a '\n' seen: `head` is final
#pragma unroll
		for (int b = 0; b < 16; b++) {
			if ((m >> b) & 1u) { // (bytes past n read as 0: no '\n' among them)
				if (!closed) {
					head = run;
					closed = true;
				} else if (run && line < n_lines) { // a line that lies wholly in these 16 bytes
					atomicAdd((unsigned long long*)&qsum[line], (unsigned long long)run);
				}
				run = 0;
				line++;
			} else if ((line & 3) == 3 && off + b < n) {
				run += s_weight[rp_qual_index((int)((w[b >> 2] >> (8 * (b & 3))) & 0xFFu) - RP_QUAL_OFFSET)];
			}
		}
		// `run` now belongs to the line that leaves the lane.  Inclusive segmented scan of it over the lanes: a lane with
		// a '\n' opens a segment (what came before belongs to other lines)
		u64 acc = run;
		bool opened = closed;
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const u64 up = rp_shfl_up64(acc, d);
			const bool up_opened = __shfl_up((int)opened, d, 64) != 0;
			if (lane >= (u32)d) {
				if (!opened) {
					acc += up;
				}
				opened = opened || up_opened;
			}
		}
		// the line that came into a lane with a '\n' ends there: what the lanes before hold of it, and this lane's head
		const u64 before_me = rp_shfl_up64(acc, 1);
		if (closed) {
			const u64 total = head + (lane ? before_me : 0);
			if (total && line0 < n_lines) {
				atomicAdd((unsigned long long*)&qsum[line0], (unsigned long long)total);
			}
		}
		if (lane == 63 && acc && line < n_lines) { // the line that runs on behind the wavefront's bytes
			atomicAdd((unsigned long long*)&qsum[line], (unsigned long long)acc);
		}
	}
}

// per record r: (1 << 32 | length + 1) when it is kept, else 0 (and 0 for r at or past the number of records).
// FILTER (--min_read_len, --min_mean_qual): the rule is rp_record_reason, k the shortest record kept without the options;
// a FASTQ record's weights are qsum[head_line[r] + 3], read only when that line is in the table (qsum: NULL without
// --min_mean_qual and for a FASTA chunk).  The records and the drops per rule are summed per wavefront and added to info
// by one atomic each per wavefront.
template <bool FILTER>
__global__ __launch_bounds__(RP_TPB) void
k_rp_records(const u64* __restrict__ sr, const u32* __restrict__ head_line, u64 n_lines, u32 k, u64* __restrict__ rec, ReadFilter f,
             const u64* __restrict__ qsum, RpInfo* info)
{
	const u64 r = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	u32 seen = 0, by_len = 0, by_mq = 0;
	if (r < n_lines) {
		u64 v = 0;
		if (r < hi32(sr[n_lines])) {
			const u32 len = lo32(sr[head_line[r + 1]]) - lo32(sr[head_line[r]]);
			bool keep;
			if (FILTER) {
				const u64 qline = (u64)head_line[r] + 3;
				const bool has_qual = qsum != nullptr && qline < n_lines;
				const u32 why = rp_record_reason(len, k, f, has_qual, has_qual ? qsum[qline] : 0);
				seen = 1;
				by_len = why == RP_DROP_LENGTH;
				by_mq = why == RP_DROP_MEAN_QUAL;
				keep = why == RP_KEPT;
			} else {
				keep = rp_record_kept(len, k);
			}
			if (keep) {
				v = (1ull << 32) | ((u64)len + 1);
			}
		}
		rec[r] = v;
	}
	if (FILTER) {
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			seen += __shfl_xor(seen, d, 64);
			by_len += __shfl_xor(by_len, d, 64);
			by_mq += __shfl_xor(by_mq, d, 64);
		}
		if ((threadIdx.x & 63) == 0 && seen) {
			atomicAdd((unsigned long long*)&info->filter.records, (unsigned long long)seen);
			atomicAdd((unsigned long long*)&info->filter.by_length, (unsigned long long)by_len);
			atomicAdd((unsigned long long*)&info->filter.by_mean_qual, (unsigned long long)by_mq);
		}
	}
}

// rec[r]: hi = kept records before r, lo = their text bytes: record r's place.  Each sequence line's place, the '\n'
// behind each kept record, and the chunk's totals.
__global__ __launch_bounds__(RP_TPB) void
k_rp_line_out(const u8* __restrict__ cls, const u64* __restrict__ sr, const u32* __restrict__ head_line, const u64* __restrict__ rec,
              u64 n_lines, u32* __restrict__ line_out, u8* __restrict__ text, u64 text_cap, RpInfo* info)
{
	const u64 line = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	if (line >= n_lines) {
		return;
	}
	if (line == 0) {
		info->records = rec[n_lines];
	}
	const u32 c = cls[line];
	u32 out = RP_NONE;
	if (c == RP_SEQ && hi32(sr[line]) > 0) {
		const u32 r = hi32(sr[line]) - 1;
		if (rec[r + 1] != rec[r]) {
			out = lo32(rec[r]) + (lo32(sr[line]) - lo32(sr[head_line[r]]));
		}
	} else if (c == RP_HEADER) {
		const u32 r = hi32(sr[line]);
		if (rec[r + 1] != rec[r]) {
			const u64 at = (u64)lo32(rec[r + 1]) - 1;
			if (at < text_cap) {
				text[at] = '\n';
			}
		}
	}
	line_out[line] = out;
}

// MASK (--min_qual on a FASTQ chunk): a byte at offset j of sequence line L (L % 4 == 1, copied) is masked by the byte at
// offset j of line L + 2 (rp_mask_base).  The copy is queued before the chunk is known clean, so nothing the grammar
// promises is relied on for memory safety: line L + 2 has to be in the table and the quality address below n, else the
// base passes as it is.  The counts are summed per wavefront and added to info by one atomic each per wavefront.
template <bool MASK>
__global__ __launch_bounds__(RP_TPB) void
k_rp_copy(const u8* __restrict__ raw, u64 n, const u64* __restrict__ tile_base, const u32* __restrict__ line_end,
          const u32* __restrict__ line_out, u64 n_lines, u8* __restrict__ text, u64 text_cap, u32 min_qual, RpInfo* info)
{
	u32 n_qual = 0, n_masked = 0;
	u32 mask[RP_IT], before[RP_IT];
	uint4 bytes[RP_IT];
	const u64 tile_off = (u64)blockIdx.x * RP_TILE;
	rp_tile_ranks(raw, n, tile_off, mask, before, bytes);
	const u64 base = tile_base[blockIdx.x];
#pragma unroll
	for (int j = 0; j < RP_IT; j++) {
		const u64 off = tile_off + (u64)j * (RP_TPB * 16) + threadIdx.x * 16;
		if (off >= n) {
			continue;
		}
		u64 line = base + before[j];
		if (line >= n_lines) {
			continue;
		}
		const u32 w[4] = { bytes[j].x, bytes[j].y, bytes[j].z, bytes[j].w };
		u32 out = line_out[line];
		// text position of raw byte p of this line: p + delta (32-bit wrap-around is exact: the result is in range)
		const u32 start = rp_line_start(line_end, line);
		u32 delta = out - start;
		// quality address of raw byte p of this line: p + qdelta (the quality line lies behind: no wrap-around)
		bool has_qual = false;
		u32 qdelta = 0;
		if (MASK && out != RP_NONE && (line & 3) == 1 && line + 2 < n_lines) {
			has_qual = true;
			qdelta = rp_line_start(line_end, line + 2) - start;
		}
		const u32 m = mask[j];
#pragma unroll
		for (int b = 0; b < 16; b++) {
			if (off + b >= n) {
				break;
			}
			if ((m >> b) & 1u) {
				line++;
				if (line >= n_lines) {
					break;
				}
				out = line_out[line];
				delta = out - (u32)(off + b + 1);
				if (MASK) {
					has_qual = out != RP_NONE && (line & 3) == 1 && line + 2 < n_lines;
					qdelta = has_qual ? rp_line_start(line_end, line + 2) - (u32)(off + b + 1) : 0;
				}
				continue;
			}
			if (out != RP_NONE) {
				const u32 at = (u32)(off + b) + delta;
				u8 ch = (u8)(w[b >> 2] >> (8 * (b & 3)));
				if (MASK && has_qual) {
					const u64 qa = off + b + (u64)qdelta;
					if (qa < n) {
						const int q = (int)raw[qa] - RP_QUAL_OFFSET;
						const bool low = rp_masked(q, min_qual);
						n_qual++;
						n_masked += low;
						ch = rp_mask_base(ch, low);
					}
				}
				if (at < text_cap) {
					text[at] = ch;
				}
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

// ------------------------------------------------------------------ genome chunks (nte_genome_grammar.h)
// per line: its class, and (headers begun << 32 | text bytes) for the scan
__global__ __launch_bounds__(RP_TPB) void
k_gp_classify(const u8* __restrict__ raw, u64 n, const u32* __restrict__ line_end, u64 n_lines, int state_in, int first_chunk,
              u8* __restrict__ cls, u64* __restrict__ val, RpInfo* info)
{
	const u64 line = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	if (line >= n_lines) {
		return;
	}
	const u32 s = rp_line_start(line_end, line), e = line_end[line];
	const u32 len = e - s;
	u32 broken = line == 0 ? gp_chunk_broken(first_chunk, (int)info->kind, n, n_lines) : 0;
	const int c = gp_line_class(state_in, line, len ? (int)raw[s] : -1, &broken);
	cls[line] = (u8)c;
	val[line] = gp_line_emit(c, len);
	if (c == RP_HEADER) {
		atomicMax(&info->last_header1, s + 1);
	}
	if (broken) {
		atomicOr(&info->broken, broken);
	}
}

// sr[L]: hi = headers begun before line L, lo = text bytes before it: line L's place; sr[n_lines] = the totals
__global__ __launch_bounds__(RP_TPB) void
k_gp_line_out(const u8* __restrict__ cls, const u64* __restrict__ sr, u64 n_lines, u32* __restrict__ line_out, u8* __restrict__ text,
              u64 text_cap, RpInfo* info)
{
	const u64 line = (u64)blockIdx.x * RP_TPB + threadIdx.x;
	if (line >= n_lines) {
		return;
	}
	const u32 c = cls[line];
	if (line == 0) {
		info->records = sr[n_lines];
	}
	if (line == n_lines - 1) {
		info->state_out = (u32)gp_state_out((int)info->last_nl, (int)c);
	}
	const u32 at = lo32(sr[line]);
	if (c == RP_HEADER && at < text_cap) {
		text[at] = '\n';
	}
	line_out[line] = c == RP_SEQ ? at : RP_NONE;
}

// ------------------------------------------------------------------ host side
// what the calls set and the last pass counted: survives ntedit_hip_sketch_free
struct ParseKeep
{
	int on = 0;                                    // ntedit_hip_reads_set_device_parse
	u32 min_qual = 0;                              // ntedit_hip_reads_set_min_qual (0: off)
	u64 qual_bases = 0, masked_bases = 0;          // ntedit_hip_reads_min_qual_info: the last pass, host parser and device
	ReadFilter filter = ReadFilter();              // ntedit_hip_reads_set_read_filter (all 0: off)
	ReadFilterCounts fcounts = ReadFilterCounts(); // ntedit_hip_reads_read_filter_info: the last pass, host parser and device
	ntedit_hip_reads_parse_stats info = {};
	ntedit_hip_genome_pass_info ginfo = {}; // ntedit_hip_genome_pass
};

enum { BUF_RAW0 = 0, BUF_RAW1 = 1, BUF_TEXT, BUF_GTEXT, N_BUFS, NO_BUF = -1 };

// device scratch, grow-only, released by ntedit_hip_sketch_free
struct ParseScratch
{
	int device = -1;
	hipStream_t stream = nullptr, copy_stream = nullptr;
	hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr }, copied[2] = { nullptr, nullptr };
	// the two raw buffers, the text, and a genome pass's text: GP_PAD bytes of carried text, then the chunk's (each is
	// allocated with RP_TILE bytes behind its cap)
	DevBuf buf[N_BUFS];
	u8* d_gstage = nullptr; // GP_PAD bytes
	u8* d_table = nullptr;  // the line table and the scans' block sums, for chunks of up to table_raw bytes
	u64 table_raw = 0;
	bool table_qsum = false; // the allocation has room for the quality sums (k_rp_qsum)
	RpInfo* d_info = nullptr;
	RpInfo* h_info = nullptr; // page-locked
};

typedef State<ParseKeep, ParseScratch> ParseState;
Registry<ParseState> g_parse;

void
release_scratch(ParseScratch* s)
{
	if (s->device < 0) {
		return;
	}
	(void)hipSetDevice(s->device);
	for (hipStream_t st : { s->stream, s->copy_stream }) {
		if (st) {
			(void)hipStreamSynchronize(st);
			(void)hipStreamDestroy(st);
		}
	}
	for (hipEvent_t e : { s->ev[0], s->ev[1], s->ev[2], s->ev[3], s->copied[0], s->copied[1] }) {
		if (e) {
			(void)hipEventDestroy(e);
		}
	}
	for (void* p : { (void*)s->buf[BUF_RAW0].p, (void*)s->buf[BUF_RAW1].p, (void*)s->buf[BUF_TEXT].p, (void*)s->d_table, (void*)s->d_info,
		                (void*)s->buf[BUF_GTEXT].p, (void*)s->d_gstage }) {
		if (p) {
			(void)hipFree(p);
		}
	}
	if (s->h_info) {
		(void)hipHostFree(s->h_info);
	}
	*s = ParseScratch();
}

int
ensure_device(const ntedit_hip_ctx* c, ParseScratch* s)
{
	if (s->device >= 0) {
		NTE_TRY(c, hipSetDevice(s->device));
		return 0;
	}
	int device = 0;
	NTE_TRY(c, hipGetDevice(&device));
	s->device = device;
	NTE_TRY(c, hipStreamCreate(&s->stream));
	NTE_TRY(c, hipStreamCreate(&s->copy_stream));
	for (hipEvent_t& e : s->ev) {
		NTE_TRY(c, hipEventCreate(&e));
	}
	for (hipEvent_t& e : s->copied) {
		NTE_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
	}
	NTE_TRY(c, hipMalloc((void**)&s->d_info, sizeof(RpInfo)));
	NTE_TRY(c, hipHostMalloc((void**)&s->h_info, sizeof(RpInfo), hipHostMallocDefault));
	return 0;
}

// this unit's buffers: a MiB of slack, a multiple of 16 (and RP_TILE bytes behind that, which cap does not count)
u64
buf_want(u64 need)
{
	return (need + (1u << 20)) / 16 * 16;
}

// the entry of every call: the context's state, its device and streams, and (but for NO_BUF) room for `need` bytes in a buffer
int
ready(const ntedit_hip_ctx* c, ParseState** state, int buf = NO_BUF, u64 need = 0)
{
	ParseState* s = *state = g_parse.find(c, true);
	int rc = ensure_device(c, &s->scr);
	if (rc == 0 && buf != NO_BUF) {
		rc = grow(c, s->scr.stream, &s->scr.buf[buf], need, buf_want(need), 0, RP_TILE);
	}
	return rc;
}

// the line table of a chunk of up to n raw bytes, carved from one allocation
struct Table
{
	u64 *tile, *sr, *rec, *bsum, *qsum;
	u32 *line_end, *head_line, *line_out;
	u8* cls;
	u64 bytes;
};

Table
carve(u8* base, u64 n_raw, bool with_qsum = false)
{
	const u64 tiles = (n_raw + RP_TILE - 1) / RP_TILE + 1, lines = rp_max_lines(n_raw) + 2;
	const u64 blocks = (lines > tiles ? lines : tiles) / SC_BLOCK + 2;
	Table t;
	Carver cut(base);
	t.tile = (u64*)cut.take(tiles * 8);
	t.sr = (u64*)cut.take(lines * 8);
	t.rec = (u64*)cut.take(lines * 8);
	t.bsum = (u64*)cut.take(blocks * 8);
	t.line_end = (u32*)cut.take(lines * 4);
	t.head_line = (u32*)cut.take(lines * 4);
	t.line_out = (u32*)cut.take(lines * 4);
	t.cls = cut.take(lines);
	t.qsum = with_qsum ? (u64*)cut.take(lines * 8) : nullptr; // (--min_mean_qual alone pays for k_rp_qsum's table: it lies last)
	t.bytes = cut.at;
	return t;
}

// data[0 .. n) to its exclusive scan in place, data[n] = the total
void
scan(ParseScratch* s, u64* data, u64 n, u64* bsum)
{
	const u64 nb = (n + SC_BLOCK - 1) / SC_BLOCK;
	hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(RP_TPB), 0, s->stream, data, n, bsum);
	hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(RP_TPB), 0, s->stream, bsum, nb, data + n);
	hipLaunchKernelGGL(k_scan_write, dim3((unsigned)nb), dim3(RP_TPB), 0, s->stream, data, n, bsum, data);
}

struct Lines
{
	Table t;
	u64 tiles, lines;
};

// The front phase of every chunk (n > 0 raw bytes): the line table, reallocated for `want` raw bytes (with_qsum: and the
// quality sums) unless it `fits` by the caller's rule; the info zeroed; the newlines per tile and their scan; the number of
// lines and the first words of the info read back (the one host sync in the middle).  *ms (when given) += the kernels' time.
int
line_table(const ntedit_hip_ctx* c, ParseScratch* s, const u8* d_raw, u64 n, bool fits, u64 want, bool with_qsum, double* ms, Lines* out)
{
	if (!fits || !s->d_table) {
		if (s->d_table) {
			NTE_TRY(c, hipStreamSynchronize(s->stream));
			NTE_TRY(c, hipFree(s->d_table));
			s->d_table = nullptr;
			s->table_raw = 0;
		}
		NTE_TRY(c, hipMalloc((void**)&s->d_table, carve(nullptr, want, with_qsum).bytes));
		s->table_raw = want;
		s->table_qsum = with_qsum;
	}
	const Table t = out->t = carve(s->d_table, s->table_raw, s->table_qsum);
	const u64 tiles = out->tiles = (n + RP_TILE - 1) / RP_TILE;
	NTE_TRY(c, hipMemsetAsync(s->d_info, 0, sizeof(RpInfo), s->stream));
	if (ms) {
		NTE_TRY(c, hipEventRecord(s->ev[0], s->stream));
	}
	hipLaunchKernelGGL(k_rp_tiles, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, s->d_info);
	scan(s, t.tile, tiles, t.bsum);
	NTE_TRY(c, hipGetLastError());
	if (ms) {
		NTE_TRY(c, hipEventRecord(s->ev[1], s->stream));
	}
	NTE_TRY(c, hipMemcpyAsync(&s->h_info->newlines, t.tile + tiles, 8, hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipMemcpyAsync(s->h_info, s->d_info, 16, hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	if (ms) {
		float front = 0;
		NTE_TRY(c, hipEventElapsedTime(&front, s->ev[0], s->ev[1]));
		*ms += front;
	}
	out->lines = s->h_info->newlines + (s->h_info->last_nl ? 0 : 1);
	return 0;
}

// the closing phase of a chunk whose later kernels were queued behind ev[2]: the chunk's info read back, *ms += their time
int
finish(const ntedit_hip_ctx* c, ParseScratch* s, double* ms)
{
	NTE_TRY(c, hipGetLastError());
	NTE_TRY(c, hipEventRecord(s->ev[3], s->stream));
	NTE_TRY(c, hipMemcpyAsync(s->h_info, s->d_info, sizeof(RpInfo), hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	float back = 0;
	NTE_TRY(c, hipEventElapsedTime(&back, s->ev[2], s->ev[3]));
	*ms += back;
	return 0;
}

int
parse_on_device(const ntedit_hip_ctx* c, ParseState* st, const u8* d_raw, u64 n, u32 k, u8* d_text, u64 text_cap,
                ntedit_hip_reads_parse_result* res)
{
	ParseKeep& keep = st->keep;
	ParseScratch* s = &st->scr;
	*res = ntedit_hip_reads_parse_result();
	if (n == 0) {
		res->clean = 1;
		return 0;
	}
	if (n >= RP_MAX_RAW) {
		res->broken = RP_BAD_SIZE;
		return 0;
	}
	// the table holds the chunk, and the quality sums when --min_mean_qual is on (they alone: the same size again)
	const bool need_qsum = keep.filter.min_mean_qual != 0;
	Lines l;
	int rc = line_table(c, s, d_raw, n, n <= s->table_raw && (!need_qsum || s->table_qsum), n > s->table_raw ? n + (1u << 20) : s->table_raw,
	                    need_qsum, &keep.info.ms_kernels, &l);
	if (rc) {
		return rc;
	}
	const Table& t = l.t;
	const u64 tiles = l.tiles, lines = l.lines;
	res->kind = (int)s->h_info->kind;
	res->lines = lines;
	// what is known by now ends the chunk here: over the table's bound nothing more may run
	res->broken = s->h_info->broken | rp_chunk_broken(res->kind, n, lines);
	if (res->broken) {
		return 0;
	}
	const unsigned line_blocks = (unsigned)((lines + RP_TPB - 1) / RP_TPB);
	NTE_TRY(c, hipEventRecord(s->ev[2], s->stream));
	hipLaunchKernelGGL(k_rp_line_ends, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, t.line_end, lines, s->d_info);
	hipLaunchKernelGGL(k_rp_classify, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, d_raw, n, t.line_end, lines, t.cls, t.sr, s->d_info);
	scan(s, t.sr, lines, t.bsum);
	hipLaunchKernelGGL(k_rp_heads, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, t.cls, t.sr, lines, t.head_line);
	if (rp_filter_on(keep.filter)) {
		// (rq is the BAM unit's; a FASTA chunk has no qualities: the length rule alone, and no sums)
		const bool sums = keep.filter.min_mean_qual && res->kind == '@';
		if (sums) {
			NTE_TRY(c, hipMemsetAsync(t.qsum, 0, lines * 8, s->stream));
			hipLaunchKernelGGL(k_rp_qsum, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, lines, t.qsum);
		}
		hipLaunchKernelGGL(k_rp_records<true>, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, t.sr, t.head_line, lines, k, t.rec, keep.filter,
		                   sums ? t.qsum : nullptr, s->d_info);
	} else {
		hipLaunchKernelGGL(k_rp_records<false>, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, t.sr, t.head_line, lines, k, t.rec,
		                   ReadFilter(), nullptr, s->d_info);
	}
	scan(s, t.rec, lines, t.bsum);
	hipLaunchKernelGGL(k_rp_line_out, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, t.cls, t.sr, t.head_line, t.rec, lines, t.line_out,
	                   d_text, text_cap, s->d_info);
	if (keep.min_qual && res->kind == '@') { // (a FASTA chunk has no qualities: the copy without the mask)
		hipLaunchKernelGGL(k_rp_copy<true>, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, t.line_end, t.line_out,
		                   lines, d_text, text_cap, keep.min_qual, s->d_info);
	} else {
		hipLaunchKernelGGL(k_rp_copy<false>, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, t.line_end, t.line_out,
		                   lines, d_text, text_cap, 0u, s->d_info);
	}
	if ((rc = finish(c, s, &keep.info.ms_kernels)) != 0) {
		return rc;
	}
	res->broken = s->h_info->broken;
	if (res->broken) {
		return 0;
	}
	keep.qual_bases += s->h_info->qual_bases; // (zero without --min_qual: the chunk's info is zeroed, and only the mask adds)
	keep.masked_bases += s->h_info->masked_bases;
	rp_counts_add(&keep.fcounts, s->h_info->filter); // (zero without a read filter, alike; by_rq and the aux counts are the BAM unit's: zero here)
	res->clean = 1;
	res->text_len = lo32(s->h_info->records);
	res->reads = hi32(s->h_info->records);
	res->bases = res->text_len - res->reads;
	return 0;
}

// one genome chunk of device bytes: the line table as parse_on_device builds it, then the genome phases
int
genome_on_device(const ntedit_hip_ctx* c, ParseState* st, const u8* d_raw, u64 n, int state_in, int first_chunk, u8* d_text, u64 text_cap,
                 ntedit_hip_genome_parse_result* res)
{
	ParseKeep& keep = st->keep;
	ParseScratch* s = &st->scr;
	*res = ntedit_hip_genome_parse_result();
	res->last_header = NTEDIT_READS_NO_START;
	res->state_out = state_in;
	if (n == 0) {
		res->clean = 1;
		return 0;
	}
	if (n >= RP_MAX_RAW) {
		res->broken = RP_BAD_SIZE;
		res->state_out = 0;
		return 0;
	}
	Lines l;
	int rc = line_table(c, s, d_raw, n, n + GP_TABLE_SLACK <= s->table_raw, n + 2 * GP_TABLE_SLACK, false, &keep.ginfo.ms_kernels,
	                    &l); // (the table holds what gp_stops lets through)
	if (rc) {
		return rc;
	}
	const Table& t = l.t;
	const u64 tiles = l.tiles, lines = l.lines;
	// over the table's bound nothing more may run
	if (gp_stops(n, lines)) {
		res->broken = gp_chunk_broken(0, 0, n, lines);
		res->lines = lines;
		res->state_out = 0;
		return 0;
	}
	const unsigned line_blocks = (unsigned)((lines + RP_TPB - 1) / RP_TPB);
	NTE_TRY(c, hipEventRecord(s->ev[2], s->stream));
	hipLaunchKernelGGL(k_rp_line_ends, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, t.line_end, lines, s->d_info);
	hipLaunchKernelGGL(k_gp_classify, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, d_raw, n, t.line_end, lines, state_in, first_chunk,
	                   t.cls, t.sr, s->d_info);
	scan(s, t.sr, lines, t.bsum);
	hipLaunchKernelGGL(k_gp_line_out, dim3(line_blocks), dim3(RP_TPB), 0, s->stream, t.cls, t.sr, lines, t.line_out, d_text, text_cap,
	                   s->d_info);
	hipLaunchKernelGGL(k_rp_copy<false>, dim3((unsigned)tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, t.tile, t.line_end, t.line_out,
	                   lines, d_text, text_cap, 0u, s->d_info); // (a genome is never masked)
	if ((rc = finish(c, s, &keep.ginfo.ms_kernels)) != 0) {
		return rc;
	}
	res->broken = s->h_info->broken;
	res->clean = res->broken == 0;
	res->state_out = (int)s->h_info->state_out;
	res->text_len = lo32(s->h_info->records);
	res->bases = res->text_len - hi32(s->h_info->records);
	res->lines = lines;
	res->last_header = s->h_info->last_header1 ? (u64)s->h_info->last_header1 - 1 : NTEDIT_READS_NO_START;
	return 0;
}

// raw as a *_parse_device call gives it: device bytes as they are, host bytes through raw buffer 0, copied on the stream
int
stage(const ntedit_hip_ctx* c, ParseState** state, const char* raw, u64 n_raw, int on_device, const u8** d_raw)
{
	const bool host = on_device == NTEDIT_HIP_BASES_HOST && n_raw;
	const int rc = ready(c, state, host ? BUF_RAW0 : NO_BUF, n_raw);
	if (rc) {
		return rc;
	}
	*d_raw = (const u8*)raw;
	if (host) {
		ParseScratch* s = &(*state)->scr;
		NTE_TRY(c, hipMemcpyAsync(s->buf[BUF_RAW0].p, raw, n_raw, hipMemcpyHostToDevice, s->stream));
		*d_raw = s->buf[BUF_RAW0].p;
	}
	return 0;
}

} // namespace

// what the other units and the pass loops need beyond the public calls (nte_reads_internal.h says what each does)
namespace nte_reads {

void
parse_release(const ntedit_hip_ctx* c)
{
	inflate_release(c);
	ParseState* s = g_parse.find(c, false);
	if (s) {
		release_scratch(&s->scr);
	}
}

int
parse_streams(const ntedit_hip_ctx* c, void** stream, void** copy_stream)
{
	ParseState* s;
	const int rc = ready(c, &s);
	if (rc == 0) {
		*stream = (void*)s->scr.stream;
		*copy_stream = (void*)s->scr.copy_stream;
	}
	return rc;
}

int
parse_lines(const ntedit_hip_ctx* c, const unsigned char* d_raw, uint64_t n, const uint32_t** line_end, uint64_t* n_lines,
            uint32_t* broken)
{
	ParseState* st;
	int rc = ready(c, &st);
	if (rc) {
		return rc;
	}
	ParseScratch* s = &st->scr;
	*line_end = nullptr;
	*n_lines = 0;
	*broken = n >= RP_MAX_RAW ? (uint32_t)RP_BAD_SIZE : 0u;
	if (n == 0 || *broken) {
		return 0;
	}
	// (no time is added: the caller's event pair has these kernels inside, inflate_last_start)
	Lines l;
	if ((rc = line_table(c, s, d_raw, n, n <= s->table_raw, n + (1u << 20), false, nullptr, &l)) != 0) {
		return rc;
	}
	if (l.lines > rp_max_lines(n)) {
		*broken = RP_BAD_TABLE;
		return 0;
	}
	hipLaunchKernelGGL(k_rp_line_ends, dim3((unsigned)l.tiles), dim3(RP_TPB), 0, s->stream, d_raw, n, l.t.tile, l.t.line_end, l.lines,
	                   s->d_info);
	NTE_TRY(c, hipGetLastError());
	*line_end = l.t.line_end;
	*n_lines = l.lines;
	return 0;
}

int
parse_buffer(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res)
{
	ParseState* s;
	const int rc = ready(c, &s, BUF_TEXT, n);
	if (rc) {
		return rc;
	}
	const DevBuf& t = s->scr.buf[BUF_TEXT];
	*text = (const char*)t.p;
	return parse_on_device(c, s, (const u8*)d_raw, n, k, t.p, t.cap, res);
}

int
parse_text_buffer(const ntedit_hip_ctx* c, uint64_t n, char** text, uint64_t* cap)
{
	ParseState* s;
	const int rc = ready(c, &s, BUF_TEXT, n);
	if (rc) {
		return rc;
	}
	*text = (char*)s->scr.buf[BUF_TEXT].p;
	*cap = s->scr.buf[BUF_TEXT].cap;
	return 0;
}

// ------------------------------------------------------------------ what genome_pass.cpp needs
constexpr u64 GP_PAD = 256; // genome_pad()

ntedit_hip_genome_pass_info*
genome_info(const ntedit_hip_ctx* c)
{
	return &g_parse.find(c, true)->keep.ginfo;
}

int
genome_pad(void)
{
	return (int)GP_PAD;
}

int
genome_begin_file(const ntedit_hip_ctx* c)
{
	ParseState* st;
	const int rc = ready(c, &st, BUF_GTEXT, GP_PAD);
	if (rc) {
		return rc;
	}
	ParseScratch* s = &st->scr;
	if (!s->d_gstage) {
		NTE_TRY(c, hipMalloc((void**)&s->d_gstage, GP_PAD));
	}
	NTE_TRY(c, hipMemsetAsync(s->buf[BUF_GTEXT].p, '\n', GP_PAD, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	return 0;
}

int
genome_raw_buffer(const ntedit_hip_ctx* c, int which, uint64_t n, char** d_raw)
{
	ParseState* s;
	const int rc = ready(c, &s, BUF_RAW0 + which, n);
	*d_raw = rc ? nullptr : (char*)s->scr.buf[BUF_RAW0 + which].p;
	return rc;
}

int
genome_parse_buffer(const ntedit_hip_ctx* c, int which, int copied, uint64_t n, int state_in, int first_chunk, const char** batch,
                    ntedit_hip_genome_parse_result* res)
{
	ParseState* st;
	int rc = ready(c, &st);
	if (rc) {
		return rc;
	}
	ParseScratch* s = &st->scr;
	DevBuf& gtext = s->buf[BUF_GTEXT];
	if (GP_PAD + n > gtext.cap || !gtext.p) {
		// (grow would free it: the pad moves to the new buffer with a synchronous copy, and the old one goes after it)
		u8* old = gtext.p;
		gtext = DevBuf();
		rc = grow(c, s->stream, &gtext, GP_PAD + n, buf_want(GP_PAD + n), 0, RP_TILE);
		if (rc == 0 && old) {
			NTE_TRY(c, hipMemcpy(gtext.p, old, GP_PAD, hipMemcpyDeviceToDevice));
		}
		if (old) {
			(void)hipFree(old);
		}
		if (rc) {
			return rc;
		}
	}
	if (copied) {
		NTE_TRY(c, hipEventSynchronize(s->copied[which]));
	}
	*batch = (const char*)gtext.p;
	return genome_on_device(c, st, s->buf[BUF_RAW0 + which].p, n, state_in, first_chunk, gtext.p + GP_PAD, gtext.cap - GP_PAD, res);
}

int
genome_carry(const ntedit_hip_ctx* c, uint64_t text_len, uint32_t keep)
{
	ParseState* st = g_parse.find(c, false);
	if (!st || !st->scr.buf[BUF_GTEXT].p || keep >= GP_PAD) {
		return pfail(c, NTEDIT_E_ARG, "genome_carry: bad argument");
	}
	ParseScratch* s = &st->scr;
	u8* d_gtext = s->buf[BUF_GTEXT].p;
	if (text_len) {
		NTE_TRY(c, hipMemcpyAsync(s->d_gstage, d_gtext + text_len, GP_PAD, hipMemcpyDeviceToDevice, s->stream));
		NTE_TRY(c, hipMemcpyAsync(d_gtext, s->d_gstage, GP_PAD, hipMemcpyDeviceToDevice, s->stream));
	}
	NTE_TRY(c, hipMemsetAsync(d_gtext, '\n', GP_PAD - keep, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	return 0;
}

} // namespace nte_reads

extern "C" {

int
ntedit_hip_genome_pass_get_info(ntedit_hip_ctx* c, ntedit_hip_genome_pass_info* info)
{
	if (!c || !info) {
		return c ? pfail(c, NTEDIT_E_ARG, "genome_pass_get_info: bad argument") : NTEDIT_E_ARG;
	}
	*info = g_parse.find(c, true)->keep.ginfo;
	return 0;
}

int
ntedit_hip_genome_parse_device(ntedit_hip_ctx* c, const char* raw, uint64_t n_raw, int on_device, int state_in, int first_chunk,
                               char* text_device, uint64_t text_cap, ntedit_hip_genome_parse_result* res)
{
	if (!c || !res || (n_raw && (!raw || !text_device)) || !gp_state_ok(state_in) ||
	    (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE)) {
		return c ? pfail(c, NTEDIT_E_ARG, "genome_parse_device: bad argument") : NTEDIT_E_ARG;
	}
	if (((uintptr_t)text_device & 15) || (on_device == NTEDIT_HIP_BASES_DEVICE && ((uintptr_t)raw & 15))) {
		return pfail(c, NTEDIT_E_ARG, "genome_parse_device: device buffers must be 16-byte aligned");
	}
	if (text_cap < n_raw) {
		return pfail(c, NTEDIT_E_ARG, "genome_parse_device: text_cap must be at least n_raw (the text is never longer than the raw bytes)");
	}
	ParseState* s;
	const u8* d_raw = nullptr;
	const int rc = stage(c, &s, raw, n_raw, on_device, &d_raw);
	if (rc) {
		return rc;
	}
	return genome_on_device(c, s, d_raw, n_raw, state_in, first_chunk != 0, (u8*)text_device, text_cap, res);
}

// the serial model (gp_model, nte_genome_grammar.h): the same grammar functions, one line after the other
int
ntedit_hip_genome_parse_model(const char* raw, uint64_t n_raw, int state_in, int first_chunk, char* out, uint64_t cap,
                              ntedit_hip_genome_parse_result* res)
{
	if (!res || (n_raw && !raw) || (cap && !out) || !gp_state_ok(state_in)) {
		return pfail(nullptr, NTEDIT_E_ARG, "genome_parse_model: bad argument");
	}
	GpResult m;
	const bool fits = gp_model(raw, n_raw, state_in, first_chunk, out, cap, &m);
	*res = ntedit_hip_genome_parse_result();
	res->clean = m.clean;
	res->broken = m.broken;
	res->state_out = m.state_out;
	res->text_len = m.text_len;
	res->bases = m.bases;
	res->lines = m.lines;
	res->last_header = m.last_header;
	return fits ? 0 : NTEDIT_E_OVERFLOW;
}

} // extern "C"

namespace nte_reads {

uint32_t
min_qual(const ntedit_hip_ctx* c)
{
	ParseState* s = g_parse.find(c, false);
	return s ? s->keep.min_qual : 0;
}

void
min_qual_count(const ntedit_hip_ctx* c, int reset, uint64_t qual_bases, uint64_t masked_bases)
{
	ParseKeep& keep = g_parse.find(c, true)->keep;
	if (reset) {
		keep.qual_bases = keep.masked_bases = 0;
	}
	keep.qual_bases += qual_bases;
	keep.masked_bases += masked_bases;
}

ReadFilter
read_filter(const ntedit_hip_ctx* c)
{
	ParseState* s = g_parse.find(c, false);
	return s ? s->keep.filter : ReadFilter();
}

void
read_filter_count(const ntedit_hip_ctx* c, int reset, const ReadFilterCounts* add)
{
	ParseKeep& keep = g_parse.find(c, true)->keep;
	if (reset) {
		keep.fcounts = ReadFilterCounts();
	}
	if (add) {
		rp_counts_add(&keep.fcounts, *add);
	}
}

int
parse_is_on(const ntedit_hip_ctx* c)
{
	ParseState* s = g_parse.find(c, false);
	return s ? s->keep.on : 0;
}

ntedit_hip_reads_parse_stats*
parse_info(const ntedit_hip_ctx* c)
{
	return &g_parse.find(c, true)->keep.info;
}

int
parse_copy_begin(const ntedit_hip_ctx* c, int which, const char* host, uint64_t n)
{
	ParseState* st;
	const int rc = ready(c, &st, BUF_RAW0 + which, n);
	if (rc) {
		return rc;
	}
	ParseScratch* s = &st->scr;
	if (n) {
		NTE_TRY(c, hipMemcpyAsync(s->buf[BUF_RAW0 + which].p, host, n, hipMemcpyHostToDevice, s->copy_stream));
	}
	NTE_TRY(c, hipEventRecord(s->copied[which], s->copy_stream));
	return 0;
}

int
parse_copy_wait(const ntedit_hip_ctx* c, int which)
{
	ParseState* s = g_parse.find(c, false);
	if (s && s->scr.copied[which]) {
		NTE_TRY(c, hipEventSynchronize(s->scr.copied[which]));
	}
	return 0;
}

int
parse_copied(const ntedit_hip_ctx* c, int which, uint64_t n, uint32_t k, const char** text, ntedit_hip_reads_parse_result* res)
{
	ParseState* s;
	const int rc = ready(c, &s, BUF_TEXT, n);
	if (rc) {
		return rc;
	}
	NTE_TRY(c, hipEventSynchronize(s->scr.copied[which]));
	const DevBuf& t = s->scr.buf[BUF_TEXT];
	*text = (const char*)t.p;
	return parse_on_device(c, s, s->scr.buf[BUF_RAW0 + which].p, n, k, t.p, t.cap, res);
}

} // namespace nte_reads

extern "C" {

int
ntedit_hip_reads_set_device_parse(ntedit_hip_ctx* c, int on)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	g_parse.find(c, true)->keep.on = on ? 1 : 0;
	return 0;
}

int
ntedit_hip_reads_set_min_qual(ntedit_hip_ctx* c, uint32_t q)
{
	if (!c || q > RP_MAX_MIN_QUAL) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_set_min_qual: the minimum base quality is 0 (off) or between 1 and 93") : NTEDIT_E_ARG;
	}
	g_parse.find(c, true)->keep.min_qual = q;
	return 0;
}

int
ntedit_hip_reads_min_qual_info(ntedit_hip_ctx* c, uint64_t* qual_bases, uint64_t* masked_bases)
{
	if (!c || !qual_bases || !masked_bases) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_min_qual_info: bad argument") : NTEDIT_E_ARG;
	}
	const ParseKeep& keep = g_parse.find(c, true)->keep;
	*qual_bases = keep.qual_bases;
	*masked_bases = keep.masked_bases;
	return 0;
}

int
ntedit_hip_reads_set_read_filter(ntedit_hip_ctx* c, uint32_t min_len, uint32_t min_mean_qual, float min_rq)
{
	ReadFilter f = ReadFilter();
	if (!c || !rp_make_filter(min_len, min_mean_qual, min_rq, &f)) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_set_read_filter: the minimum read length is 0 (off) or up to 2^31 - 1, the minimum mean "
		                                  "quality 0 (off) or between 1 and 60, the minimum rq 0 (off) or above 0 and at most 1")
		         : NTEDIT_E_ARG;
	}
	g_parse.find(c, true)->keep.filter = f;
	return 0;
}

int
ntedit_hip_reads_get_read_filter(ntedit_hip_ctx* c, uint32_t* min_len, uint32_t* min_mean_qual, float* min_rq)
{
	if (!c || !min_len || !min_mean_qual || !min_rq) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_get_read_filter: bad argument") : NTEDIT_E_ARG;
	}
	const ReadFilter f = g_parse.find(c, true)->keep.filter;
	*min_len = f.min_len;
	*min_mean_qual = f.min_mean_qual;
	memcpy(min_rq, &f.rq_bits, 4);
	return 0;
}

int
ntedit_hip_reads_read_filter_info(ntedit_hip_ctx* c, ntedit_hip_reads_read_filter_stats* st)
{
	if (!c || !st) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_read_filter_info: bad argument") : NTEDIT_E_ARG;
	}
	static_assert(sizeof(ntedit_hip_reads_read_filter_stats) == sizeof(ReadFilterCounts), "the counts are the grammar's, field for field");
	memcpy(st, &g_parse.find(c, true)->keep.fcounts, sizeof *st);
	return 0;
}

int
ntedit_hip_reads_parse_info(ntedit_hip_ctx* c, ntedit_hip_reads_parse_stats* st)
{
	if (!c || !st) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_parse_info: bad argument") : NTEDIT_E_ARG;
	}
	*st = g_parse.find(c, true)->keep.info;
	return 0;
}

int
ntedit_hip_reads_parse_device(ntedit_hip_ctx* c, const char* raw, uint64_t n_raw, int on_device, uint32_t k, char* text_device,
                              uint64_t text_cap, ntedit_hip_reads_parse_result* res)
{
	if (!c || !res || (n_raw && (!raw || !text_device)) || k == 0 ||
	    (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE)) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_parse_device: bad argument") : NTEDIT_E_ARG;
	}
	if (((uintptr_t)text_device & 15) || (on_device == NTEDIT_HIP_BASES_DEVICE && ((uintptr_t)raw & 15))) {
		return pfail(c, NTEDIT_E_ARG, "reads_parse_device: device buffers must be 16-byte aligned");
	}
	if (text_cap < n_raw) {
		return pfail(c, NTEDIT_E_ARG, "reads_parse_device: text_cap must be at least n_raw (the text is never longer than the raw bytes)");
	}
	ParseState* s;
	const u8* d_raw = nullptr;
	const int rc = stage(c, &s, raw, n_raw, on_device, &d_raw);
	if (rc) {
		return rc;
	}
	return parse_on_device(c, s, d_raw, n_raw, k, (u8*)text_device, text_cap, res);
}

int
ntedit_hip_reads_parse_model(const char* raw, uint64_t n_raw, uint32_t k, char* out, uint64_t cap, ntedit_hip_reads_parse_result* res)
{
	return ntedit_hip_reads_parse_model_q(raw, n_raw, k, 0, out, cap, res);
}

// the serial model (rp_model, nte_reads_model.h): the same grammar functions, one line after the other
int
ntedit_hip_reads_parse_model_q(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, char* out, uint64_t cap,
                               ntedit_hip_reads_parse_result* res)
{
	if (!res || (n_raw && !raw) || (cap && !out) || k == 0 || min_qual > RP_MAX_MIN_QUAL) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_parse_model: bad argument");
	}
	return ntedit_hip_reads_parse_model_f(raw, n_raw, k, min_qual, 0, 0, 0.0f, out, cap, res, nullptr);
}

int
ntedit_hip_reads_parse_model_f(const char* raw, uint64_t n_raw, uint32_t k, uint32_t min_qual, uint32_t min_len, uint32_t min_mean_qual,
                               float min_rq, char* out, uint64_t cap, ntedit_hip_reads_parse_result* res,
                               ntedit_hip_reads_read_filter_stats* st)
{
	ReadFilter f = ReadFilter();
	if (!res || (n_raw && !raw) || (cap && !out) || k == 0 || min_qual > RP_MAX_MIN_QUAL || !rp_make_filter(min_len, min_mean_qual, min_rq, &f)) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_parse_model: bad argument");
	}
	RpResult m;
	ReadFilterCounts fc = ReadFilterCounts();
	const bool fits = rp_model_f(raw, n_raw, k, min_qual, f, out, cap, &m, &fc);
	static_assert(sizeof(ntedit_hip_reads_parse_result) == sizeof(RpResult), "the result is the grammar's, field for field");
	memcpy(res, &m, sizeof m);
	if (st) {
		memcpy(st, &fc, sizeof fc);
	}
	return fits ? 0 : NTEDIT_E_OVERFLOW;
}

} // extern "C"
