// nte_apply.h -- the device applier and the k-mer QV counts (nte_apply.hip): what nte_api.hip launches.
//
// The applier restates host/render.cpp (render_contig + the FASTA part of write_contig) on the device: from the arena of
// rope items and the per-event first-chunk table it writes the edited contigs into one buffer in HBM, one separator byte
// behind each, plus a u64 offset and a u32 length per entry.  Stages (all on one stream):
//   k_apply_summary  thread per event: header, bounds, the event's nodes folded into an ApplyEvent; the contigs' event
//                    ranges from the headers' contig indices
//   k_apply_chain    wavefront per contig: 64 headers at a time, the serial-order filter (start >= cover) and the open
//                    node resolved in registers; per applied event its output offset and piece index inside the contig
//   k_apply_scan     one workgroup: 64-bit exclusive scans of the contigs' bytes and pieces
//   k_apply_pieces   thread per applied event + k_apply_tail thread per contig: the scanned piece table
//   k_apply_copy     workgroup per tile of APPLY_TILE output bytes: pieces by binary search, 16-byte accesses
//   k_apply_mods     thread per applied event: TAG_MOD items overwrite single output bytes
// k_qv_count counts, per entry of a batch, the k-mer starts whose k bytes are A, C, G or T (either case) and the set bits
// of an absent bitmap among the entry's starts.
#pragma once
#include "nte_common.h"

#include <hip/hip_runtime.h>

namespace nte {

constexpr u32 APPLY_TILE = 16384; // output bytes per workgroup of k_apply_copy
constexpr u32 APPLY_TPB = 256;
constexpr u32 APPLY_LDS_PIECES = 1024; // pieces of a tile kept in LDS (more: the searches go to global memory)
constexpr u32 QV_TPB = 256;
constexpr u32 QV_TILE = QV_TPB * 64; // positions per workgroup of k_qv_count: one bitmap word per thread
constexpr u32 QV_MAX_K = 1024;       // look-ahead words of a tile held in LDS

// status bits (the renderer's return codes: host/render.cpp)
enum ApplyStatus : u32
{
	AP_BAD_INDEX = 1,   // -1: a chunk index outside the arena (or a chain longer than the arena)
	AP_BAD_ORDER = 2,   // -2: a header names a contig the batch does not have
	AP_BAD_COUNT = 4,   // -3: a chunk with more than CHUNK_ITEMS items
	AP_BAD_ITEM = 8,    // -4: an unknown item tag, a node outside its contig
	AP_UNFINISHED = 16, // -6: a parked event among the applied ones
	AP_TOO_LONG = 32    // an edited contig of 4 GiB or more
};

struct ApplyEvent // what an event's chain says, whatever is applied in front of it
{
	u32 start, cover_end, hflags;
	u32 contig;  // NONE32: no output
	u32 n_nodes; // up to and including a node of type -1
	u32 first;   // type | c << 8 of its first node
	u32 first_s, first_e;
	u32 last; // the same of its last node
	u32 last_s, last_e;
	u32 mid_len; // bytes of the nodes between the two
};

struct ApplyPlace // an event in the serial order of its contig
{
	u32 out_off; // where its first node's bytes begin, from the contig's first output byte
	u32 piece;   // index of that node's piece, from the contig's first piece
	u32 open_s;  // s_pos of the open node it replaces
	u32 flags;   // 1 applied, 2 its nodes count (the rope was not terminated in front of it)
};

struct ApplyContig
{
	u64 out_len;
	u32 n_pieces; // the open node's piece and the separator's included
	u32 open;     // type | c << 8 of the node that ends the rope
	u32 open_s, open_e;
	u32 open_off;
	u32 applied;
};

// src: an offset into the batch, or APPLY_LIT | key << 8 | byte for a single byte (key: the batch offset the rope stood
// at, so that the pieces of a contig stay ordered by draft position for k_apply_mods); a piece's length is the distance
// to the next piece's out_off
struct ApplyPiece
{
	u64 out_off;
	u64 src;
};
constexpr u64 APPLY_LIT = 1ULL << 63;

struct ApplyArgs
{
	const u8* seq;
	u64 n_seq;
	const u64* offs;
	const u32* lens;
	u32 n_contigs;
	const Item* arena;
	u64 arena_items;
	const u32* ev_first;
	u32 n_events;
	ApplyEvent* ev;
	ApplyPlace* place;
	u32* ev_begin; // per contig (set to NONE32 / 0 before k_apply_summary)
	u32* ev_end;
	ApplyContig* contig;
	u64* out_offs;   // per contig
	u32* out_lens;
	u64* piece_base; // n_contigs + 1
	u64* totals;     // [0] bytes, [1] pieces, [2] applied events
	u32* status;
	ApplyPiece* pieces;
	u8* out;
};

struct QvRow // = ntedit_hip_qv_row
{
	u64 len_before, len_after, kmers_before, absent_before, kmers_after, absent_after;
};

void launch_apply_plan(hipStream_t stream, const ApplyArgs& a);  // summary, chain, scan: totals and status are ready
void launch_apply_write(hipStream_t stream, const ApplyArgs& a, u64 total_bytes, u64 total_pieces); // pieces, copy, mods
void launch_qv_rows(hipStream_t stream, QvRow* rows, const u32* lens_before, const u32* lens_after, u32 n);
// which: 0 = kmers_before / absent_before, 1 = kmers_after / absent_after
void launch_qv_count(hipStream_t stream, const u8* seq, u64 n, const u64* offs, const u32* lens, u32 n_entries, const u64* bitmap, u32 k,
                     QvRow* rows, int which);

} // namespace nte
