// nte_track.h -- the unsupported regions of a batch as intervals (nte_track.hip): what nte_api.hip launches.
//
// Input: an absent bitmap (one bit per k-mer start, position p = bit p % 64 of word p / 64: what k_qv_count reads) and the
// entries of the batch.  A position is a marked start of entry e iff its bit is set and offs[e] <= p < offs[e] + lens[e] -
// k + 1 (k_qv_count's m_st).  An interval of e is a maximal sequence of its marked starts in which consecutive starts are at
// most k apart -- the k-mers' spans [p, p + k) overlap or are book-ended -- and never continues into another entry.  Its
// record: entry, begin = first start - offs[e], end = last start - offs[e] + k, absent = its marked starts.  Records are in
// batch order.  Stages (all on one stream):
//   k_track_tile<false>  workgroup per tile of TRACK_TILE positions, one bitmap word per thread: the tile's interval
//                        starts, interval ends and marked starts
//   k_track_scan         one workgroup: exclusive 64-bit prefixes of the tiles' three counts; the totals
//   k_track_tile<true>   the same pass again: the i-th start writes entry, begin and the marked starts in front of it into
//                        record i, the i-th end writes end and, into a side array, the marked starts up to it
//   k_track_finish       thread per record: absent from the two prefix counts; the covered bases summed
#pragma once
#include "nte_common.h"

#include <hip/hip_runtime.h>

namespace nte {

constexpr u32 TRACK_TPB = 256;
constexpr u32 TRACK_TILE = TRACK_TPB * 64; // positions per workgroup: one bitmap word per thread
constexpr u32 TRACK_MAX_K = 1024;                    // = QV_MAX_K (nte_apply.h)
constexpr u32 TRACK_MAX_HALO = TRACK_MAX_K / 64 + 1; // words of look-behind / look-ahead of a tile held in LDS

struct TrackInterval // = ntedit_hip_track_interval
{
	u32 entry, begin, end, absent;
};

struct TrackTile // a tile's counts; behind k_track_scan: the counts of all tiles in front of it
{
	u64 starts, ends, marks;
};

struct TrackArgs
{
	const u64* bitmap; // ceil(n / 64) words
	u64 n;             // positions
	const u64* offs;
	const u32* lens;
	u32 n_entries;
	u32 k; // 1 .. TRACK_MAX_K
};

inline u64
track_tiles(u64 n)
{
	return (n + TRACK_TILE - 1) / TRACK_TILE;
}

// tiles: track_tiles(a.n) elements; totals: [0] interval starts, [1] interval ends, [2] marked starts, [3] zeroed
void launch_track_count(hipStream_t stream, const TrackArgs& a, TrackTile* tiles, u64* totals);
// recs, upto: n_recs elements (= totals[0] = totals[1]); totals[3] += the covered bases
void launch_track_emit(hipStream_t stream, const TrackArgs& a, const TrackTile* tiles, TrackInterval* recs, u32* upto, u64 n_recs, u64* totals);

} // namespace nte
