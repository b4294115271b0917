// nte_track.hip -- the unsupported regions of a batch as intervals, from an absent bitmap and the batch's entries
// (nte_track.h has the definition and the stages).
#include "nte_track.h"
#include "nte_tile.h" // (entry_behind, bit_range)

namespace nte {

namespace {

// where entry e's k-mer starts end (its own begin: it has none)
__device__ __forceinline__ u64
starts_end(const TrackArgs& a, u32 e)
{
	return a.lens[e] >= a.k ? a.offs[e] + a.lens[e] - a.k + 1 : a.offs[e];
}

// the start range of entry e inside the word at p0, as a mask
__device__ __forceinline__ u64
starts_mask(const TrackArgs& a, u32 e, u64 p0)
{
	const u64 s0 = a.offs[e], s1 = starts_end(a, e);
	if (s1 <= p0 || s1 <= s0) {
		return 0;
	}
	return bit_range(s0 > p0 ? (u32)(s0 - p0) : 0, s1 - p0 < 64 ? (u32)(s1 - p0) : 64);
}

// The tile's masked words in LDS, `halo` words in front and behind: s_m[i] is word first_word + i of the batch, zero
// where the batch has none.
struct Tile
{
	const u64* s_m;
	long long first_word;

	// a marked start among the positions [lo, hi)?  (within the halo: lo, hi at most k + 1 from a position of the tile)
	__device__ __forceinline__ bool any(u64 lo, u64 hi) const
	{
		if (hi <= lo) {
			return false;
		}
		const long long w0 = (long long)(lo / 64), w1 = (long long)((hi - 1) / 64);
		for (long long w = w0; w <= w1; w++) {
			const u32 b0 = w == w0 ? (u32)(lo % 64) : 0;
			const u32 b1 = w == w1 ? (u32)((hi - 1) % 64) + 1 : 64;
			if (s_m[w - first_word] & bit_range(b0, b1)) {
				return true;
			}
		}
		return false;
	}
};

// inclusive scan of v over the workgroup's TPB threads; *total = the sum (s_wave: TPB / 64 words)
template <u32 TPB>
__device__ __forceinline__ unsigned long long
block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long* total)
{
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (u32 o = 1; o < 64; o <<= 1) {
		const unsigned long long t = __shfl_up(v, o);
		if (lane >= o) {
			v += t;
		}
	}
	__syncthreads(); // (s_wave may still be read from an earlier scan)
	if (lane == 63) {
		s_wave[wave] = v;
	}
	__syncthreads();
	unsigned long long before = 0, all = 0;
	for (u32 q = 0; q < TPB / 64; q++) {
		const unsigned long long t = s_wave[q];
		before += q < wave ? t : 0;
		all += t;
	}
	*total = all;
	return v + before;
}

// One workgroup per tile of TRACK_TILE positions, one bitmap word per thread, whatever entries the tile holds.  Phase 1:
// the words of the tile and of the halo, each masked with the start ranges of the entries it touches, go to LDS.  Phase 2:
// every thread classifies the marked starts of its word, entry by entry: a start begins an interval iff none of its
// entry's starts is marked in the k positions in front of it, and ends one iff none is in the k positions behind it.
// Inside the word that is the distance to the neighbouring bit; for the first and the last bit of an entry in the word
// the words in LDS answer, never further than the entry's own first and last start -- so nothing is taken from another
// entry, however close.  COUNT: the tile's three counts.  EMIT: the counts of the tiles in front (k_track_scan) plus an
// exclusive scan over the workgroup give every start and every end its index; the two halves of a record are written by
// whoever owns them (an interval can span many tiles), and nobody reads the other half here.
template <bool EMIT>
__global__ __launch_bounds__(TRACK_TPB) void
k_track_tile(TrackArgs a, TrackTile* tiles, TrackInterval* recs, u32* upto, u64 n_recs)
{
	__shared__ u64 s_m[TRACK_TPB + 2 * TRACK_MAX_HALO];
	__shared__ unsigned long long s_wave[TRACK_TPB / 64];
	const u32 halo = (a.k + 63) / 64 + 1;
	const u64 n_words = (a.n + 63) / 64;
	const long long first_word = (long long)blockIdx.x * TRACK_TPB - (long long)halo;
	for (u32 i = threadIdx.x; i < TRACK_TPB + 2 * halo; i += TRACK_TPB) {
		const long long gw = first_word + i;
		u64 m = 0;
		if (gw >= 0 && (u64)gw < n_words) {
			const u64 bits = a.bitmap[gw];
			if (bits) {
				const u64 p0 = (u64)gw * 64;
				u64 mask = 0;
				for (u32 e = entry_behind(a.offs, a.lens, a.n_entries, p0); e < a.n_entries && a.offs[e] < p0 + 64; e++) {
					mask |= starts_mask(a, e, p0);
				}
				m = bits & mask;
			}
		}
		s_m[i] = m;
	}
	__syncthreads();
	const Tile tile = { s_m, first_word };
	const u64 p0 = ((u64)blockIdx.x * TRACK_TPB + threadIdx.x) * 64;
	const u64 own = s_m[halo + threadIdx.x];
	u64 is_start = 0, is_end = 0;
	if (own) {
		for (u32 e = entry_behind(a.offs, a.lens, a.n_entries, p0); e < a.n_entries && a.offs[e] < p0 + 64; e++) {
			u64 rest = own & starts_mask(a, e, p0);
			const u64 s0 = a.offs[e], s1 = starts_end(a, e);
			int prev = -1;
			while (rest) {
				const int b = __builtin_ctzll(rest);
				rest &= rest - 1;
				const u64 p = p0 + (u32)b;
				bool st, en;
				if (prev >= 0) {
					st = (u32)(b - prev) > a.k;
				} else {
					const u64 lo = p > a.k ? p - a.k : 0;
					st = !tile.any(lo > s0 ? lo : s0, p);
				}
				if (rest) {
					en = (u32)(__builtin_ctzll(rest) - b) > a.k;
				} else {
					const u64 hi = p + a.k + 1;
					en = !tile.any(p + 1, hi < s1 ? hi : s1);
				}
				is_start |= (u64)st << b;
				is_end |= (u64)en << b;
				prev = b;
			}
		}
	}
	// starts | ends << 20 | marks << 40: a tile has at most 2^14 of each
	const unsigned long long mine = (unsigned long long)__popcll(is_start) | (unsigned long long)__popcll(is_end) << 20 |
	                                (unsigned long long)__popcll(own) << 40;
	unsigned long long all = 0;
	const unsigned long long upto_me = block_scan<TRACK_TPB>(mine, s_wave, &all);
	if (!EMIT) {
		if (threadIdx.x == 0) {
			TrackTile t;
			t.starts = all & 0xFFFFF;
			t.ends = (all >> 20) & 0xFFFFF;
			t.marks = all >> 40;
			tiles[blockIdx.x] = t;
		}
		return;
	}
	if (!own) {
		return;
	}
	const unsigned long long before = upto_me - mine;
	const TrackTile t = tiles[blockIdx.x];
	const u64 base_s = t.starts + (before & 0xFFFFF), base_e = t.ends + ((before >> 20) & 0xFFFFF);
	const u64 base_m = t.marks + (before >> 40);
	for (u32 e = entry_behind(a.offs, a.lens, a.n_entries, p0); e < a.n_entries && a.offs[e] < p0 + 64; e++) {
		const u64 r = starts_mask(a, e, p0);
		const u64 s0 = a.offs[e];
		for (u64 ms = is_start & r; ms; ms &= ms - 1) {
			const u32 b = (u32)__builtin_ctzll(ms);
			const u64 below = (1ULL << b) - 1;
			const u64 i = base_s + (u64)__popcll(is_start & below);
			if (i < n_recs) {
				recs[i].entry = e;
				recs[i].begin = (u32)(p0 + b - s0);
				recs[i].absent = (u32)(base_m + (u64)__popcll(own & below)); // (the marked starts in front of it: k_track_finish)
			}
		}
		for (u64 me = is_end & r; me; me &= me - 1) {
			const u32 b = (u32)__builtin_ctzll(me);
			const u64 below = (1ULL << b) - 1;
			const u64 i = base_e + (u64)__popcll(is_end & below);
			if (i < n_recs) {
				recs[i].end = (u32)(p0 + b - s0 + a.k);
				upto[i] = (u32)(base_m + (u64)__popcll(own & below) + 1);
			}
		}
	}
}

// One workgroup: every thread sums a contiguous run of tiles, the sums are scanned over the workgroup, and the tiles get
// the counts of all tiles in front of them.  (183 k tiles at 3 Gbp: 179 per thread.)
__global__ __launch_bounds__(1024) void
k_track_scan(TrackTile* tiles, u64 n_tiles, u64* totals)
{
	__shared__ unsigned long long s_wave[1024 / 64];
	const u64 per = (n_tiles + 1023) / 1024;
	const u64 t0 = per * threadIdx.x < n_tiles ? per * threadIdx.x : n_tiles;
	const u64 t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
	unsigned long long sum[3] = { 0, 0, 0 };
	for (u64 t = t0; t < t1; t++) {
		sum[0] += tiles[t].starts;
		sum[1] += tiles[t].ends;
		sum[2] += tiles[t].marks;
	}
	unsigned long long run[3], all[3];
	for (u32 q = 0; q < 3; q++) {
		run[q] = block_scan<1024>(sum[q], s_wave, &all[q]) - sum[q];
	}
	for (u64 t = t0; t < t1; t++) {
		const TrackTile c = tiles[t];
		TrackTile o;
		o.starts = run[0];
		o.ends = run[1];
		o.marks = run[2];
		tiles[t] = o;
		run[0] += c.starts;
		run[1] += c.ends;
		run[2] += c.marks;
	}
	if (threadIdx.x == 0) {
		totals[0] = all[0];
		totals[1] = all[1];
		totals[2] = all[2];
		totals[3] = 0;
	}
}

// thread per record: absent = (marked starts up to its end) - (marked starts in front of its begin), exact modulo 2^32
// because no entry is longer than that; the covered bases: wavefront reduction, one atomic per wavefront
__global__ __launch_bounds__(256) void
k_track_finish(TrackInterval* recs, const u32* __restrict__ upto, u64 n_recs, u64* totals)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	unsigned long long covered = 0;
	if (i < n_recs) {
		TrackInterval r = recs[i];
		r.absent = upto[i] - r.absent;
		recs[i] = r;
		covered = r.end - r.begin;
	}
	for (int o = 32; o > 0; o >>= 1) {
		covered += __shfl_down(covered, o);
	}
	if ((threadIdx.x & 63) == 0 && covered) {
		atomicAdd(reinterpret_cast<unsigned long long*>(totals + 3), covered);
	}
}

} // namespace

void
launch_track_count(hipStream_t stream, const TrackArgs& a, TrackTile* tiles, u64* totals)
{
	const u64 n_tiles = track_tiles(a.n);
	if (n_tiles) {
		hipLaunchKernelGGL(k_track_tile<false>, dim3((unsigned)n_tiles), dim3(TRACK_TPB), 0, stream, a, tiles, (TrackInterval*)nullptr, (u32*)nullptr, (u64)0);
	}
	hipLaunchKernelGGL(k_track_scan, dim3(1), dim3(1024), 0, stream, tiles, n_tiles, totals);
}

void
launch_track_emit(hipStream_t stream, const TrackArgs& a, const TrackTile* tiles, TrackInterval* recs, u32* upto, u64 n_recs, u64* totals)
{
	const u64 n_tiles = track_tiles(a.n);
	if (n_tiles == 0 || n_recs == 0) {
		return;
	}
	hipLaunchKernelGGL(k_track_tile<true>, dim3((unsigned)n_tiles), dim3(TRACK_TPB), 0, stream, a, const_cast<TrackTile*>(tiles), recs, upto, n_recs);
	hipLaunchKernelGGL(k_track_finish, dim3((unsigned)((n_recs + 255) / 256)), dim3(256), 0, stream, recs, (const u32*)upto, n_recs, totals);
}

} // namespace nte
