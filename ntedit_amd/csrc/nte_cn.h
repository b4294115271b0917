// nte_cn.h -- the k-mer spectrum split by assembly copy number (nte_cn.hip): what nte_api.hip calls.
//
// F is the PRIMARY counting filter: h hashes, k, multiplicity m = min of a k-mer's h counters (k_spectrum's value).  A
// k-mer is k bytes of ACGTacgt inside one entry; entries may abut and may be shorter than k.  A SIDE is every batch that
// was appended to it (before: the batches as they came; after: their edited entries).  For one side:
//   the sketch S has `counters` 8-bit counters, a power of two; every k-mer occurrence of the side adds 1, saturating at
//   255, to its h counters S[hv_i & (counters - 1)] -- the filter's hash values, plain count-min, whatever the order;
//   cn(x) = min_i S[slot_i(x)], 1 .. 255 (255: "255 or more"), never below the true count; the class c = min(cn, 5);
//   occ[c][m]  the occurrences of class c with multiplicity m;
//   w5[m]      the sum of RECIP[cn] = (2^32 + cn / 2) / cn over the class-5 occurrences with multiplicity m;
//   a row per entry in the order the entries were appended: kmers and the five class counts of its occurrences.
// All of it is sums of integers: bit-for-bit independent of batching, order and launch geometry.
//
// The store keeps both sides' batches in device memory (the bytes, offs, lens) until the round ends: copy number is a
// property of the whole draft.  cn_append() only copies; cn_finish() runs, for each side in turn, the memset of the one
// sketch, k_cn_count over every stored batch, k_nonzero, k_spectrum_cn over every stored batch, then one copy to the host.
#pragma once
#include "nte_common.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

namespace nte {

constexpr int CN_CLASSES = 5;
constexpr int CN_BINS = 256;
constexpr int CN_ROW_WORDS = 6; // kmers, cn1, cn2, cn3, cn4, cn5plus
constexpr int CN_MAXK = 256;    // = TILE_MAXK (nte_tile.h: the tile's halo)
constexpr u64 CN_MIN_COUNTERS = 1ull << 20, CN_MAX_COUNTERS = 1ull << 36; // the default's range, and --cn_sketch's
constexpr u64 CN_FLOOR_COUNTERS = 1ull << 6; // what cn_finish takes (eight words for k_cn_nonzero): collisions on purpose
// one side's words on the device and in the host copy: occ[5][256] | w5[256] | nonzero counters | pad
constexpr size_t CN_SIDE_WORDS = (size_t)(CN_CLASSES + 1) * CN_BINS + 8;

// the states (= NTEDIT_CN_* of include/ntedit_hip.h)
constexpr int CN_OFF = 0, CN_ON = 1, CN_OVER_CAP = 2, CN_NO_MEMORY = 3;

struct CnBatch
{
	u8* bases = nullptr; // n bytes (the allocation is padded to whole 16 bytes)
	u64* offs = nullptr;
	u32* lens = nullptr;
	u64 n = 0;
	u32 n_entries = 0;
};

struct CnStore
{
	int state = CN_OFF;
	u64 cap = 0; // bytes of bases both sides may hold together
	std::vector<CnBatch> side[2];
	u64 bytes[2] = { 0, 0 }, entries[2] = { 0, 0 };
	// the results of the last cn_finish
	bool finished = false;
	u64 counters = 0;
	u64 nonzero[2] = { 0, 0 };
	float ms[4] = { 0.f, 0.f, 0.f, 0.f }; // k_cn_count before, k_spectrum_cn before, k_cn_count after, k_spectrum_cn after
	std::vector<u64> table[2];           // CN_SIDE_WORDS
	std::vector<u64> rows[2];            // entries x CN_ROW_WORDS
	// device memory of cn_finish: the sketch, the tables and rows; the events
	u8* sketch = nullptr;
	u64 sketch_bytes = 0;
	u64* d_out = nullptr;
	size_t d_out_words = 0;
	hipEvent_t evt[8] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
};

// the store begins (state ON, nothing held) or ends (OFF); both release what it holds
void cn_switch(CnStore& st, bool on, u64 cap_bytes);
// the batches go, the state returns to ON unless it is OFF (a new round: drop_filter, ntedit_hip_cn_reset)
void cn_reset(CnStore& st);
// everything goes, the events too (ntedit_hip_destroy, ntedit_hip_cn_free)
void cn_free(CnStore& st);
// one batch to side `which`: device copies of bases (host or device memory), offs, lens (host or device), queued on
// `stream`.  A batch that would pass the cap, or an allocation that fails, releases the whole store (OVER_CAP /
// NO_MEMORY) and is no error: 0.  A HIP error: its text in *why, NTEDIT_E_DEVICE.
int cn_append(CnStore& st, int which, hipStream_t stream, const void* bases, u64 n, const u64* offs, const u32* lens, u32 n_entries, std::string* why);
// the smallest power of two at or above 8 x the larger side's stored bytes, within [CN_MIN_COUNTERS, CN_MAX_COUNTERS]
u64 cn_default_counters(const CnStore& st);
// both sides from the store, against filter f (counting, device data) with the context's DevParams and seed tables; waits
// for `stream`.  0, or a code with its text in *why.
int cn_finish(CnStore& st, hipStream_t stream, const Filter& f, const DevParams& p, const u64* d_tab, u64 counters, std::string* why);

} // namespace nte
