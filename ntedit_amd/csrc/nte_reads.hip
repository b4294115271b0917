// nte_reads.hip -- gfx950 kernels and C ABI of the reads k-mer filter build (ntedit-make-reads-bf).
//
//   k_count<H, POW2>          pass 1: every k-mer of a batch of reads increments all h of its counters in a
//                             count-min sketch of 8-bit counters, saturating at 255
//   k_solid<H, POW2, COUNTS>  pass 2: est(x) = min of x's h sketch counters; a k-mer with est(x) >= cmin sets its h
//                             bits in a plain output filter, or raises its h counters of a counting output filter to
//                             est(x) (byte atomic max)
//   k_solid2<H, POW2>         pass 2 with a reject cutoff: one walk, one est(x); a k-mer with est(x) >= cmin sets its bits
//                             in the plain primary output, one with est(x) >= rmin also in the plain reject output (-e)
//   k_hist<H, POW2>           histogram pass: bin est(x) of a 256-bin histogram of every k-mer occurrence, summed in
//                             per-wave LDS sub-histograms and flushed once per block (one 64-bit add per non-zero bin)
//   k_pack                    after k_count, when the context keeps the reads resident: a batch packed into the store,
//                             per 16 bases one u32 of 2-bit codes and one u16 of validity bits (3 bits per base)
//   k_count / k_hist / k_solid / k_solid2 <.., PACKED = true>  the same passes staged from a stored batch instead of
//                             its bytes (pass 1 too: a later sketch, at another k, is counted from the store)
//   k_nonzero                 non-zero counters of the sketch (occupancy)
//   k_merge<OP>               n_src equal byte chunks folded into one: saturating add (sketches), OR (plain filters),
//                             max (counting filters) -- the merge of a sharded build
//
// k-mers, hashes and slots are the filter build's (k_screen<., ., true> in nte_kernels.hip): runs of k bytes of
// ACGTacgt, canonical base fh + rh, hash_extend, filter_slot.  Every result is independent of the order in which the
// atomics land: a counter ends at min(255, occurrences that hit it), a bit is an OR, a counting output is a max.
//
// gfx950 has no byte atomics: both byte updates are 32-bit compare-and-swap loops on the containing word, entered
// only when a plain read of the word says the byte still has to change (a saturated poly-A counter, a solid k-mer's
// bits already set, a counter already at est(x)).  Counters only grow, so a stale read can never skip an update that
// was due: it can only cost one extra CAS.
//
// This unit does not see the context's internals (nte_api.hip): the sketch lives in a small per-context state of its
// own, the output filter is reached through the public calls (ntedit_hip_filter_device_ptr / _info / _set_filter).
#include "nte_tile.h"
#include "nte_reads_internal.h"

#include "../host/bfio.h"
#include "../host/params.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

using namespace nte;

namespace {

// The tile (256 threads x 64 consecutive k-mer starts, one 2-bit code or RD_BAD per byte in LDS), its staging from bytes
// and the walk are nte_tile.h's; the k limit is this unit's own.
constexpr int RD_TPB = TILE_TPB;
constexpr int RD_TILE = TILE_STARTS;
constexpr int RD_MAXK = 200;
static_assert(RD_MAXK <= TILE_MAXK, "the tile's halo holds the unit's largest k");
constexpr u8 RD_BAD = CODE_BAD;

struct RdFilter // one filter as the reads kernels address it
{
	u32* words;
	Filter f; // geometry only (f.data unused)
};

// One stored batch of the resident store: group g holds bases [16 g, 16 g + 16) of the batch's bytes, base j of the
// group in bits 2j..2j+1 of codes[g] (0..3 = ACGT, case folded) and bit j of valid[g] (1: one of ACGTacgt; 0: anything
// else, the '\n' between reads included, and every position past n).  groups = ceil(n / 16), both arrays that long.
struct RdPacked
{
	const u32* codes;
	const u16* valid;
};

// prologue shared by the walking kernels: seed tables + LUT in LDS, the tile's codes staged -- from the batch's bytes,
// or (PACKED) from its stored groups: the same LDS codes either way, RD_BAD where a base is not ACGTacgt or lies past n
template<bool PACKED>
__device__ __forceinline__ void
rd_stage(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, u64* s_tab, u8* s_lut,
         u8* s_codes)
{
	const u32 tid = threadIdx.x;
	tile_load_tabs(tabs, s_tab, tid);
	if (!PACKED) {
		tile_fill_lut(s_lut, true, tid); // k-mers of ACGTacgt only (as the filter build)
	}
	__syncthreads();
	const u64 tile_base = (u64)blockIdx.x * RD_TILE;
	if (PACKED) {
		const u32 n_chunks = (RD_TILE + k - 1 + 15) / 16;
		// one group of 16 bases per lane: 6 bytes in, 16 LDS codes out (RD_TILE is a multiple of 16, so a tile starts
		// on a group); groups past the batch are all RD_BAD, as the byte path pads with '\n'
		const u64 groups = (n + 15) / 16;
		for (u32 c = tid; c < n_chunks; c += RD_TPB) {
			const u64 g = tile_base / 16 + c;
			u32 codes = 0, valid = 0;
			if (g < groups) {
				codes = pk.codes[g];
				valid = pk.valid[g];
			}
#pragma unroll
			for (int q = 0; q < 4; q++) {
				u32 x = 0;
#pragma unroll
				for (int b = 0; b < 4; b++) {
					const int j = q * 4 + b;
					const u32 code = (valid >> j) & 1u ? (codes >> (2 * j)) & 3u : (u32)RD_BAD;
					x |= code << (8 * b);
				}
				*reinterpret_cast<u32*>(&s_codes[tile_phys(c * 16 + q * 4)]) = x;
			}
		}
		__syncthreads();
		return;
	}
	tile_stage(seq, n, tile_base, RD_TILE, k, s_lut, s_codes, tid, RD_TPB);
	__syncthreads();
}

template<bool POW2>
__device__ __forceinline__ u64
rd_slot(const Filter& f, u64 hv)
{
	return POW2 ? (hv & f.mask) : filter_slot(f, hv);
}

// byte s of the counter array := max(byte, v)
__device__ __forceinline__ void
byte_max(u32* words, u64 s, u32 v)
{
	u32* w = words + (s >> 2);
	const u32 sh = (u32)(s & 3) * 8;
	u32 old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	while (((old >> sh) & 0xFFu) < v) {
		const u32 prev = atomicCAS(w, old, (old & ~(0xFFu << sh)) | (v << sh));
		if (prev == old) {
			break;
		}
		old = prev;
	}
}

// est(x): the minimum of x's h sketch counters (k_solid, k_hist)
template<int H, bool POW2>
__device__ __forceinline__ u32
rd_est(const u8* sk_bytes, const Filter& f, const u64 (&hv)[H])
{
	u32 est = 255;
#pragma unroll
	for (int i = 0; i < H; i++) {
		const u32 c = sk_bytes[rd_slot<POW2>(f, hv[i])];
		est = c < est ? c : est;
	}
	return est;
}

// the h bits of one k-mer in a plain filter (k_solid2): a plain read first, the atomic only for a bit still unset
template<int H>
__device__ __forceinline__ void
rd_set_bits(const RdFilter& out, const u64 (&hv)[H])
{
#pragma unroll
	for (int i = 0; i < H; i++) {
		const u64 s = filter_slot(out.f, hv[i]);
		u32* w = out.words + (s >> 5);
		const u32 bit = 1u << (s & 31);
		if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) {
			atomicOr(w, bit);
		}
	}
}

// ------------------------------------------------------------------ k_count / k_solid / k_solid2 / k_hist
// One thread walks 64 consecutive k-mer starts of the tile.  The hash state is exact once k codes of ACGT have
// entered since the last RD_BAD (an RD_BAD code has zero seeds both ways, so it leaves nothing behind).
// PASS 0: k_count; 1: k_solid into bits; 2: k_solid into counters; 3: k_hist into s_hist (this wave's 256 bins);
// 4: k_solid2 into the bits of out (est >= cmin) and of out2 (est >= rmin)
template<int H, bool POW2, int PASS, bool PACKED = false>
__device__ __forceinline__ void
rd_walk(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, const DevParams& p, RdFilter sk,
        RdFilter out, u32 cmin, u32* s_hist, RdFilter out2 = RdFilter{}, u32 rmin = 0)
{
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	__shared__ u8 s_lut[256];
	__shared__ __attribute__((aligned(16))) u8 s_codes[TILE_LDS_BYTES];
	rd_stage<PACKED>(seq, pk, n, k, tabs, s_tab, s_lut, s_codes);

	TileWalk walk;
	walk.prime(s_codes, s_tab, threadIdx.x * TILE_L, k);
	const u8* sk_bytes = reinterpret_cast<const u8*>(sk.words);
	for (u32 j = 0; j < TILE_L; j++) {
		if (walk.valid()) {
			const u64 base = walk.base();
			u64 hv[H];
#pragma unroll
			for (int i = 0; i < H; i++) {
				hv[i] = hash_extend(base, p, i);
			}
			if (PASS == 0) {
#pragma unroll
				for (int i = 0; i < H; i++) {
					byte_sat_inc(sk.words, rd_slot<POW2>(sk.f, hv[i]));
				}
			} else if (PASS == 3) {
				atomicAdd(&s_hist[rd_est<H, POW2>(sk_bytes, sk.f, hv)], 1u);
			} else if (PASS == 4) {
				const u32 est = rd_est<H, POW2>(sk_bytes, sk.f, hv);
				if (est >= cmin) {
					rd_set_bits<H>(out, hv);
				}
				if (est >= rmin) {
					rd_set_bits<H>(out2, hv);
				}
			} else {
				const u32 est = rd_est<H, POW2>(sk_bytes, sk.f, hv);
				if (est >= cmin) {
#pragma unroll
					for (int i = 0; i < H; i++) {
						const u64 s = filter_slot(out.f, hv[i]);
						if (PASS == 1) {
							u32* w = out.words + (s >> 5);
							const u32 bit = 1u << (s & 31);
							if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) {
								atomicOr(w, bit);
							}
						} else {
							byte_max(out.words, s, est);
						}
					}
				}
			}
		}
		walk.roll_bytes(s_codes, s_tab, j);
	}
}

template<int H, bool POW2, bool PACKED>
__global__ __launch_bounds__(RD_TPB) void
k_count(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, DevParams p, RdFilter sk)
{
	rd_walk<H, POW2, 0, PACKED>(seq, pk, n, k, tabs, p, sk, sk, 0, nullptr);
}

template<int H, bool POW2, bool COUNTS, bool PACKED>
__global__ __launch_bounds__(RD_TPB) void
k_solid(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, DevParams p, RdFilter sk,
        RdFilter out, u32 cmin)
{
	rd_walk<H, POW2, COUNTS ? 2 : 1, PACKED>(seq, pk, n, k, tabs, p, sk, out, cmin, nullptr);
}

// Pass 2 with a reject cutoff: the staging, the hash roll and the h sketch gathers of est(x) -- what bounds k_solid --
// happen once for both outputs; two k_solid launches would do all three twice.
template<int H, bool POW2, bool PACKED>
__global__ __launch_bounds__(RD_TPB) void
k_solid2(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, DevParams p, RdFilter sk,
         RdFilter out, RdFilter out2, u32 cmin, u32 rmin)
{
	rd_walk<H, POW2, 4, PACKED>(seq, pk, n, k, tabs, p, sk, out, cmin, nullptr, out2, rmin);
}

// Occurrences crowd into a few bins near the coverage peak, so each wave adds into a sub-histogram of its own: a
// block's adds are one LDS atomic per k-mer, and its global traffic one 64-bit add per non-zero bin.  A tile holds
// 16384 k-mer starts, so 32-bit bins cannot overflow.  The sums are integers: the result is independent of order.
constexpr int RD_HIST_BINS = 256;
constexpr int RD_HIST_SUBS = RD_TPB / 64;

template<int H, bool POW2, bool PACKED>
__global__ __launch_bounds__(RD_TPB) void
k_hist(const u8* __restrict__ seq, RdPacked pk, u64 n, u32 k, const u64* __restrict__ tabs, DevParams p, RdFilter sk,
       unsigned long long* hist)
{
	__shared__ u32 s_hist[RD_HIST_SUBS * RD_HIST_BINS];
	for (u32 i = threadIdx.x; i < RD_HIST_SUBS * RD_HIST_BINS; i += RD_TPB) {
		s_hist[i] = 0;
	}
	// (rd_stage's barriers order the zeroing before any add)
	rd_walk<H, POW2, 3, PACKED>(seq, pk, n, k, tabs, p, sk, sk, 0, s_hist + (threadIdx.x / 64) * RD_HIST_BINS);
	__syncthreads();
	static_assert(RD_TPB == RD_HIST_BINS, "one thread per bin flushes");
	u32 sum = 0;
#pragma unroll
	for (int w = 0; w < RD_HIST_SUBS; w++) {
		sum += s_hist[w * RD_HIST_BINS + threadIdx.x];
	}
	if (sum) {
		atomicAdd(&hist[threadIdx.x], (unsigned long long)sum);
	}
}

// One thread per group of 16 bases of a batch of n bytes: its codes and validity bits (RdPacked).  Bytes past n are
// invalid, so the last group's tail reads nothing of the batch.
__global__ __launch_bounds__(256) void
k_pack(const u8* __restrict__ seq, u64 n, u32* __restrict__ codes, u16* __restrict__ valid)
{
	const u64 groups = (n + 15) / 16;
	for (u64 g = (u64)blockIdx.x * 256 + threadIdx.x; g < groups; g += (u64)gridDim.x * 256) {
		const u64 at = g * 16;
		u32 c = 0, v = 0;
		if (at + 16 <= n && ((uintptr_t)(seq + at) & 15) == 0) {
			const uint4 w = *reinterpret_cast<const uint4*>(seq + at);
			const u32 words[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
			for (int j = 0; j < 16; j++) {
				const u8 code = char_code((u8)(words[j / 4] >> (8 * (j % 4))));
				if (code <= 3) {
					c |= (u32)code << (2 * j);
					v |= 1u << j;
				}
			}
		} else {
			for (int j = 0; j < 16 && at + j < n; j++) {
				const u8 code = char_code(seq[at + j]);
				if (code <= 3) {
					c |= (u32)code << (2 * j);
					v |= 1u << j;
				}
			}
		}
		codes[g] = c;
		valid[g] = (u16)v;
	}
}

// non-zero bytes of an array of n_words 64-bit words (allocations are whole words, zero behind the counters)
__global__ __launch_bounds__(256) void
k_nonzero(const u64* __restrict__ w, u64 n_words, unsigned long long* total)
{
	__shared__ unsigned long long s_sum[256];
	unsigned long long acc = 0;
	for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (u64)gridDim.x * 256) {
		u64 x = w[i];
		x |= x >> 4;
		x |= x >> 2;
		x |= x >> 1;
		acc += __popcll(x & 0x0101010101010101ULL);
	}
	s_sum[threadIdx.x] = acc;
	__syncthreads();
	for (u32 s = 128; s > 0; s >>= 1) {
		if (threadIdx.x < s) {
			s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		atomicAdd(total, s_sum[0]);
	}
}

// ------------------------------------------------------------------ k_merge
// A pure stream of (n_src + 1) * n bytes: each lane moves 16 bytes per load / store, four 32-bit words of four bytes.
// gfx950 has no byte-SIMD add or max, so both work on the packed words with borrow/carry tricks (no byte crosses
// into its neighbour):
//   t     = (a & 0x7F..) + (b & 0x7F..) ^ ((a ^ b) & 0x80..)           bytewise a + b mod 256
//   carry = ((a & b) | ((a | b) & ~t)) & 0x80..                         the bytes that overflowed (full-adder carry out)
//   sat   = t | (carry >> 7) * 0xFF
//   d     = ((a | 0x80..) - (b & 0x7F..)) ^ ((a ^ ~b) & 0x80..)        bytewise a - b mod 256
//   lt    = ((~a & b) | ((~a | b) & d)) & 0x80..                        the bytes with a < b (borrow out)
//   max   = (a & ~m) | (b & m), m = (lt >> 7) * 0xFF
constexpr u32 MG_HI = 0x80808080u, MG_LO = 0x7F7F7F7Fu;

template<int OP>
__host__ __device__ __forceinline__ u32
merge_word(u32 a, u32 b)
{
	if (OP == NTEDIT_MERGE_SAT_ADD) {
		const u32 t = ((a & MG_LO) + (b & MG_LO)) ^ ((a ^ b) & MG_HI);
		const u32 carry = ((a & b) | ((a | b) & ~t)) & MG_HI;
		return t | ((carry >> 7) * 0xFFu);
	} else if (OP == NTEDIT_MERGE_OR) {
		return a | b;
	} else {
		const u32 d = ((a | MG_HI) - (b & MG_LO)) ^ ((a ^ ~b) & MG_HI);
		const u32 lt = ((~a & b) | ((~a | b) & d)) & MG_HI;
		const u32 m = (lt >> 7) * 0xFFu;
		return (a & ~m) | (b & m);
	}
}

constexpr int MG_TPB = 256;

// dst[0 .. n) = fold of srcs[i * n + x] over i.  VEC: dst and every chunk are 16-byte aligned, so [0, n & ~15) moves in
// 16-byte vectors and the last n % 16 bytes one by one; otherwise every byte goes one by one.  dst may alias chunk 0
// (each byte is read by the thread that writes it).
template<int OP, bool VEC>
__global__ __launch_bounds__(MG_TPB) void
k_merge(u8* dst, const u8* srcs, u32 n_src, u64 n)
{
	const u64 stride = (u64)gridDim.x * MG_TPB;
	const u64 tid = (u64)blockIdx.x * MG_TPB + threadIdx.x;
	u64 tail = 0;
	if (VEC) {
		const u64 n16 = n / 16;
		for (u64 v = tid; v < n16; v += stride) {
			uint4 acc = reinterpret_cast<const uint4*>(srcs)[v];
			for (u32 i = 1; i < n_src; i++) {
				const uint4 x = reinterpret_cast<const uint4*>(srcs + (u64)i * n)[v];
				acc.x = merge_word<OP>(acc.x, x.x);
				acc.y = merge_word<OP>(acc.y, x.y);
				acc.z = merge_word<OP>(acc.z, x.z);
				acc.w = merge_word<OP>(acc.w, x.w);
			}
			reinterpret_cast<uint4*>(dst)[v] = acc;
		}
		tail = n16 * 16;
	}
	for (u64 x = tail + tid; x < n; x += stride) {
		u32 acc = srcs[x];
		for (u32 i = 1; i < n_src; i++) {
			acc = merge_word<OP>(acc, srcs[(u64)i * n + x]) & 0xFFu;
		}
		dst[x] = (u8)acc;
	}
}

// ------------------------------------------------------------------ host side
struct ReadsState
{
	const ntedit_hip_ctx* owner = nullptr;
	int device = 0;
	hipStream_t stream = nullptr;
	u8* sketch = nullptr; // counters, zero-filled up to a whole 64-bit word
	bool adopted = false; // the sketch is the caller's memory (ntedit_hip_sketch_set_device)
	u64 counters = 0;
	u32 hash_num = 0, k = 0;
	DevParams dp;
	u64* d_tab = nullptr;
	u8* d_seq = nullptr; // staging of host batches (grow-only)
	u64 seq_cap = 0;
	unsigned long long* d_total = nullptr;
	unsigned long long* d_hist = nullptr; // 256 bins of k_hist (zeroed at ntedit_hip_sketch_alloc)
	// the resident store (ntedit_hip_resident_begin): every batch of pass 1, packed, while it stays within store_cap
	struct Stored
	{
		void* mem; // codes (groups u32, padded to 16 bytes), then valid (groups u16)
		u64 n;
	};
	std::vector<Stored> store;
	u64 store_bytes = 0, store_cap = 0;
	int store_state = NTEDIT_RESIDENT_OFF;
	u32 reject_cmin = 0; // ntedit_hip_reads_set_reject_cutoff: the SOLID pass of ntedit_hip_reads_pass fills both slots
	u32 min_read = 0;    // ntedit_hip_reads_set_min_read: the shortest record the parsers keep (0: k)
	std::string err;
};

u64
stored_groups(u64 n)
{
	return (n + 15) / 16;
}

u64
stored_bytes(u64 n)
{
	return (stored_groups(n) * 4 + 15) / 16 * 16 + stored_groups(n) * 2;
}

RdPacked
stored_view(const ReadsState::Stored& b)
{
	RdPacked pk;
	pk.codes = (const u32*)b.mem;
	pk.valid = (const u16*)((const u8*)b.mem + (stored_groups(b.n) * 4 + 15) / 16 * 16);
	return pk;
}

void
drop_store(ReadsState* s, int state)
{
	for (ReadsState::Stored& b : s->store) {
		(void)hipFree(b.mem);
	}
	s->store.clear();
	s->store_bytes = 0;
	s->store_state = state;
}

std::mutex g_reads_mu;
std::vector<ReadsState*> g_reads;       // one per context that holds a sketch
std::vector<std::pair<const ntedit_hip_ctx*, std::string>> g_reads_err; // last failure per context

int
rfail(const ntedit_hip_ctx* c, int code, const char* fmt, ...)
{
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	std::lock_guard<std::mutex> lk(g_reads_mu);
	for (auto& e : g_reads_err) {
		if (e.first == c) {
			e.second = buf;
			return code;
		}
	}
	g_reads_err.emplace_back(c, buf);
	return code;
}

#define RD_TRY(ctx, expr)                                                                        \
	do {                                                                                         \
		hipError_t e_ = (expr);                                                                  \
		if (e_ != hipSuccess) {                                                                  \
			return rfail((ctx), NTEDIT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));        \
		}                                                                                        \
	} while (0)

// the context's state, with its sketch or after ntedit_hip_sketch_reset released the counters and kept the store
ReadsState*
find_any_state(const ntedit_hip_ctx* c)
{
	std::lock_guard<std::mutex> lk(g_reads_mu);
	for (ReadsState* s : g_reads) {
		if (s->owner == c) {
			return s;
		}
	}
	return nullptr;
}

// ... and only while it holds a sketch: what every call that touches the counters asks for
ReadsState*
find_state(const ntedit_hip_ctx* c)
{
	ReadsState* s = find_any_state(c);
	return s && s->sketch ? s : nullptr;
}

void
release_state(ReadsState* s)
{
	(void)hipSetDevice(s->device);
	if (s->stream) {
		(void)hipStreamSynchronize(s->stream);
		(void)hipStreamDestroy(s->stream);
	}
	drop_store(s, NTEDIT_RESIDENT_OFF);
	for (void* p : { s->adopted ? nullptr : (void*)s->sketch, (void*)s->d_tab, (void*)s->d_seq, (void*)s->d_total, (void*)s->d_hist }) {
		if (p) {
			(void)hipFree(p);
		}
	}
	delete s;
}

Filter
geometry(u64 slots, u32 hash_num, bool counting)
{
	Filter f;
	f.data = nullptr;
	filter_set_size(f, slots);
	f.hash_num = hash_num;
	f.counting = counting ? 1 : 0;
	return f;
}

// the batch in HBM (host batches are copied into the state's staging buffer)
int
stage(const ntedit_hip_ctx* c, ReadsState* s, const char* bases, u64 n, int on_device, const u8** d_seq)
{
	if (on_device == NTEDIT_HIP_BASES_DEVICE) {
		if ((uintptr_t)bases & 15) {
			return rfail(c, NTEDIT_E_ARG, "reads: device batches must be 16-byte aligned");
		}
		*d_seq = (const u8*)bases;
		return 0;
	}
	if (on_device != NTEDIT_HIP_BASES_HOST) {
		return rfail(c, NTEDIT_E_ARG, "reads: bases must be host or device bytes");
	}
	if (n > s->seq_cap) {
		if (s->d_seq) {
			RD_TRY(c, hipFree(s->d_seq));
			s->d_seq = nullptr;
			s->seq_cap = 0;
		}
		RD_TRY(c, hipMalloc((void**)&s->d_seq, n + 64));
		s->seq_cap = n;
	}
	RD_TRY(c, hipMemcpyAsync(s->d_seq, bases, n, hipMemcpyHostToDevice, s->stream));
	*d_seq = s->d_seq;
	return 0;
}

template<bool POW2, int PASS, bool PACKED>
void
launch_walk(ReadsState* s, const u8* d_seq, RdPacked pk, u64 n, u64 tiles, RdFilter sk, RdFilter out, u32 cmin, RdFilter out2,
            u32 rmin)
{
	dim3 grid((unsigned)tiles), block(RD_TPB);
#define RD_LAUNCH(H)                                                                                               \
	case H:                                                                                                        \
		if constexpr (PASS == 0) {                                                                                 \
			hipLaunchKernelGGL((k_count<H, POW2, PACKED>), grid, block, 0, s->stream, d_seq, pk, n, s->k, s->d_tab,   \
			                   s->dp, sk);                                                                         \
		} else if constexpr (PASS == 4) {                                                                          \
			hipLaunchKernelGGL((k_solid2<H, POW2, PACKED>), grid, block, 0, s->stream, d_seq, pk, n, s->k, s->d_tab,  \
			                   s->dp, sk, out, out2, cmin, rmin);                                                  \
		} else if constexpr (PASS == 3) {                                                                          \
			hipLaunchKernelGGL((k_hist<H, POW2, PACKED>), grid, block, 0, s->stream, d_seq, pk, n, s->k, s->d_tab, \
			                   s->dp, sk, s->d_hist);                                                              \
		} else {                                                                                                   \
			hipLaunchKernelGGL((k_solid<H, POW2, PASS == 2, PACKED>), grid, block, 0, s->stream, d_seq, pk, n, s->k, \
			                   s->d_tab, s->dp, sk, out, cmin);                                                    \
		}                                                                                                          \
		break
	switch (s->hash_num) {
		RD_LAUNCH(1);
		RD_LAUNCH(2);
		RD_LAUNCH(3);
		RD_LAUNCH(4);
		RD_LAUNCH(5);
		RD_LAUNCH(6);
		RD_LAUNCH(7);
		RD_LAUNCH(8);
	default:
		break;
	}
#undef RD_LAUNCH
}

RdFilter
sketch_view(const ReadsState* s)
{
	RdFilter sk;
	sk.words = (u32*)s->sketch;
	sk.f = geometry(s->counters, s->hash_num, true);
	return sk;
}

template<bool PACKED>
void
launch_pass(ReadsState* s, const u8* d_seq, RdPacked pk, u64 n, u64 tiles, int pass, RdFilter out, u32 cmin, RdFilter out2, u32 rmin)
{
	const RdFilter sk = sketch_view(s);
	const bool pow2 = sk.f.mask != 0;
	if (pass == 1) {
		pow2 ? launch_walk<true, 1, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin)
		     : launch_walk<false, 1, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin);
	} else if (pass == 2) {
		pow2 ? launch_walk<true, 2, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin)
		     : launch_walk<false, 2, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin);
	} else if (pass == 4) {
		pow2 ? launch_walk<true, 4, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin)
		     : launch_walk<false, 4, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin);
	} else if (pass == 3) {
		pow2 ? launch_walk<true, 3, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin)
		     : launch_walk<false, 3, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin);
	} else {
		pow2 ? launch_walk<true, 0, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin)
		     : launch_walk<false, 0, PACKED>(s, d_seq, pk, n, tiles, sk, out, cmin, out2, rmin);
	}
}

// after k_count: the batch packed into the resident store, or the store dropped when it would pass its cap or an
// allocation fails (the later passes then read the inputs again)
void
store_batch(ReadsState* s, const u8* d_seq, u64 n)
{
	const u64 bytes = stored_bytes(n);
	if (s->store_bytes + bytes > s->store_cap) {
		drop_store(s, NTEDIT_RESIDENT_OVER_CAP);
		return;
	}
	ReadsState::Stored b = { nullptr, n };
	if (hipMalloc(&b.mem, bytes) != hipSuccess) {
		(void)hipGetLastError(); // (a failed allocation leaves no error behind for the next check)
		drop_store(s, NTEDIT_RESIDENT_NO_MEMORY);
		return;
	}
	s->store.push_back(b);
	s->store_bytes += bytes;
	const RdPacked pk = stored_view(b);
	const u64 groups = stored_groups(n), want = (groups + 255) / 256;
	hipLaunchKernelGGL(k_pack, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s->stream, d_seq, n,
	                   (u32*)pk.codes, (u16*)pk.valid);
}

int
run_pass(const ntedit_hip_ctx* c, ReadsState* s, const char* bases, u64 n, int on_device, int pass, RdFilter out, u32 cmin,
         RdFilter out2 = RdFilter{}, u32 rmin = 0)
{
	RD_TRY(c, hipSetDevice(s->device));
	if (n == 0) {
		return 0;
	}
	const u64 tiles = (n + RD_TILE - 1) / RD_TILE;
	if (tiles > 0x7FFFFFFFull) {
		return rfail(c, NTEDIT_E_ARG, "reads: batch too large");
	}
	const u8* d_seq = nullptr;
	int rc = stage(c, s, bases, n, on_device, &d_seq);
	if (rc) {
		return rc;
	}
	launch_pass<false>(s, d_seq, RdPacked{}, n, tiles, pass, out, cmin, out2, rmin);
	RD_TRY(c, hipGetLastError());
	if (pass == 0 && s->store_state == NTEDIT_RESIDENT_ON) {
		store_batch(s, d_seq, n);
		RD_TRY(c, hipGetLastError());
	}
	RD_TRY(c, hipStreamSynchronize(s->stream));
	return 0;
}

// pass 1, the histogram pass or pass 2 over every stored batch, each launched with its own n as it was stored
int
run_store_pass(const ntedit_hip_ctx* c, ReadsState* s, int pass, RdFilter out, u32 cmin, RdFilter out2 = RdFilter{}, u32 rmin = 0)
{
	RD_TRY(c, hipSetDevice(s->device));
	if (s->store_state != NTEDIT_RESIDENT_ON) {
		return rfail(c, NTEDIT_E_ARG, "resident_pass: the context holds no complete resident store");
	}
	for (const ReadsState::Stored& b : s->store) {
		const u64 tiles = (b.n + RD_TILE - 1) / RD_TILE;
		launch_pass<true>(s, nullptr, stored_view(b), b.n, tiles, pass, out, cmin, out2, rmin);
		RD_TRY(c, hipGetLastError());
	}
	RD_TRY(c, hipStreamSynchronize(s->stream));
	return 0;
}

// the output filter of pass 2 (filter_insert_solid and the store's pass 2 check it alike)
int
solid_target(const ntedit_hip_ctx* c, const ReadsState* s, int slot, u32 cmin, const char* what, RdFilter* out)
{
	if (cmin < 1 || cmin > 255) {
		return rfail(c, NTEDIT_E_ARG, "%s: cmin = %u: needs 1 <= cmin <= 255", what, cmin);
	}
	uint32_t k = 0, hash_num = 0;
	uint64_t nbytes = 0;
	int counting = 0;
	void* data = ntedit_hip_filter_device_ptr(c, slot);
	if (!data || ntedit_hip_filter_info(c, slot, &k, &hash_num, &nbytes, &counting) != 0) {
		return rfail(c, NTEDIT_E_NOFILTER, "%s: filter slot %d not set", what, slot);
	}
	if (k != s->k || hash_num != s->hash_num) {
		return rfail(c, NTEDIT_E_ARG, "%s: the filter has k = %u, hash_num = %u, the sketch k = %u, hash_num = %u", what,
		             k, hash_num, s->k, s->hash_num);
	}
	hipPointerAttribute_t attr;
	RD_TRY(c, hipPointerGetAttributes(&attr, data));
	if (attr.device != s->device) {
		return rfail(c, NTEDIT_E_ARG, "%s: the filter is on device %d, the sketch on device %d", what, attr.device, s->device);
	}
	out->words = (u32*)data;
	out->f = geometry(counting ? nbytes : nbytes * 8, hash_num, counting != 0);
	return 0;
}

// both outputs of pass 2 with a reject cutoff: PRIMARY takes cmin, SECONDARY (a plain filter) rmin
int
solid2_targets(const ntedit_hip_ctx* c, const ReadsState* s, u32 cmin, u32 rmin, const char* what, RdFilter* out, RdFilter* out2)
{
	if (!(cmin < rmin && rmin <= 255)) {
		return rfail(c, NTEDIT_E_ARG, "%s: cmin = %u, rmin = %u: needs cmin < rmin <= 255", what, cmin, rmin);
	}
	int rc = solid_target(c, s, NTEDIT_FILTER_PRIMARY, cmin, what, out);
	if (rc == 0) {
		rc = solid_target(c, s, NTEDIT_FILTER_SECONDARY, rmin, what, out2);
	}
	if (rc) {
		return rc;
	}
	if (out->f.counting || out2->f.counting) {
		return rfail(c, NTEDIT_E_ARG, "%s: the %s filter is a counting filter: the reject filter and the filter built with it are plain",
		             what, out2->f.counting ? "SECONDARY" : "PRIMARY");
	}
	return 0;
}

} // namespace

namespace nte_reads {
int
set_error(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return rfail(c, code, "%s", why.c_str());
}
uint32_t
reject_cutoff(const ntedit_hip_ctx* c)
{
	const ReadsState* s = find_state(c);
	return s ? s->reject_cmin : 0;
}
uint32_t
min_read(const ntedit_hip_ctx* c, uint32_t k)
{
	const ReadsState* s = find_state(c);
	return s && s->min_read && s->min_read < k ? s->min_read : k;
}
} // namespace nte_reads

extern "C" {

const char*
ntedit_hip_reads_last_error(const ntedit_hip_ctx* c)
{
	std::lock_guard<std::mutex> lk(g_reads_mu);
	for (auto& e : g_reads_err) {
		if (e.first == c) {
			return e.second.c_str();
		}
	}
	return "";
}

static int make_state(ntedit_hip_ctx* c, uint64_t counters, uint32_t hash_num, uint32_t k, void* adopt, bool keep_store = false);

int
ntedit_hip_sketch_alloc(ntedit_hip_ctx* c, uint64_t counters, uint32_t hash_num, uint32_t k)
{
	return make_state(c, counters, hash_num, k, nullptr);
}

int
ntedit_hip_sketch_set_device(ntedit_hip_ctx* c, void* device_counters, uint64_t counters, uint32_t hash_num, uint32_t k)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	if (!device_counters || ((uintptr_t)device_counters & 15) || counters % 8) {
		return rfail(c, NTEDIT_E_ARG, "sketch_set_device: needs a 16-byte aligned device pointer and a multiple of 8 counters");
	}
	return make_state(c, counters, hash_num, k, device_counters);
}

int
ntedit_hip_sketch_info(ntedit_hip_ctx* c, uint64_t* counters, uint32_t* hash_num, uint32_t* k)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_info: no sketch") : NTEDIT_E_ARG;
	}
	if (counters) {
		*counters = s->counters;
	}
	if (hash_num) {
		*hash_num = s->hash_num;
	}
	if (k) {
		*k = s->k;
	}
	return 0;
}

int
ntedit_hip_merge_bytes(ntedit_hip_ctx* c, void* dst, const void* srcs, uint32_t n_src, uint64_t n, int op)
{
	if (!c || !dst || !srcs || n_src == 0 || op < NTEDIT_MERGE_SAT_ADD || op > NTEDIT_MERGE_MAX) {
		return c ? rfail(c, NTEDIT_E_ARG, "merge_bytes: bad argument") : NTEDIT_E_ARG;
	}
	if (n == 0) {
		return 0;
	}
	hipPointerAttribute_t attr;
	RD_TRY(c, hipPointerGetAttributes(&attr, dst));
	if (attr.type != hipMemoryTypeDevice) {
		return rfail(c, NTEDIT_E_ARG, "merge_bytes: dst is not device memory");
	}
	RD_TRY(c, hipSetDevice(attr.device));
	const bool vec = (((uintptr_t)dst | (uintptr_t)srcs) & 15) == 0 && (n % 16 == 0 || n_src == 1);
	const u64 items = vec ? n / 16 + n % 16 : n;
	int cus = 256;
	(void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, attr.device);
	const u64 want = (items + MG_TPB - 1) / MG_TPB, cap = (u64)cus * 8;
	const dim3 grid((unsigned)(want < cap ? want : cap)), block(MG_TPB);
	u8* d = (u8*)dst;
	const u8* sp = (const u8*)srcs;
#define MG_LAUNCH(OP)                                                                              \
	case OP:                                                                                       \
		if (vec) {                                                                                 \
			hipLaunchKernelGGL((k_merge<OP, true>), grid, block, 0, nullptr, d, sp, n_src, n);   \
		} else {                                                                                   \
			hipLaunchKernelGGL((k_merge<OP, false>), grid, block, 0, nullptr, d, sp, n_src, n);  \
		}                                                                                          \
		break
	switch (op) {
		MG_LAUNCH(NTEDIT_MERGE_SAT_ADD);
		MG_LAUNCH(NTEDIT_MERGE_OR);
		MG_LAUNCH(NTEDIT_MERGE_MAX);
	default:
		break;
	}
#undef MG_LAUNCH
	RD_TRY(c, hipGetLastError());
	RD_TRY(c, hipStreamSynchronize(nullptr));
	return 0;
}

static int
make_state(ntedit_hip_ctx* c, uint64_t counters, uint32_t hash_num, uint32_t k, void* adopt, bool keep_store)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	if (counters == 0 || hash_num == 0 || hash_num > MAX_HASHES || k < 12 || k > RD_MAXK) {
		return rfail(c, NTEDIT_E_ARG, "sketch_alloc: %llu counters, hash_num = %u, k = %u: needs counters > 0, hash_num in [1, %u] and k in [12, %u]",
		             (unsigned long long)counters, hash_num, k, MAX_HASHES, RD_MAXK);
	}
	// ntedit_hip_sketch_reset: the store and the settings that go with the reads, not with one sketch, move to the new
	// state (the old stream is drained first: the store's pack kernels ran on it)
	// (every call that can fail comes before the store changes hands: a failure here leaves the old state whole)
	int device = 0;
	RD_TRY(c, hipGetDevice(&device));
	ReadsState carried;
	ReadsState* old = find_any_state(c);
	if (old) {
		device = old->device; // (releasing the old state makes its device current, as it always did)
	}
	if (old && keep_store) {
		RD_TRY(c, hipSetDevice(old->device));
		RD_TRY(c, hipStreamSynchronize(old->stream));
		carried.store.swap(old->store);
		carried.store_bytes = old->store_bytes;
		carried.store_cap = old->store_cap;
		carried.store_state = old->store_state;
		carried.min_read = old->min_read;
		old->store_bytes = 0;
		old->store_state = NTEDIT_RESIDENT_OFF;
	}
	ntedit_hip_sketch_free(c);
	ReadsState* s = new ReadsState();
	s->owner = c;
	s->device = device;
	s->store.swap(carried.store);
	s->store_bytes = carried.store_bytes;
	s->store_cap = carried.store_cap;
	s->store_state = carried.store_state;
	s->min_read = carried.min_read;
	s->counters = (counters + 7) / 8 * 8; // btllib rounds a counting filter up to whole 64-bit words
	s->adopted = adopt != nullptr;
	s->sketch = (u8*)adopt;
	s->hash_num = hash_num;
	s->k = k;
	ntedit_hip_params hp;
	nte_host::params_default(&hp);
	int rc = nte_host::make_dev_params(hp, k, hash_num, false, &s->dp);
	u64 tab[TAB_WORDS];
	build_seed_tables(k, tab);
	hipError_t e = rc ? hipSuccess : hipStreamCreate(&s->stream);
	if (e == hipSuccess && !rc && !adopt) {
		e = hipMalloc((void**)&s->sketch, s->counters);
	}
	if (e == hipSuccess && !rc) {
		e = hipMalloc((void**)&s->d_tab, sizeof tab);
	}
	if (e == hipSuccess && !rc) {
		e = hipMalloc((void**)&s->d_total, 8);
	}
	if (e == hipSuccess && !rc) {
		e = hipMalloc((void**)&s->d_hist, 256 * sizeof(unsigned long long));
	}
	if (e == hipSuccess && !rc && !adopt) {
		e = hipMemsetAsync(s->sketch, 0, s->counters, s->stream);
	}
	if (e == hipSuccess && !rc) {
		e = hipMemsetAsync(s->d_hist, 0, 256 * sizeof(unsigned long long), s->stream);
	}
	if (e == hipSuccess && !rc) {
		e = hipMemcpyAsync(s->d_tab, tab, sizeof tab, hipMemcpyHostToDevice, s->stream);
	}
	if (e == hipSuccess && !rc) {
		e = hipStreamSynchronize(s->stream);
	}
	if (rc || e != hipSuccess) {
		release_state(s);
		if (rc) {
			return rfail(c, rc, "sketch_alloc: unsupported k / hash_num");
		}
		return rfail(c, NTEDIT_E_DEVICE, "sketch_alloc: %llu counters: %s", (unsigned long long)counters, hipGetErrorString(e));
	}
	std::lock_guard<std::mutex> lk(g_reads_mu);
	g_reads.push_back(s);
	return 0;
}

void
ntedit_hip_sketch_free(ntedit_hip_ctx* c)
{
	nte_reads::parse_release(c); // (the device parser's scratch, nte_reads_parse.hip)
	ReadsState* s = nullptr;
	{
		std::lock_guard<std::mutex> lk(g_reads_mu);
		for (size_t i = 0; i < g_reads.size(); i++) {
			if (g_reads[i]->owner == c) {
				s = g_reads[i];
				g_reads.erase(g_reads.begin() + (long)i);
				break;
			}
		}
	}
	if (s) {
		release_state(s);
	}
}

int
ntedit_hip_sketch_count(ntedit_hip_ctx* c, const char* bases, uint64_t n, int on_device)
{
	ReadsState* s = find_state(c);
	if (!c || !bases) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_count: bad argument") : NTEDIT_E_ARG;
	}
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "sketch_count: no sketch (ntedit_hip_sketch_alloc)");
	}
	RdFilter none = {};
	return run_pass(c, s, bases, n, on_device, 0, none, 0);
}

int
ntedit_hip_sketch_histogram(ntedit_hip_ctx* c, const char* bases, uint64_t n, int on_device)
{
	ReadsState* s = find_state(c);
	if (!c || !bases) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_histogram: bad argument") : NTEDIT_E_ARG;
	}
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "sketch_histogram: no sketch (ntedit_hip_sketch_alloc)");
	}
	RdFilter none = {};
	return run_pass(c, s, bases, n, on_device, 3, none, 0);
}

int
ntedit_hip_sketch_histogram_download(ntedit_hip_ctx* c, uint64_t occ[256])
{
	ReadsState* s = find_state(c);
	if (!s || !occ) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_histogram_download: bad argument or no sketch") : NTEDIT_E_ARG;
	}
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit bins");
	RD_TRY(c, hipSetDevice(s->device));
	RD_TRY(c, hipMemcpy(occ, s->d_hist, 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
	return 0;
}

int
ntedit_hip_reads_hist_summary(const uint64_t occ[256], uint64_t f[256], uint64_t* F0, uint64_t* F1)
{
	if (!occ || !f || !F0 || !F1) {
		return rfail(nullptr, NTEDIT_E_ARG, "reads_hist_summary: bad argument");
	}
	uint64_t f0 = 0, f1 = occ[0];
	f[0] = 0;
	for (uint64_t c = 1; c < 256; c++) {
		f1 += occ[c];
		f[c] = (occ[c] + c / 2) / c;
		f0 += f[c];
	}
	*F0 = f0;
	*F1 = f1;
	return 0;
}

int
ntedit_hip_reads_solid_cutoff(const uint64_t f[256], uint32_t* cmin)
{
	if (!f || !cmin) {
		return rfail(nullptr, NTEDIT_E_ARG, "reads_solid_cutoff: bad argument");
	}
	for (uint32_t c = 1; c <= 253; c++) {
		if (f[c + 1] > f[c]) {
			*cmin = c;
			return 0;
		}
	}
	return rfail(nullptr, NTEDIT_E_ARG, "reads_solid_cutoff: the k-mer histogram has no valley (no c in [1, 253] with f[c+1] > f[c])");
}

int
ntedit_hip_sketch_occupancy(ntedit_hip_ctx* c, uint64_t* nonzero, uint64_t* counters)
{
	ReadsState* s = find_state(c);
	if (!s || !nonzero) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_occupancy: bad argument or no sketch") : NTEDIT_E_ARG;
	}
	RD_TRY(c, hipSetDevice(s->device));
	RD_TRY(c, hipMemsetAsync(s->d_total, 0, 8, s->stream));
	hipLaunchKernelGGL(k_nonzero, dim3(1024), dim3(256), 0, s->stream, (const u64*)s->sketch, s->counters / 8, s->d_total);
	RD_TRY(c, hipGetLastError());
	unsigned long long h = 0;
	RD_TRY(c, hipMemcpyAsync(&h, s->d_total, 8, hipMemcpyDeviceToHost, s->stream));
	RD_TRY(c, hipStreamSynchronize(s->stream));
	*nonzero = h;
	if (counters) {
		*counters = s->counters;
	}
	return 0;
}

int
ntedit_hip_sketch_download(ntedit_hip_ctx* c, uint8_t* counters)
{
	ReadsState* s = find_state(c);
	if (!s || !counters) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_download: bad argument or no sketch") : NTEDIT_E_ARG;
	}
	RD_TRY(c, hipSetDevice(s->device));
	RD_TRY(c, hipMemcpy(counters, s->sketch, s->counters, hipMemcpyDeviceToHost));
	return 0;
}

int
ntedit_hip_sketch_save_file(ntedit_hip_ctx* c, const char* path)
{
	ReadsState* s = find_state(c);
	if (!s || !path) {
		return c ? rfail(c, NTEDIT_E_ARG, "sketch_save_file: bad argument or no sketch") : NTEDIT_E_ARG;
	}
	std::vector<u8> host(s->counters);
	int rc = ntedit_hip_sketch_download(c, host.data());
	if (rc) {
		return rc;
	}
	nte_host::BfHeader h;
	h.bytes = s->counters;
	h.hash_num = s->hash_num;
	h.k = s->k;
	h.counting = true;
	if (nte_host::bf_save(path, h, host.data())) {
		return rfail(c, NTEDIT_E_IO, "`%s': cannot write", path);
	}
	return 0;
}

int
ntedit_hip_filter_alloc_counting(ntedit_hip_ctx* c, int slot, uint64_t nbytes, uint32_t hash_num, uint32_t k)
{
	if (!c || slot < 0 || slot > 1 || nbytes == 0 || hash_num == 0 || hash_num > MAX_HASHES) {
		return c ? rfail(c, NTEDIT_E_ARG, "filter_alloc_counting: bad argument") : NTEDIT_E_ARG;
	}
	nbytes = (nbytes + 7) / 8 * 8; // as ntedit_hip_filter_alloc (btllib: whole 64-bit words)
	// calloc'd pages are the kernel's zero page until written: the upload reads them without committing memory
	void* zeros = calloc(nbytes, 1);
	if (!zeros) {
		return rfail(c, NTEDIT_E_ARG, "filter_alloc_counting: %llu bytes of host memory", (unsigned long long)nbytes);
	}
	const int rc = ntedit_hip_set_filter(c, slot, (const uint8_t*)zeros, nbytes, hash_num, k, 1);
	free(zeros);
	if (rc) {
		return rfail(c, rc, "filter_alloc_counting: %s", ntedit_hip_last_error(c));
	}
	return 0;
}

int
ntedit_hip_filter_insert_solid(ntedit_hip_ctx* c, int slot, const char* bases, uint64_t n, int on_device, uint32_t cmin)
{
	if (!c || !bases || slot < 0 || slot > 1) {
		return c ? rfail(c, NTEDIT_E_ARG, "filter_insert_solid: bad argument") : NTEDIT_E_ARG;
	}
	ReadsState* s = find_state(c);
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "filter_insert_solid: no sketch (ntedit_hip_sketch_alloc)");
	}
	RdFilter out;
	const int rc = solid_target(c, s, slot, cmin, "filter_insert_solid", &out);
	if (rc) {
		return rc;
	}
	return run_pass(c, s, bases, n, on_device, out.f.counting ? 2 : 1, out, cmin);
}

int
ntedit_hip_filter_insert_solid2(ntedit_hip_ctx* c, const char* bases, uint64_t n, int on_device, uint32_t cmin, uint32_t rmin)
{
	if (!c || !bases) {
		return c ? rfail(c, NTEDIT_E_ARG, "filter_insert_solid2: bad argument") : NTEDIT_E_ARG;
	}
	ReadsState* s = find_state(c);
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "filter_insert_solid2: no sketch (ntedit_hip_sketch_alloc)");
	}
	RdFilter out, out2;
	const int rc = solid2_targets(c, s, cmin, rmin, "filter_insert_solid2", &out, &out2);
	if (rc) {
		return rc;
	}
	return run_pass(c, s, bases, n, on_device, 4, out, cmin, out2, rmin);
}

int
ntedit_hip_reads_set_reject_cutoff(ntedit_hip_ctx* c, uint32_t rmin)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "reads_set_reject_cutoff: no sketch (ntedit_hip_sketch_alloc / _set_device)") : NTEDIT_E_ARG;
	}
	if (rmin > 255) {
		return rfail(c, NTEDIT_E_ARG, "reads_set_reject_cutoff: rmin = %u: needs rmin <= 255", rmin);
	}
	s->reject_cmin = rmin;
	return 0;
}

int
ntedit_hip_resident_begin(ntedit_hip_ctx* c, uint64_t cap_bytes)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "resident_begin: no sketch (ntedit_hip_sketch_alloc / _set_device)") : NTEDIT_E_ARG;
	}
	RD_TRY(c, hipSetDevice(s->device));
	RD_TRY(c, hipStreamSynchronize(s->stream));
	drop_store(s, NTEDIT_RESIDENT_ON);
	s->store_cap = cap_bytes;
	return 0;
}

int
ntedit_hip_resident_info(ntedit_hip_ctx* c, ntedit_hip_resident_stats* st)
{
	ReadsState* s = find_any_state(c); // (the store outlives the counters: ntedit_hip_sketch_reset)
	if (!s || !st) {
		return c ? rfail(c, NTEDIT_E_ARG, "resident_info: bad argument or no sketch") : NTEDIT_E_ARG;
	}
	st->state = s->store_state;
	st->batches = s->store.size();
	st->bases = 0;
	for (const ReadsState::Stored& b : s->store) {
		st->bases += b.n;
	}
	st->bytes = s->store_bytes;
	st->cap = s->store_cap;
	return 0;
}

int
ntedit_hip_resident_histogram(ntedit_hip_ctx* c)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "resident_histogram: no sketch (ntedit_hip_sketch_alloc / _set_device)") : NTEDIT_E_ARG;
	}
	RdFilter none = {};
	return run_store_pass(c, s, 3, none, 0);
}

int
ntedit_hip_resident_insert_solid(ntedit_hip_ctx* c, int slot, uint32_t cmin)
{
	if (!c || slot < 0 || slot > 1) {
		return c ? rfail(c, NTEDIT_E_ARG, "resident_insert_solid: bad argument") : NTEDIT_E_ARG;
	}
	ReadsState* s = find_state(c);
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "resident_insert_solid: no sketch (ntedit_hip_sketch_alloc / _set_device)");
	}
	RdFilter out;
	const int rc = solid_target(c, s, slot, cmin, "resident_insert_solid", &out);
	if (rc) {
		return rc;
	}
	return run_store_pass(c, s, out.f.counting ? 2 : 1, out, cmin);
}

int
ntedit_hip_resident_insert_solid2(ntedit_hip_ctx* c, uint32_t cmin, uint32_t rmin)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	ReadsState* s = find_state(c);
	if (!s) {
		return rfail(c, NTEDIT_E_ARG, "resident_insert_solid2: no sketch (ntedit_hip_sketch_alloc / _set_device)");
	}
	RdFilter out, out2;
	const int rc = solid2_targets(c, s, cmin, rmin, "resident_insert_solid2", &out, &out2);
	if (rc) {
		return rc;
	}
	return run_store_pass(c, s, 4, out, cmin, out2, rmin);
}

int
ntedit_hip_resident_count(ntedit_hip_ctx* c)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "resident_count: no sketch (ntedit_hip_sketch_reset / _alloc / _set_device)") : NTEDIT_E_ARG;
	}
	RdFilter none = {};
	return run_store_pass(c, s, 0, none, 0);
}

int
ntedit_hip_sketch_reset(ntedit_hip_ctx* c, uint64_t counters, uint32_t hash_num, uint32_t k)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	if (counters == 0) {
		// the counters alone are released: the state stays for its store, and holds no sketch until the next reset
		nte_reads::parse_release(c);
		ReadsState* s = find_any_state(c);
		if (s && s->sketch) {
			RD_TRY(c, hipSetDevice(s->device));
			RD_TRY(c, hipStreamSynchronize(s->stream));
			if (!s->adopted) {
				RD_TRY(c, hipFree(s->sketch));
			}
			s->sketch = nullptr;
			s->adopted = false;
			s->counters = 0;
			s->reject_cmin = 0;
		}
		if (s && s->d_seq) {
			RD_TRY(c, hipFree(s->d_seq)); // (the staging of host batches: the polish sizes its own buffers next)
			s->d_seq = nullptr;
			s->seq_cap = 0;
		}
		return 0;
	}
	return make_state(c, counters, hash_num, k, nullptr, true);
}

int
ntedit_hip_reads_set_min_read(ntedit_hip_ctx* c, uint32_t len)
{
	ReadsState* s = find_state(c);
	if (!s) {
		return c ? rfail(c, NTEDIT_E_ARG, "reads_set_min_read: no sketch (ntedit_hip_sketch_alloc / _set_device)") : NTEDIT_E_ARG;
	}
	s->min_read = len;
	return 0;
}

void
ntedit_hip_resident_free(ntedit_hip_ctx* c)
{
	ReadsState* s = find_any_state(c);
	if (s) {
		(void)hipSetDevice(s->device);
		(void)hipStreamSynchronize(s->stream);
		drop_store(s, NTEDIT_RESIDENT_OFF);
	}
}

} // extern "C"
