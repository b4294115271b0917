// nte_bin_wc.inc -- write-combining partition of the probe records (included by nte_kernels.hip).
//
// The binned screening pipeline (see "binned screening" in nte_kernels.hip) makes the Bloom probes
// L2-resident by sorting the h probes of every k-mer by filter slice first.  Its cost is moving
// 8 bytes per probe; this file is the software write-combiner that moves them as full 64-byte
// segments, ONE pass over the draft, no counting pass:
//
//   layout        the record array is a matrix of RUNS, one per (slice, persistent workgroup) pair,
//                 `cap` records apart (cap = expected records of a pair + 6 sigma, host-computed).
//                 A pair that gets more than `cap` (repeats: the same k-mers again and again -- simple-sequence
//                 arrays, satellites) sends the excess to the overflow list, which is probed directly.  The list is
//                 sized as a share of the chunk's records and handed out in blocks of WC_OVF_BLOCK entries, one
//                 global atomic per block and wavefront (OvfCursor); a list that runs out all the same costs the
//                 CHUNK its binned screening (k_ovf_check: the host screens that chunk again with k_screen).
//   k_wc_scatter_b  (default; further down) the barrier-phased partition kernel: tiles of 1,024 threads x 32 k-mer starts,
//                 staged as 4-bit codes, two per byte (the packed tile of nte_tile.h: one staging, one barrier and one
//                 prime of k rolls per 32 starts, in the LDS 16 starts per thread took as bytes); rounds of one k-mer
//                 per thread, records into the rings, barrier, complete 64-byte groups out, barrier.
//   k_wc_scatter  (tuning knob bin_scatter = 1) the same partition without workgroup barriers in the main loop:
//                 persistent workgroups, one per CU, whose WAVEFRONTS run independently: a wavefront
//                 stages its own 64 x WC_L k-mer starts as codes in its corner of the LDS, every lane
//                 rolls its stream, and each probe record takes the next index L of its pair's run
//                 with one returning LDS atomic on {tail, heads} and goes to ring[slice][L % CAP].
//                 Ring slots carry a generation bit (bit 63 of the record = (L / CAP) & 1), so a
//                 slot's validity is visible in the slot itself.  The lane whose record completes a
//                 group of 8 (64 bytes, aligned in the run) keeps a note of it and, one round later -- when
//                 the other owners of the group's slots, wavefronts that took their indices earlier, have
//                 long filled them -- reads the group back (4 x ds_read_b128), checks the generation bits (a
//                 slot that is still missing makes the lane try again in the round after) and copies it to
//                 the run with four 16-byte stores into ONE 64-byte segment.  A ring
//                 of CAP = 16 is two halves of one group each with a head of its own (the number of groups
//                 that have left that half); a record whose half still holds the previous group waits in
//                 its lane.  Every wait is a bounded attempt inside ONE loop that services all pending
//                 records and groups of the wavefront, and no step depends on a group that is younger or in
//                 another half, so no wavefront ever blocks another (progress: the oldest group of a half that
//                 has not left can always be completed by the lanes that own its indices, and flushed).
//   longest[]     one word per slice, zeroed with the probe stage's control words before every record chunk: the drain of
//                 either partition kernel leaves the largest fill[] of the slice's runs there (one atomicMax per (slice,
//                 workgroup) pair).  It is where the probe stage's counter for the slice ends.
//   k_bin_probe   every XCD takes slices from a shared counter and probes its current slice step by step, 512 records
//                 of one run at a time, the run index fastest, up to the last step of the slice's longest run
//                 (nte_probe_draw.h): the slice's 2 MiB of filter (4 MiB parts of the slices of filters beyond 4 GiB)
//                 stay in that XCD's L2 (nte_kernels.hip).
//   k_ovf_probe   the overflow list, probed directly.
//
// Bit-exact by construction: the same hashes, the same records, only their order inside a slice
// differs, and the probe stage ORs bits.
#ifndef NTE_WC_TPB
#define NTE_WC_TPB 1024
#endif
#ifndef NTE_WC_L
#define NTE_WC_L 16
#endif
#ifndef NTE_WC_R
#define NTE_WC_R 1
#endif
#ifndef NTE_WC_CAP
#define NTE_WC_CAP 16
#endif
#ifndef NTE_WC_CARRY
#define NTE_WC_CARRY 2
#endif
constexpr int WC_TPB = NTE_WC_TPB;
constexpr int WC_WAVES = WC_TPB / 64;
constexpr int WC_L = NTE_WC_L;               // k-mer starts per lane per wavefront tile (multiple of 4)
constexpr int WC_R = NTE_WC_R;               // k-mer starts per lane per round (1, 2 or 4)
constexpr int WC_WTILE = 64 * WC_L;          // k-mer starts per wavefront tile
constexpr int WC_GROUP = 8;                  // records per flushed group (64 bytes)
constexpr int WC_CAP = NTE_WC_CAP;           // ring slots per slice (8 or 16)
constexpr int WC_CARRY = NTE_WC_CARRY;       // completed groups a lane can hold until its next round
constexpr int WC_MAX_SLICES = 1024;           // slices of k_wc_scatter and of k_wc_scatter_b with rings of WC_CAP slots
constexpr int WCB_WIDE_SLICES = 2048;         // slices of k_wc_scatter_b<.., WIDE>: rings of WCB_WIDE_CAP slots in the same LDS
constexpr int WCB_WIDE_CAP = 8;
constexpr u32 WCB_WIDE_MIN_RUN = 4096;        // records a (slice, workgroup) pair must expect for the host to cut a filter into more than WC_MAX_SLICES
constexpr u64 WC_EMPTY = WC_EMPTY_REC;       // never a record: the position bits of a record are never all ones
constexpr u64 WC_GEN = ~WC_REC_POS_MASK;     // generation bit of a ring slot; stays in the stored record
static_assert(WC_L % 4 == 0 && (WC_R == 1 || WC_R == 2 || WC_R == 4), "rounds work on 32-bit words of 4 codes");
static_assert(WC_CAP == 8 || WC_CAP == 16, "one or two groups per ring");
constexpr int WC_HALVES = WC_CAP / WC_GROUP;
constexpr u32 WC_MAX_RUN = (1u << 20) - 16;  // records per run: the 16-bit half heads must not wrap

struct WcOvf
{
	u64 rec;
	u32 bin;
	u32 pad;
};

// The overflow list is handed out in blocks: a wavefront owns the block [at, end) and takes a new one (ONE global atomic)
// when its records do not fit what is left, padding the rest with empty entries, so that every entry below the
// list's counter is either a record or empty.  (One atomic per record on ONE counter -- 270 M of them for the
// simple-sequence arrays of a 3 Gbp genome -- would serialise the partition kernel behind the L2.)
constexpr u32 WC_OVF_BLOCK = 256;
constexpr u32 WC_OVF_DEAD = 0xFFFFFFFFu; // the list was full when this wavefront asked: it stops asking (the chunk is lost anyway)
constexpr u32 WC_OVF_MAX_CAP = 0xF0000000u; // so that the 32-bit counter cannot wrap: every wavefront overshoots by one block at most
struct OvfCursor
{
	u32 at, end; // wavefront-uniform
};

// all lanes of the wavefront call this together; lanes with `put` append {rec, bin}
__device__ __forceinline__ void
ovf_push(WcOvf* __restrict__ ovf, u32* __restrict__ ovf_count, u32 ovf_cap, OvfCursor& cur, bool put, u64 rec, u32 bin)
{
	const u64 m = __ballot(put);
	if (m == 0 || cur.end == WC_OVF_DEAD) {
		return;
	}
	const u32 n = (u32)__popcll(m);
	const u32 lane = __lane_id();
	if (cur.at + n > cur.end) {
		const u32 rest = cur.end - cur.at; // < n <= 64
		if (lane < rest && cur.at + lane < ovf_cap) {
			WcOvf e;
			e.rec = WC_EMPTY_REC;
			e.bin = 0;
			e.pad = 0;
			ovf[cur.at + lane] = e;
		}
		u32 base = 0;
		if (lane == 0) {
			base = atomicAdd(ovf_count, WC_OVF_BLOCK);
		}
		base = (u32)__builtin_amdgcn_readfirstlane((int)base);
		if (base >= ovf_cap) {
			cur.at = cur.end = WC_OVF_DEAD;
			return;
		}
		cur.at = base;
		cur.end = base + WC_OVF_BLOCK;
	}
	if (put) {
		const u32 i = cur.at + (u32)__popcll(m & ((1ULL << lane) - 1));
		if (i < ovf_cap) {
			WcOvf v;
			v.rec = rec;
			v.bin = bin;
			v.pad = 0;
			ovf[i] = v;
		}
	}
	cur.at += n;
}

// end of the kernel: what is left of the wavefront's block becomes empty entries
__device__ __forceinline__ void
ovf_close(WcOvf* __restrict__ ovf, u32 ovf_cap, const OvfCursor& cur)
{
	if (cur.end == WC_OVF_DEAD) {
		return;
	}
	for (u32 i = cur.at + __lane_id(); i < cur.end; i += 64) {
		if (i < ovf_cap) {
			WcOvf e;
			e.rec = WC_EMPTY_REC;
			e.bin = 0;
			e.pad = 0;
			ovf[i] = e;
		}
	}
}

struct WcArgs
{
	BinArgs b;
	u32* fill;      // [n_slices][n_wg] records of the pair's run, padding of its last group included (multiple of 8)
	u32* longest;   // [n_slices] the largest fill[] of the slice (zeroed before the launch): where the probe stage's counter ends
	WcOvf* ovf;     // records of pairs whose run is full
	u32* ovf_count; // entries handed out, in blocks (may exceed ovf_cap: then records were lost, k_ovf_check)
	u32 ovf_cap;
	u32 n_wg;
	u32 cap;        // records per run (multiple of 8)
	u32 wcodes;     // LDS bytes of one wavefront's codes (wc_codes_bytes(k))
	u64 n_wtiles;   // wavefront tiles of the chunk
	u32* cand32;    // MODE 1 (the candidate map of -s 1, see k_wc_scatter_b): the map itself, for positions the records cannot serve
};

// codes of one wavefront tile: WC_WTILE + k - 1 of them (+ the word the last roll reads), padded rows (see k_screen)
inline size_t
wc_codes_bytes(u32 k)
{
	return (size_t)((WC_WTILE + k + 24 + 63) / 64) * 68 + 16;
}
constexpr size_t WC_LDS_RING = (size_t)WC_MAX_SLICES * WC_CAP * 8;
inline size_t
wc_lds_bytes(u32 k)
{
	return WC_LDS_RING + (size_t)WC_MAX_SLICES * 8 + (size_t)WC_WAVES * wc_codes_bytes(k) + (size_t)WC_WAVES * 32;
}

// orders this wavefront's LDS traffic (its LDS instructions execute in order; this keeps the compiler from
// moving them and makes the data of other lanes / wavefronts visible to the reads that follow)
__device__ __forceinline__ void
wave_lds_fence()
{
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template<int H, bool POW2>
__global__ __launch_bounds__(WC_TPB) void
k_wc_scatter(WcArgs a)
{
	constexpr int N = WC_R * H; // records per lane and round
	extern __shared__ __attribute__((aligned(16))) u8 s_dyn[];
	u64* s_ring = reinterpret_cast<u64*>(s_dyn);
	// per slice, one 64-bit word: low half = tail (index the next record of this pair gets), high half = two
	// 16-bit heads, one per ring half (groups of that half that have left; cap <= 2^20 keeps them from wrapping).
	// One returning 64-bit LDS atomic hands a record both.
	unsigned long long* s_state = reinterpret_cast<unsigned long long*>(s_dyn + WC_LDS_RING);
	u8* s_codes_all = reinterpret_cast<u8*>(s_state + WC_MAX_SLICES);
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	__shared__ u8 s_lut[256];

	const u32 tid = threadIdx.x;
	const u32 lane = tid & 63, wave = tid >> 6;
	const u32 nsl = a.b.n_slices;
	if (tid < TAB_WORDS) {
		s_tab[tid] = a.b.tabs[tid];
	}
	if (tid < 256) {
		s_lut[tid] = char_code((u8)tid);
	}
	for (u32 i = tid; i < nsl * WC_CAP; i += WC_TPB) {
		s_ring[i] = WC_EMPTY; // generation bit 1: never matches the first generation
	}
	for (u32 b = tid; b < nsl; b += WC_TPB) {
		s_state[b] = 0;
	}
	__syncthreads();

	u8* s_codes = s_codes_all + (size_t)wave * a.wcodes;
	const u32 k = a.b.p.k;
	const u32 ksh = (k & 3) * 8;
	const u32 slog = a.b.slice_log2;
	const u64 slice_mask = (1ULL << slog) - 1;
	const u32 cap = a.cap;
	const u32 n_wg = a.n_wg;
	u64* __restrict__ records = a.b.records;
	const u32 x0 = lane * WC_L;

	// groups completed by this lane's records that have not left yet: {slice, index of the completing record} as in pk[]
	// (never 0: that index is 7 mod 8)
	u32 cq[WC_CARRY];
#pragma unroll
	for (int q = 0; q < WC_CARRY; q++) {
		cq[q] = 0;
	}
	OvfCursor ovc = { 0, 0 };
	// the group that record `tok` completed: read it back, check that every slot carries this generation's bit (bit 31
	// of its high word), copy it to its run, give the ring half to the next generation.  false: a slot is not there yet.
	auto flush_group = [&](u32 tok) -> bool {
		const u32 b = tok >> 20, Lx = tok & 0xFFFFFu;
		const u32 g = Lx / WC_GROUP;
		const ulonglong2* src = reinterpret_cast<const ulonglong2*>(s_ring + (b * WC_CAP + (WC_HALVES == 2 ? (g & 1) * WC_GROUP : 0)));
		const ulonglong2 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
		const u32 e = (g / WC_HALVES) & 1 ? 0x80000000u : 0u;
		const u32 diff = ((u32)(v0.x >> 32) ^ e) | ((u32)(v0.y >> 32) ^ e) | ((u32)(v1.x >> 32) ^ e) | ((u32)(v1.y >> 32) ^ e) |
		                 ((u32)(v2.x >> 32) ^ e) | ((u32)(v2.y >> 32) ^ e) | ((u32)(v3.x >> 32) ^ e) | ((u32)(v3.y >> 32) ^ e);
		if (diff & 0x80000000u) {
			return false;
		}
		ulonglong2* dst = reinterpret_cast<ulonglong2*>(records + ((u64)(b * n_wg + blockIdx.x) * cap + (Lx & ~(u32)(WC_GROUP - 1))));
		dst[0] = v0;
		dst[1] = v1;
		dst[2] = v2;
		dst[3] = v3;
		atomicAdd(reinterpret_cast<u32*>(&s_state[b]) + 1, WC_HALVES == 2 && (g & 1) ? 0x10000u : 1u);
		return true;
	};

	for (u64 wt = (u64)blockIdx.x * WC_WAVES + wave; wt < a.n_wtiles; wt += (u64)n_wg * WC_WAVES) {
		const u64 tile_base = a.b.chunk_begin + wt * WC_WTILE;
		tile_stage(a.b.seq, a.b.n, tile_base, WC_WTILE + 8, k, s_lut, s_codes, lane, 64);
		wave_lds_fence();
		HashState hs = { 0, 0 };
		u32 good = 0;
		for (u32 i = 0; i < k; i++) {
			const u8 in = s_codes[tile_phys(x0 + i)];
			hash_roll(hs, s_tab, CODE_BAD, in);
			good = in == CODE_BAD ? 0 : good + 1;
		}
		u32 in_lo = *reinterpret_cast<const u32*>(&s_codes[tile_phys((x0 + k) & ~3u)]);
#pragma unroll 1
		for (u32 jw = 0; jw < WC_L; jw += 4) {
			const u32 outw = *reinterpret_cast<const u32*>(&s_codes[tile_phys(x0 + jw)]);
			const u32 in_hi = *reinterpret_cast<const u32*>(&s_codes[tile_phys(((x0 + jw + k) & ~3u) + 4)]);
			const u32 inw = ksh ? ((in_lo >> ksh) | (in_hi << (32 - ksh))) : in_lo;
			in_lo = in_hi;
#pragma unroll
			for (int part = 0; part < 4 / WC_R; part++) {
				// ---- the round's records
				u64 rec[N];
				u32 bin[N];
				u32 todo = 0; // bit x: record x still has to go into its ring
#pragma unroll
				for (int u = 0; u < WC_R; u++) {
					const int uu = part * WC_R + u;
					const u64 pos = tile_base + x0 + jw + uu;
					const bool have = good >= k && pos < a.b.chunk_end;
					const u64 base = hs.fh + hs.rh;
#pragma unroll
					for (int i = 0; i < H; i++) {
						const u64 hv = hash_extend(base, a.b.p, i);
						const u64 slot = POW2 ? (hv & a.b.f.mask) : filter_slot(a.b.f, hv);
						bin[u * H + i] = (u32)(slot >> slog);
						rec[u * H + i] = (pos << slog) | (slot & slice_mask);
						todo |= have ? 1u << (u * H + i) : 0u;
					}
					const u8 out = (outw >> (8 * uu)) & 0xFF;
					const u8 in = (inw >> (8 * uu)) & 0xFF;
					hash_roll(hs, s_tab, out, in);
					good = in == CODE_BAD ? 0 : good + 1;
				}
				// ---- groups that the previous round completed leave now: a hashing's worth of time later the other
				// owners of their slots (wavefronts that took their indices before the completing record took its own
				// and were between their atomic and their store) have filled them, and the ring half is free again
				// long before its next group needs it
#pragma unroll
				for (int q = 0; q < WC_CARRY; q++) {
					if (cq[q] != 0 && flush_group(cq[q])) {
						cq[q] = 0;
					}
				}
				// ---- indices: all cursor bumps in flight together.  Kept per record: {slice, index in the run} in one
				// word (the run holds < 2^20 records), and whether its ring half was free when the index was taken.
				u32 pk[N];
				u32 free0 = 0;
				u32 over = 0;
#pragma unroll
				for (int x = 0; x < N; x++) {
					unsigned long long st = 0;
					if ((todo >> x) & 1) {
						st = atomicAdd(&s_state[bin[x]], 1ULL);
					}
					const u32 Lx = (u32)st, h = (u32)(st >> 32);
					const u32 g = Lx / WC_GROUP; // group g lives in half g % HALVES as that half's generation g / HALVES
					const u32 hh = WC_HALVES == 2 ? (h >> (16 * (g & 1))) & 0xFFFFu : h & 0xFFFFu;
					free0 |= hh == ((g / WC_HALVES) & 0xFFFFu) ? 1u << x : 0u;
					over |= Lx >= cap ? 1u << x : 0u;
					pk[x] = (bin[x] << 20) | (Lx & 0xFFFFFu);
				}
				over &= todo;
				if (__any(over != 0)) {
					// the pair's run is full: these records go to the overflow list
#pragma unroll
					for (int x = 0; x < N; x++) {
						ovf_push(a.ovf, a.ovf_count, a.ovf_cap, ovc, (over >> x) & 1, rec[x], pk[x] >> 20);
					}
					todo &= ~over;
				}
				// ---- into the rings, right away: the time between taking an index and filling its slot is what
				// other wavefronts' group flushes may have to wait for
				u32 done = 0; // bit x: record x completed its group
#pragma unroll
				for (int x = 0; x < N; x++) {
					if ((todo >> x) & (free0 >> x) & 1) {
						const u32 b = pk[x] >> 20, Lx = pk[x] & 0xFFFFFu;
						const u64 gen = (Lx / WC_CAP) & 1 ? WC_GEN : 0;
						s_ring[b * WC_CAP + (Lx & (WC_CAP - 1))] = rec[x] | gen;
						done |= ((Lx + 1) & (WC_GROUP - 1)) == 0 ? 1u << x : 0u;
					}
				}
				todo &= ~free0;
				// ---- this round's completed groups wait in the lane for the next round
				u32 now = 0; // bit x: no room to wait: the group leaves in this round
#pragma unroll
				for (int x = 0; x < N; x++) {
					if ((done >> x) & 1) {
						bool put = false;
#pragma unroll
						for (int q = 0; q < WC_CARRY; q++) {
							if (!put && cq[q] == 0) {
								cq[q] = pk[x];
								put = true;
							}
						}
						now |= put ? 0u : 1u << x;
					}
				}
				// ---- the rare rest: records whose ring half still holds its previous group, groups with nowhere to wait.
				// Bounded attempts in one loop that also flushes what this wavefront carries (see the head of the file).
				for (u32 pass = 0; __any((todo | now) != 0); pass++) {
					__builtin_amdgcn_s_sleep(1);
					asm volatile("" ::: "memory"); // LDS is shared with wavefronts that do not synchronise with this one
					// (what this wavefront carries must leave too -- another wavefront may be waiting for it while this one
					// waits here -- but it need not be tried on every pass: the wait is usually over after one or two)
					if ((pass & 3) == 3) {
#pragma unroll
						for (int q = 0; q < WC_CARRY; q++) {
							if (cq[q] != 0 && flush_group(cq[q])) {
								cq[q] = 0;
							}
						}
					}
#pragma unroll
					for (int x = 0; x < N; x++) {
						const u32 b = pk[x] >> 20, Lx = pk[x] & 0xFFFFFu;
						if ((todo >> x) & 1) {
							const u32 g = Lx / WC_GROUP;
							const u32 h = __hip_atomic_load(reinterpret_cast<u32*>(&s_state[b]) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
							const u32 hh = WC_HALVES == 2 ? (h >> (16 * (g & 1))) & 0xFFFFu : h & 0xFFFFu;
							if (hh == ((g / WC_HALVES) & 0xFFFFu)) {
								const u64 gen = (Lx / WC_CAP) & 1 ? WC_GEN : 0;
								s_ring[b * WC_CAP + (Lx & (WC_CAP - 1))] = rec[x] | gen;
								todo &= ~(1u << x);
								if (((Lx + 1) & (WC_GROUP - 1)) == 0) {
									now |= 1u << x;
								}
							}
						}
						if (((now >> x) & 1) && flush_group(pk[x])) {
							now &= ~(1u << x);
						}
					}
				}
			}
		}
	}
	// what the lanes still carry
	for (;;) {
		u32 left = 0;
#pragma unroll
		for (int q = 0; q < WC_CARRY; q++) {
			if (cq[q] != 0 && flush_group(cq[q])) {
				cq[q] = 0;
			}
			left |= cq[q];
		}
		if (!__any(left != 0)) {
			break;
		}
		__builtin_amdgcn_s_sleep(2);
		asm volatile("" ::: "memory");
	}
	ovf_close(a.ovf, a.ovf_cap, ovc);
	__syncthreads();
	// ---- drain: the incomplete last group of every run, padded to 64 bytes with the empty record
	{
		const u32 j = tid & (WC_GROUP - 1);
		for (u32 b = tid / WC_GROUP; b < nsl; b += WC_TPB / WC_GROUP) {
			const unsigned long long st = s_state[b];
			u32 tl = (u32)st;
			tl = tl < cap ? tl : cap;
			const u32 hd = tl & ~(u32)(WC_GROUP - 1); // every complete group has left
			const u32 left = tl - hd;
			if (left) {
				const u32 i = hd + j;
				const u64 v = j < left ? s_ring[b * WC_CAP + (i & (WC_CAP - 1))] : WC_EMPTY;
				records[(u64)(b * n_wg + blockIdx.x) * cap + i] = v;
			}
			if (j == 0) {
				a.fill[(size_t)b * n_wg + blockIdx.x] = left ? hd + WC_GROUP : hd;
				atomicMax(&a.longest[b], left ? hd + WC_GROUP : hd);
			}
		}
	}
}

// ---- the barrier-phased variant of the partition kernel (round 2's, on this round's run layout) -----------------
// One workgroup per CU, rounds of ONE k-mer start per thread: phase A puts the round's records into the rings (cursor
// bumps first, all in flight together), the lane that fills the last slot of an 8-record group leaves a token; after an
// LDS-only barrier phase B copies the complete groups out, 8 lanes x 8 bytes = one coalesced 64-byte store per group.
// A slice that gets more than a ring-full in one round (low-complexity sequence) stores the excess directly.  The
// barriers make every slot of a group valid by construction: no generation bits, no waiting, no retries -- at the
// price of 16 wavefronts marching in step.  Same records, same runs, same fill[] as k_wc_scatter.
// WIDE: 2048 slices instead of 1024 in the same LDS (a 4 GiB filter in slices of 2 MiB, which leave half of an XCD's L2 to
// the record stream and the bitmap atomics): rings of 8 slots -- a slice's ninth record of a round is stored directly, as
// its seventeenth is otherwise -- and a 32-bit state word per slice (below).
constexpr int WCB_TPB = 1024;
constexpr int WCB_L = 32;                      // k-mer starts per thread per tile: one staging, one barrier, one prime of k rolls for 32 starts
constexpr int WCB_TILE = WCB_TPB * WCB_L;      // = TILE_PACKED_STARTS: the tile in the packed form (nte_tile.h), in the LDS of the byte tile
// k-mer starts per thread and round: two while the tokens of a round fit the LDS next to the rings (h <= 2; at h = 3 two per
// round were measured and lost: more of a ring's 16 slots arrive per round than leave)
#ifndef NTE_WCB_R3
#define NTE_WCB_R3 1
#endif
constexpr int
wcb_round(int h)
{
	return h <= 2 ? 2 : (h == 3 ? NTE_WCB_R3 : 1);
}
// tokens of a round: a group per 8 records on average (R x H <= 6: 768) + what the LDS has left -- with 2048 slices and
// h = 5 the groups that complete in one round are 640 +- 21
constexpr int WCB_MAX_TOKENS = WCB_TPB * 6 / WC_GROUP + 8 + 256;
static_assert(WCB_TILE == TILE_PACKED_STARTS && WCB_TILE % SCREEN_TILE == 0 && WCB_TILE % WC_WTILE == 0 && WCB_L % 8 == 0,
              "tiles of the two partition kernels and of the screening nest; a thread reads words of eight codes");
constexpr size_t WCB_LDS_BYTES = WC_LDS_RING + (size_t)WC_MAX_SLICES * 8 + (size_t)WCB_MAX_TOKENS * 4 + TILE_LDS_BYTES;
constexpr size_t WCB_LDS_STATIC = ((size_t)TAB_WORDS * 8 + 256 + 8 + 15) / 16 * 16; // s_tab, s_lut, s_ntok
static_assert((size_t)WCB_WIDE_SLICES * WCB_WIDE_CAP * 8 == WC_LDS_RING && (size_t)WCB_WIDE_SLICES * 4 == (size_t)WC_MAX_SLICES * 8,
              "the wide layout (8-slot rings, 32-bit state words) takes the LDS of the narrow one");
// (TILE_LDS_BYTES holds the codes of k = SCREEN_MAXK: the worst case is the only case)
static_assert(WCB_LDS_BYTES + WCB_LDS_STATIC + 1024 <= 160 * 1024, "k_wc_scatter_b: LDS of a CU, with 1 KiB to spare");
// a token: slice | first << IDX | index of the record that completed the group (< 2^IDX: the run limit), slice above
// them; first = first lane of the group whose record is still in the ring (the ones below were stored directly).
// IDX = 19 with 10 slice bits, 18 with the 11 of the wide layout.
constexpr u32
wcb_idx_bits(bool wide)
{
	return wide ? 18u : 19u;
}
constexpr u32 WCB_MAX_RUN = (1u << wcb_idx_bits(false)) - 16;
constexpr u32 WCB_WIDE_MAX_RUN = (1u << wcb_idx_bits(true)) - 16;
static_assert(10 + 3 + wcb_idx_bits(false) <= 32 && 11 + 3 + wcb_idx_bits(true) <= 32 && WC_MAX_SLICES <= 1 << 10 && WCB_WIDE_SLICES <= 1 << 11,
              "a token is one 32-bit word");
// The wide layout's state word: tail in the low WCB_TAIL_BITS, head modulo 2^WCB_HEAD_BITS above it (a carry out of bit
// 31 is lost, harmlessly).  A lane that draws an index >= cap takes its increment back, so the tail never passes cap + the
// records of one round, however often a draft repeats a k-mer; the head trails the tail by at most a round's records + a
// ring, so the tail and the head's low bits give the whole head.
constexpr u32 WCB_TAIL_BITS = 19, WCB_HEAD_BITS = 32 - WCB_TAIL_BITS;
constexpr u32 WCB_TAIL_MASK = (1u << WCB_TAIL_BITS) - 1, WCB_HEAD_MASK = (1u << WCB_HEAD_BITS) - 1;
static_assert(WCB_WIDE_MAX_RUN + WCB_TPB * 6 < (1u << WCB_TAIL_BITS), "tail: a full run and one round of over-draws");
static_assert(WCB_TPB * 6 + WCB_WIDE_CAP + WC_GROUP < (1u << WCB_HEAD_BITS), "head: tail - head within the modulus");

// MODE 1 (round 6; -s 1 on a plain filter): instead of the H probes of every k-mer, the FIRST probe of the k-mers that the
// three substitution candidates of a position make of it (the k-mer with its last base replaced, ntedit.cpp:1916-1934;
// candidate order of polish_bases_array / snv_bases_array :180-199) -- the gate of k_assess asks for them at EVERY
// position of a draft, 3 random gathers per position, 4 in 5 of which find a zero bit.  Partitioned and probed like the
// screening's (record position = 4 * position + candidate, the probe stage ORs the bits that ARE set into the
// candidate map), they cost an eighth of that; k_assess then probes on from the second hash for the candidates
// that are left.  H = 3 records per position; positions whose last base is no A/C/G/T get all four bits (unknown).
template<int H, bool POW2, int MODE = 0, bool WIDE = false>
__global__ __launch_bounds__(WCB_TPB) void
k_wc_scatter_b(WcArgs a)
{
	static_assert(MODE == 0 || H == 3, "the candidate map: three candidates per position");
	constexpr int R = wcb_round(H); // k-mer starts per thread and round
	constexpr int N = R * H;        // records per thread and round
	constexpr int CAP = WIDE ? WCB_WIDE_CAP : WC_CAP; // ring slots per slice
	constexpr u32 IDX = wcb_idx_bits(WIDE);           // index bits of a token
	extern __shared__ __attribute__((aligned(16))) u8 s_dyn[];
	u64* s_ring = reinterpret_cast<u64*>(s_dyn);
	// per slice, one 64-bit word: low half = tail (index the next record of this pair gets), high half = head
	// (records of the run that are in memory).  One returning 64-bit LDS atomic hands a record both.
	// WIDE: one 32-bit word, {head modulo 2^13, tail} (WCB_TAIL_BITS above), in the same place.
	unsigned long long* s_state = reinterpret_cast<unsigned long long*>(s_dyn + WC_LDS_RING);
	u32* s_state32 = reinterpret_cast<u32*>(s_dyn + WC_LDS_RING);
	u32* s_tok = reinterpret_cast<u32*>(s_state + WC_MAX_SLICES);
	u8* s_codes = reinterpret_cast<u8*>(s_tok + WCB_MAX_TOKENS);
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	__shared__ u8 s_lut[256];
	__shared__ u32 s_ntok[2];

	const u32 tid = threadIdx.x;
	const u32 nsl = a.b.n_slices;
	if (tid < TAB_WORDS) {
		s_tab[tid] = a.b.tabs[tid];
	}
	if (tid < 256) {
		s_lut[tid] = char_code((u8)tid);
	}
	if (tid < 2) {
		s_ntok[tid] = 0;
	}
	for (u32 b = tid; b < nsl; b += WCB_TPB) {
		if (WIDE) {
			s_state32[b] = 0;
		} else {
			s_state[b] = 0;
		}
	}
	__syncthreads();

	const u32 k = a.b.p.k;
	const u32 slog = a.b.slice_log2;
	const u64 slice_mask = (1ULL << slog) - 1;
	const u32 cap = a.cap;
	const u32 n_wg = a.n_wg;
	u64* __restrict__ records = a.b.records;
	const u64 n_tiles = (a.n_wtiles * WC_WTILE + WCB_TILE - 1) / WCB_TILE;
	u32 round = 0;
	OvfCursor ovc = { 0, 0 };
	for (u64 tile = blockIdx.x; tile < n_tiles; tile += n_wg) {
		const u64 tile_base = a.b.chunk_begin + tile * WCB_TILE;
		// (positions at or beyond chunk_end are staged -- a chunk is whole SCREEN_TILEs, half of this tile -- and never emitted)
		tile_stage_packed(a.b.seq, a.b.n, tile_base, WCB_TILE + 8, k, s_lut, s_codes, tid, WCB_TPB);
		__syncthreads();
		const u32 x0 = tid * WCB_L;
		HashState hs = { 0, 0 };
		u32 good = 0;
		u32 last_code = CODE_BAD; // (MODE 1) the last base of the k-mer under the cursor
		for (u32 i = 0; i < k; i += 8) {
			const u32 w8 = tile_packed_word(s_codes, x0 + i);
#pragma unroll
			for (u32 b = 0; b < 8; b++) {
				if (i + b < k) {
					const u8 in = (w8 >> (4 * b)) & 15u;
					hash_roll(hs, s_tab, CODE_BAD, in);
					good = in == CODE_BAD ? 0 : good + 1;
					last_code = in;
				}
			}
		}
		// (codes are read as words of eight, TileOct's way: one LDS read per eight k-mer starts for each of the two streams)
		const u32 ksh = (k & 7) * 4;
		u32 in_lo = tile_packed_word(s_codes, (x0 + k) & ~7u);
		u32 outw = 0, inw = 0;
		for (u32 j0 = 0; j0 < WCB_L; j0 += R, round++) {
			if ((j0 & 7u) == 0) {
				outw = tile_packed_word(s_codes, x0 + j0);
				const u32 in_hi = tile_packed_word(s_codes, ((x0 + j0 + k) & ~7u) + 8);
				inw = ksh ? ((in_lo >> ksh) | (in_hi << (32 - ksh))) : in_lo;
				in_lo = in_hi;
			}
			// ---- phase A: records into the rings
			u64 rec[N];
			u32 bin[N];
			bool have0[R];
#pragma unroll
			for (int u = 0; u < R; u++) {
				const u64 pos = tile_base + x0 + j0 + u;
				have0[u] = good >= k && pos < a.b.chunk_end;
				if (MODE == 0) {
					const u64 base = hs.fh + hs.rh;
#pragma unroll
					for (int i = 0; i < H; i++) {
						const u64 hv = hash_extend(base, a.b.p, i);
						const u64 slot = POW2 ? (hv & a.b.f.mask) : filter_slot(a.b.f, hv);
						bin[u * H + i] = (u32)(slot >> slog);
						rec[u * H + i] = (pos << slog) | (slot & slice_mask);
					}
				} else {
					// candidates of draft base A: T C G, C: A T G, G: A T C, T: A C G (codes A C G T = 0 1 2 3), one byte per base
					const u32 d = last_code;
					if (have0[u] && d > 3u) {
						atomicOr(&a.cand32[pos >> 3], 0xFu << (4 * (pos & 7))); // (an IUPAC code: k_assess asks everything itself)
					}
					have0[u] = have0[u] && d <= 3u;
					const u32 row = d == 0 ? 0x020103u : d == 1 ? 0x020300u : d == 2 ? 0x010300u : 0x020100u;
#pragma unroll
					for (int i = 0; i < H; i++) {
						HashState t = hs;
						hash_changelast(t, s_tab, (u8)(d & 3u), (u8)((row >> (8 * i)) & 3u));
						const u64 hv = hash_extend(t.fh + t.rh, a.b.p, 0);
						const u64 slot = POW2 ? (hv & a.b.f.mask) : filter_slot(a.b.f, hv);
						bin[u * H + i] = (u32)(slot >> slog);
						rec[u * H + i] = ((pos * 4 + (u64)i) << slog) | (slot & slice_mask);
					}
				}
				const u32 sh = 4 * ((j0 + u) & 7u);
				const u8 out = (outw >> sh) & 15u;
				const u8 in = (inw >> sh) & 15u;
				hash_roll(hs, s_tab, out, in);
				good = in == CODE_BAD ? 0 : good + 1;
				last_code = in;
			}
			u32 G[N], hd[N];
			bool have[N];
#pragma unroll
			for (int x = 0; x < N; x++) {
				if (WIDE) {
					const u32 st = have0[x / H] ? atomicAdd(&s_state32[bin[x]], 1u) : 0u;
					G[x] = st & WCB_TAIL_MASK;
					hd[x] = G[x] - ((G[x] - (st >> WCB_TAIL_BITS)) & WCB_HEAD_MASK);
				} else {
					const unsigned long long st = have0[x / H] ? atomicAdd(&s_state[bin[x]], 1ULL) : 0ULL;
					G[x] = (u32)st;
					hd[x] = (u32)(st >> 32);
				}
				have[x] = have0[x / H] && G[x] < cap;
			}
			{
				// pairs whose run is full: to the overflow list
				bool over[N];
				bool any_over = false;
#pragma unroll
				for (int x = 0; x < N; x++) {
					over[x] = have0[x / H] && G[x] >= cap;
					any_over |= over[x];
					if (WIDE && over[x]) {
						atomicSub(&s_state32[bin[x]], 1u); // (the tail stays at cap + what is being drawn right now)
					}
				}
				if (__any(any_over)) {
#pragma unroll
					for (int x = 0; x < N; x++) {
						ovf_push(a.ovf, a.ovf_count, a.ovf_cap, ovc, over[x], rec[x], bin[x]);
					}
				}
			}
			u32 dend[N]; // 1: the record was stored directly
			u64 tokm[N]; // lanes whose record filled the last slot of a group
			u32 n_tok = 0;
#pragma unroll
			for (int x = 0; x < N; x++) {
				dend[x] = 0;
				const u32 lim = (hd[x] & ~(u32)(WC_GROUP - 1)) + CAP;
				const bool in_ring = have[x] && G[x] < lim;
				u64* run = records + (u64)(bin[x] * n_wg + blockIdx.x) * cap;
				if (in_ring) {
					s_ring[(size_t)bin[x] * CAP + (G[x] & (CAP - 1))] = rec[x];
				} else if (have[x]) {
					// more than a ring-full for this slice in one round: straight to memory
					run[G[x]] = rec[x];
					dend[x] = 1;
				}
				tokm[x] = __ballot(in_ring && ((G[x] + 1) & (WC_GROUP - 1)) == 0);
				n_tok += (u32)__popcll(tokm[x]);
			}
			if (n_tok) {
				// one bump of the token counter per wavefront and round
				const u32 lane_id = __lane_id();
				u32 base_idx = 0;
				if (lane_id == 0) {
					base_idx = atomicAdd(&s_ntok[round & 1], n_tok);
				}
				base_idx = __shfl(base_idx, 0, 64);
#pragma unroll
				for (int x = 0; x < N; x++) {
					if ((tokm[x] >> lane_id) & 1) {
						const u32 g0 = G[x] + 1 - WC_GROUP;
						const u32 first = hd[x] > g0 ? hd[x] - g0 : 0;
						s_tok[base_idx + (u32)__popcll(tokm[x] & ((1ULL << lane_id) - 1))] = (bin[x] << (IDX + 3)) | (first << IDX) | G[x];
					}
					base_idx += (u32)__popcll(tokm[x]);
				}
			}
			lds_barrier();
			// ---- phase B: complete groups out, one coalesced 64-byte store per group
			if (tid == 0) {
				s_ntok[(round + 1) & 1] = 0;
			}
			const u32 nt = s_ntok[round & 1];
			const u32 lane = tid & (WC_GROUP - 1);
			for (u32 w = tid / WC_GROUP; w < nt; w += WCB_TPB / WC_GROUP) {
				const u32 t = s_tok[w];
				const u32 tb = t >> (IDX + 3), first = (t >> IDX) & 7u;
				const u32 Gi = ((t & ((1u << IDX) - 1u)) & ~(u32)(WC_GROUP - 1)) + lane;
				if (lane >= first) {
					records[(u64)(tb * n_wg + blockIdx.x) * cap + Gi] = s_ring[(size_t)tb * CAP + (Gi & (CAP - 1))];
				}
				if (lane == 0) {
					if (WIDE) {
						atomicAdd(&s_state32[tb], (u32)(WC_GROUP - first) << WCB_TAIL_BITS);
					} else {
						atomicAdd(&s_state[tb], (unsigned long long)(WC_GROUP - first) << 32);
					}
				}
			}
#pragma unroll
			for (int x = 0; x < N; x++) {
				if (dend[x]) {
					if (WIDE) {
						atomicAdd(&s_state32[bin[x]], 1u << WCB_TAIL_BITS);
					} else {
						atomicAdd(&s_state[bin[x]], 1ULL << 32);
					}
				}
			}
			lds_barrier();
		}
	}
	ovf_close(a.ovf, a.ovf_cap, ovc);
	// ---- drain: what is left in the rings (records [head, tail) of every run; at most CAP of them), the last group
	// padded to 64 bytes with the empty record
	{
		const u32 j = tid & (WC_GROUP - 1);
		for (u32 b = tid / WC_GROUP; b < nsl; b += WCB_TPB / WC_GROUP) {
			u32 tl, hdm; // tail; head: everything below is in memory
			if (WIDE) {
				const u32 st = s_state32[b];
				tl = st & WCB_TAIL_MASK; // (every over-draw has been taken back: <= cap)
				hdm = tl - ((tl - (st >> WCB_TAIL_BITS)) & WCB_HEAD_MASK);
			} else {
				const unsigned long long st = s_state[b];
				tl = (u32)st;
				hdm = (u32)(st >> 32);
			}
			tl = tl < cap ? tl : cap;
			u64* run = records + (u64)(b * n_wg + blockIdx.x) * cap;
			const u32 g0 = hdm & ~(u32)(WC_GROUP - 1);
#pragma unroll
			for (int g = 0; g < CAP / WC_GROUP + 1; g++) {
				const u32 i = g0 + g * WC_GROUP + j;
				if (i >= hdm && i < tl) {
					run[i] = s_ring[(size_t)b * CAP + (i & (CAP - 1))];
				}
			}
			const u32 end = (tl + WC_GROUP - 1) & ~(u32)(WC_GROUP - 1);
			if (tl + j < end) {
				run[tl + j] = WC_EMPTY;
			}
			if (j == 0) {
				a.fill[(size_t)b * n_wg + blockIdx.x] = end;
				atomicMax(&a.longest[b], end);
			}
		}
	}
}

// the overflow list: direct probes (repetitive sequence: its few distinct k-mers keep hitting the same filter lines)
__global__ __launch_bounds__(256) void
k_ovf_probe(const u8* __restrict__ filter, const WcOvf* __restrict__ ovf, const u32* __restrict__ ovf_count, u32 ovf_cap, u32 slog, u32* __restrict__ absent32,
            u32 counting, u32 count_lo, u32 mark_present)
{
	u32 n = *ovf_count;
	n = n < ovf_cap ? n : ovf_cap;
	const u64 off_mask = (1ULL << slog) - 1;
	for (u32 i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
		const WcOvf v = ovf[i];
		if (v.rec == WC_EMPTY_REC) {
			continue; // (padding of a wavefront's block)
		}
		const u64 off = ((u64)v.bin << slog) | (v.rec & off_mask);
		const bool absent = counting ? (u32)filter[off] < count_lo : !((filter[off >> 3] >> (off & 7)) & 1);
		if (absent != (mark_present != 0)) { // (the candidate map marks the bits that are SET)
			const u64 pos = (v.rec & WC_REC_POS_MASK) >> slog;
			atomicOr(&absent32[pos >> 5], 1u << (pos & 31));
		}
	}
}

// more overflow entries than the list holds: probes of this record chunk were lost, its part of the bitmap is void and
// the host screens it again with the direct kernel before anything reads it (bin_recover).  state[0..1] = entries handed
// out over all chunks since the last reset (a statistic), state[BIN_LOST_FLAGS + chunk] = this chunk's flag.
constexpr u32 BIN_LOST_FLAGS = 4;
__global__ void
k_ovf_check(const u32* __restrict__ ovf_count, u32 ovf_cap, u32* __restrict__ state, u32 chunk)
{
	const u32 n = *ovf_count;
	*reinterpret_cast<unsigned long long*>(state) += n;
	state[BIN_LOST_FLAGS + chunk] = n > ovf_cap ? 1u : 0u;
}
