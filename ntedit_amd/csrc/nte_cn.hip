// nte_cn.hip -- the k-mer spectrum split by assembly copy number: the draft store, the two passes and their driver
// (nte_cn.h has the definitions).
//
//   k_cn_count<H>             pass 1 over one stored batch: every k-mer adds 1, saturating at 255, to its H counters of
//                             the copy-number sketch (k_count's store rule, nte_reads.hip)
//   k_cn_nonzero              the sketch's non-zero counters (k_nonzero's form)
//   k_spectrum_cn<H, POW2>    pass 2: per k-mer H gathers into the counting filter (the multiplicity m) and H into the
//                             sketch (the copy number cn); occ[min(cn, 5)][m], w5[m] and the entry's row
//
// The tile, its staging, the walk and the entry cursor are nte_tile.h's, as k_spectrum's are.
#include "nte_cn.h"
#include "nte_tile.h"

#include "../../include/ntedit_hip.h"

namespace nte {

namespace {

constexpr int CN_WAVES = TILE_TPB / 64;
static_assert(CN_MAXK <= TILE_MAXK, "the tile's halo holds the unit's largest k");

// seed tables and the look-up table into LDS, then the tile's codes: CODE_BAD for every byte that is not one of ACGTacgt
// and for every position past n
__device__ __forceinline__ void
cn_stage(const u8* __restrict__ seq, u64 n, u32 k, const u64* __restrict__ tabs, u64* s_tab, u8* s_lut, u8* s_codes)
{
	const u32 tid = threadIdx.x;
	tile_load_tabs(tabs, s_tab, tid);
	tile_fill_lut(s_lut, true, tid);
	__syncthreads();
	tile_stage(seq, n, (u64)blockIdx.x * TILE_STARTS, TILE_STARTS, k, s_lut, s_codes, tid, TILE_TPB);
	__syncthreads();
}

// ------------------------------------------------------------------ k_cn_count
// One thread walks 64 consecutive starts; a start is a k-mer when k good codes have entered and the window lies inside
// the entry of its position (k_spectrum's bounds: entries may abut, a window never spans two).  Each k-mer adds 1 to its
// H counters by k_count's store rule (byte_sat_inc).
template<int H>
__global__ __launch_bounds__(TILE_TPB) void
k_cn_count(const u8* __restrict__ seq, u64 n, DevParams p, const u64* __restrict__ tabs, const u64* __restrict__ offs,
           const u32* __restrict__ lens, u32 n_entries, u32* __restrict__ sketch, u64 smask)
{
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	__shared__ u8 s_lut[256];
	__shared__ __attribute__((aligned(16))) u8 s_codes[TILE_LDS_BYTES];
	const u32 k = p.k;
	cn_stage(seq, n, k, tabs, s_tab, s_lut, s_codes);

	const u32 x0 = threadIdx.x * TILE_L;
	TileWalk walk;
	walk.prime(s_codes, s_tab, x0, k);
	const u64 pos0 = (u64)blockIdx.x * TILE_STARTS + x0;
	EntryCursor cur;
	cur.start(offs, lens, n_entries, pos0);
	for (u32 j = 0; j < TILE_L; j++) {
		const u64 pos = pos0 + j;
		cur.advance(offs, lens, n_entries, pos);
		if (walk.valid() && cur.holds(pos, k)) {
			const u64 base = walk.base();
#pragma unroll
			for (int i = 0; i < H; i++) {
				byte_sat_inc(sketch, hash_extend(base, p, i) & smask);
			}
		}
		walk.roll_bytes(s_codes, s_tab, j);
	}
}

// non-zero bytes of an array of n_words 64-bit words
__global__ __launch_bounds__(256) void
k_cn_nonzero(const u64* __restrict__ w, u64 n_words, unsigned long long* total)
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
	if (threadIdx.x == 0 && s_sum[0]) {
		atomicAdd(total, s_sum[0]);
	}
}

// ------------------------------------------------------------------ k_spectrum_cn
// k_spectrum with a second gather target.  Four starts per iteration: the H hash values of a start are computed once and
// give H slots of the filter (POW2 or not: the filter's) and H of the sketch (always a mask); all 4 x 2H gathers are issued
// before the first is used, a start that is no k-mer reads byte 0 of both instead of branching, and no probe ends early.
// LDS: one u32 [5][256] histogram per wavefront (20 KiB per workgroup; a tile has 16,384 starts, so a bin cannot
// overflow), one u64 [256] per workgroup for w5 (64-bit LDS atomics; class 5 is rare outside satellites), the
// reciprocals of 5 .. 255 as u32 (RECIP[5] < 2^30).  Non-zero bins are flushed with one 64-bit global atomic each.
// The rows follow k_spectrum's scheme with six fields: what belongs to the entry the tile begins in is reduced over the
// workgroup into one atomic per field, every other entry begins inside the tile and takes the atomics of the threads
// that met it.  The class counters of a thread are five named sums updated by comparison, never an array indexed by
// the class: that would live in scratch.
template<int H, bool POW2>
__global__ __launch_bounds__(TILE_TPB) void
k_spectrum_cn(const u8* __restrict__ seq, u64 n, Filter f, DevParams p, const u64* __restrict__ tabs, const u64* __restrict__ offs,
              const u32* __restrict__ lens, u32 n_entries, const u8* __restrict__ sketch, u64 smask,
              unsigned long long* __restrict__ occ,  // [5][256]
              unsigned long long* __restrict__ w5,   // [256]
              unsigned long long* __restrict__ rows) // [n_entries][6]
{
	__shared__ __attribute__((aligned(16))) u64 s_tab[TAB_WORDS];
	__shared__ u8 s_lut[256];
	__shared__ __attribute__((aligned(16))) u8 s_codes[TILE_LDS_BYTES];
	__shared__ u32 s_hist[CN_WAVES][CN_CLASSES * CN_BINS];
	__shared__ unsigned long long s_w5[CN_BINS];
	__shared__ u32 s_recip[CN_BINS];
	__shared__ u32 s_row[CN_CLASSES];

	const u32 tid = threadIdx.x;
#pragma unroll
	for (int w = 0; w < CN_WAVES; w++) {
#pragma unroll
		for (int c = 0; c < CN_CLASSES; c++) {
			s_hist[w][c * CN_BINS + tid] = 0;
		}
	}
	s_w5[tid] = 0;
	s_recip[tid] = tid >= 5 ? (u32)(((1ull << 32) + tid / 2) / tid) : 0;
	if (tid < CN_CLASSES) {
		s_row[tid] = 0;
	}
	const u32 k = p.k;
	cn_stage(seq, n, k, tabs, s_tab, s_lut, s_codes); // (its barriers order the zeroing before any add)

	const u64 tile_base = (u64)blockIdx.x * TILE_STARTS;
	const u32 x0 = tid * TILE_L;
	TileWalk walk;
	walk.prime(s_codes, s_tab, x0, k);

	// the entry of the stream's position
	const u64 pos0 = tile_base + x0;
	const u32 e_tile = entry_behind(offs, lens, n_entries, tile_base);
	EntryCursor cur;
	cur.start(offs, lens, n_entries, pos0);
	// the row of the entry the thread is counting (e_acc), and what it has counted of the tile's own entry
	u32 e_acc = cur.e, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0;
	u32 t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
	auto flush = [&]() {
		const u32 all = a1 + a2 + a3 + a4 + a5;
		if (all) {
			if (e_acc == e_tile) {
				t1 += a1;
				t2 += a2;
				t3 += a3;
				t4 += a4;
				t5 += a5;
			} else {
				unsigned long long* r = rows + (u64)e_acc * CN_ROW_WORDS;
				atomicAdd(r, (unsigned long long)all);
				if (a1) {
					atomicAdd(r + 1, (unsigned long long)a1);
				}
				if (a2) {
					atomicAdd(r + 2, (unsigned long long)a2);
				}
				if (a3) {
					atomicAdd(r + 3, (unsigned long long)a3);
				}
				if (a4) {
					atomicAdd(r + 4, (unsigned long long)a4);
				}
				if (a5) {
					atomicAdd(r + 5, (unsigned long long)a5);
				}
			}
		}
		a1 = a2 = a3 = a4 = a5 = 0;
	};

	u32* hist = s_hist[tid >> 6];
	TileQuad quad;
	quad.begin(s_codes, walk);
	for (u32 j0 = 0; j0 < TILE_L; j0 += 4) {
		u32 outw, inw;
		quad.read(s_codes, walk, j0, outw, inw);

		u64 fslot[4][H], sslot[4][H];
		bool valid[4];
		u32 ent[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const u64 pos = pos0 + j0 + u;
			cur.advance(offs, lens, n_entries, pos);
			valid[u] = walk.valid() && cur.holds(pos, k);
			ent[u] = cur.e;
			const u64 base = walk.base();
#pragma unroll
			for (int i = 0; i < H; i++) {
				const u64 hv = hash_extend(base, p, i);
				fslot[u][i] = POW2 ? (hv & f.mask) : filter_slot(f, hv);
				sslot[u][i] = hv & smask;
			}
			walk.roll_quad(s_tab, outw, inw, u);
		}
		u8 fb[4][H], sb[4][H];
#pragma unroll
		for (int u = 0; u < 4; u++) {
#pragma unroll
			for (int i = 0; i < H; i++) {
				fb[u][i] = f.data[valid[u] ? fslot[u][i] : 0];
				sb[u][i] = sketch[valid[u] ? sslot[u][i] : 0];
			}
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			u32 m = 255, cn = 255;
#pragma unroll
			for (int i = 0; i < H; i++) {
				m = fb[u][i] < m ? fb[u][i] : m;
				cn = sb[u][i] < cn ? sb[u][i] : cn;
			}
			if (valid[u]) {
				// (pass 1 counted this very occurrence: cn >= 1; a sketch that was not counted must not index below the histogram)
				const u32 cls = cn < 5 ? (cn ? cn : 1) : 5;
				atomicAdd(&hist[(cls - 1) * CN_BINS + m], 1u);
				if (cls == 5) {
					atomicAdd(&s_w5[m], (unsigned long long)s_recip[cn]);
				}
				if (ent[u] != e_acc) {
					flush();
					e_acc = ent[u];
				}
				a1 += cls == 1;
				a2 += cls == 2;
				a3 += cls == 3;
				a4 += cls == 4;
				a5 += cls == 5;
			}
		}
	}
	flush();
	for (int o = 32; o > 0; o >>= 1) {
		t1 += __shfl_down(t1, o);
		t2 += __shfl_down(t2, o);
		t3 += __shfl_down(t3, o);
		t4 += __shfl_down(t4, o);
		t5 += __shfl_down(t5, o);
	}
	if ((tid & 63) == 0 && (t1 | t2 | t3 | t4 | t5)) {
		atomicAdd(&s_row[0], t1);
		atomicAdd(&s_row[1], t2);
		atomicAdd(&s_row[2], t3);
		atomicAdd(&s_row[3], t4);
		atomicAdd(&s_row[4], t5);
	}
	__syncthreads();
	static_assert(TILE_TPB == CN_BINS, "one thread per multiplicity flushes");
#pragma unroll
	for (int c = 0; c < CN_CLASSES; c++) {
		u32 total = 0;
#pragma unroll
		for (int w = 0; w < CN_WAVES; w++) {
			total += s_hist[w][c * CN_BINS + tid];
		}
		if (total) {
			atomicAdd(occ + c * CN_BINS + tid, (unsigned long long)total);
		}
	}
	if (s_w5[tid]) {
		atomicAdd(w5 + tid, s_w5[tid]);
	}
	if (e_tile < n_entries) {
		if (tid < CN_CLASSES && s_row[tid]) {
			atomicAdd(rows + (u64)e_tile * CN_ROW_WORDS + 1 + tid, (unsigned long long)s_row[tid]);
		}
		if (tid == CN_CLASSES) {
			const u32 all = s_row[0] + s_row[1] + s_row[2] + s_row[3] + s_row[4];
			if (all) {
				atomicAdd(rows + (u64)e_tile * CN_ROW_WORDS, (unsigned long long)all);
			}
		}
	}
}

// ------------------------------------------------------------------ host side
int
cn_fail(std::string* why, int code, const char* what, hipError_t he)
{
	if (why) {
		*why = std::string(what) + ": " + hipGetErrorString(he);
	}
	return code;
}

#define CN_TRY(expr, what)                                      \
	do {                                                        \
		const hipError_t he_ = (expr);                          \
		if (he_ != hipSuccess) {                                \
			return cn_fail(why, NTEDIT_E_DEVICE, what, he_);    \
		}                                                       \
	} while (0)

void
cn_release_batches(CnStore& st)
{
	for (auto& side : st.side) {
		for (CnBatch& b : side) {
			(void)hipFree(b.bases);
			(void)hipFree(b.offs);
			(void)hipFree(b.lens);
		}
		side.clear();
	}
	st.bytes[0] = st.bytes[1] = 0;
	st.entries[0] = st.entries[1] = 0;
}

void
cn_clear_results(CnStore& st)
{
	st.finished = false;
	st.counters = 0;
	st.nonzero[0] = st.nonzero[1] = 0;
	for (float& m : st.ms) {
		m = 0.f;
	}
	for (int w = 0; w < 2; w++) {
		st.table[w].clear();
		st.rows[w].clear();
	}
}

template<int H>
void
cn_launch_count(dim3 grid, hipStream_t s, const CnBatch& b, const DevParams& p, const u64* d_tab, u32* sketch, u64 smask)
{
	hipLaunchKernelGGL((k_cn_count<H>), grid, dim3(TILE_TPB), 0, s, b.bases, b.n, p, d_tab, b.offs, b.lens, b.n_entries, sketch, smask);
}

template<int H>
void
cn_launch_spectrum(dim3 grid, hipStream_t s, const CnBatch& b, const Filter& f, const DevParams& p, const u64* d_tab, const u8* sketch, u64 smask,
                   unsigned long long* occ, unsigned long long* w5, unsigned long long* rows)
{
	if (f.mask) {
		hipLaunchKernelGGL((k_spectrum_cn<H, true>), grid, dim3(TILE_TPB), 0, s, b.bases, b.n, f, p, d_tab, b.offs, b.lens, b.n_entries, sketch, smask, occ, w5, rows);
	} else {
		hipLaunchKernelGGL((k_spectrum_cn<H, false>), grid, dim3(TILE_TPB), 0, s, b.bases, b.n, f, p, d_tab, b.offs, b.lens, b.n_entries, sketch, smask, occ, w5, rows);
	}
}

} // namespace

void
cn_switch(CnStore& st, bool on, u64 cap_bytes)
{
	cn_release_batches(st);
	cn_clear_results(st);
	st.state = on ? CN_ON : CN_OFF;
	st.cap = on ? cap_bytes : 0;
}

void
cn_reset(CnStore& st)
{
	cn_release_batches(st);
	cn_clear_results(st);
	if (st.state != CN_OFF) {
		st.state = CN_ON;
	}
}

void
cn_free(CnStore& st)
{
	cn_release_batches(st);
	cn_clear_results(st);
	(void)hipFree(st.sketch);
	(void)hipFree(st.d_out);
	st.sketch = nullptr;
	st.sketch_bytes = 0;
	st.d_out = nullptr;
	st.d_out_words = 0;
	for (auto& e : st.evt) {
		if (e) {
			(void)hipEventDestroy(e);
			e = nullptr;
		}
	}
	if (st.state != CN_OFF) {
		st.state = CN_ON;
	}
}

int
cn_append(CnStore& st, int which, hipStream_t stream, const void* bases, u64 n, const u64* offs, const u32* lens, u32 n_entries, std::string* why)
{
	if (st.state != CN_ON || n_entries == 0) {
		return 0; // (released earlier in the round: the rest of the round is not kept either)
	}
	st.finished = false;
	if (n > st.cap || st.bytes[0] + st.bytes[1] > st.cap - n) {
		cn_release_batches(st);
		st.state = CN_OVER_CAP;
		return 0;
	}
	CnBatch b;
	b.n = n;
	b.n_entries = n_entries;
	hipError_t he = n ? hipMalloc((void**)&b.bases, (size_t)((n + 15) / 16 * 16)) : hipSuccess;
	if (he == hipSuccess) {
		he = hipMalloc((void**)&b.offs, (size_t)n_entries * 8);
	}
	if (he == hipSuccess) {
		he = hipMalloc((void**)&b.lens, (size_t)n_entries * 4);
	}
	if (he != hipSuccess) {
		(void)hipGetLastError();
		(void)hipFree(b.bases);
		(void)hipFree(b.offs);
		(void)hipFree(b.lens);
		cn_release_batches(st);
		st.state = CN_NO_MEMORY;
		return 0;
	}
	st.side[which].push_back(b);
	st.bytes[which] += n;
	st.entries[which] += n_entries;
	if (n) {
		CN_TRY(hipMemcpyAsync(b.bases, bases, (size_t)n, hipMemcpyDefault, stream), "cn_append");
	}
	CN_TRY(hipMemcpyAsync(b.offs, offs, (size_t)n_entries * 8, hipMemcpyDefault, stream), "cn_append");
	CN_TRY(hipMemcpyAsync(b.lens, lens, (size_t)n_entries * 4, hipMemcpyDefault, stream), "cn_append");
	return 0;
}

u64
cn_default_counters(const CnStore& st)
{
	const u64 larger = st.bytes[0] > st.bytes[1] ? st.bytes[0] : st.bytes[1];
	u64 c = CN_MIN_COUNTERS;
	while (c < CN_MAX_COUNTERS && c / 8 < larger) {
		c <<= 1;
	}
	return c;
}

int
cn_finish(CnStore& st, hipStream_t stream, const Filter& f, const DevParams& p, const u64* d_tab, u64 counters, std::string* why)
{
	cn_clear_results(st);
	for (auto& e : st.evt) {
		if (!e) {
			CN_TRY(hipEventCreate(&e), "cn_finish");
		}
	}
	if (st.sketch_bytes != counters) {
		(void)hipFree(st.sketch);
		st.sketch = nullptr;
		st.sketch_bytes = 0;
		if (hipMalloc((void**)&st.sketch, (size_t)counters) != hipSuccess) {
			(void)hipGetLastError();
			cn_release_batches(st);
			st.state = CN_NO_MEMORY;
			if (why) {
				*why = "cn_finish: no device memory for a sketch of " + std::to_string(counters) + " counters; the draft store was released";
			}
			return NTEDIT_E_OVERFLOW;
		}
		st.sketch_bytes = counters;
	}
	const size_t row_words[2] = { (size_t)st.entries[0] * CN_ROW_WORDS, (size_t)st.entries[1] * CN_ROW_WORDS };
	const size_t words = 2 * CN_SIDE_WORDS + row_words[0] + row_words[1];
	if (st.d_out_words < words) {
		(void)hipFree(st.d_out);
		st.d_out = nullptr;
		st.d_out_words = 0;
		CN_TRY(hipMalloc((void**)&st.d_out, words * 8), "cn_finish");
		st.d_out_words = words;
	}
	CN_TRY(hipMemsetAsync(st.d_out, 0, words * 8, stream), "cn_finish");
	const u64 smask = counters - 1;
	for (int which = 0; which < 2; which++) {
		unsigned long long* table = (unsigned long long*)st.d_out + (size_t)which * CN_SIDE_WORDS;
		unsigned long long* rows = (unsigned long long*)st.d_out + 2 * CN_SIDE_WORDS + (which ? row_words[0] : 0);
		hipEvent_t* ev = st.evt + 4 * which;
		CN_TRY(hipMemsetAsync(st.sketch, 0, (size_t)counters, stream), "cn_finish");
		for (int pass = 0; pass < 2; pass++) {
			CN_TRY(hipEventRecord(ev[2 * pass], stream), "cn_finish");
			u64 row_base = 0;
			for (const CnBatch& b : st.side[which]) {
				const u64 blocks = (b.n + TILE_STARTS - 1) / TILE_STARTS;
				if (blocks > 0x7FFFFFFFull) {
					if (why) {
						*why = "cn_finish: a stored batch is too large";
					}
					return NTEDIT_E_ARG;
				}
				if (blocks) {
					const dim3 grid((unsigned)blocks);
					unsigned long long* r = rows + row_base * CN_ROW_WORDS;
#define CN_LAUNCH(H)                                                                                                                 \
	case H:                                                                                                                          \
		if (pass == 0) {                                                                                                             \
			cn_launch_count<H>(grid, stream, b, p, d_tab, (u32*)st.sketch, smask);                                                   \
		} else {                                                                                                                     \
			cn_launch_spectrum<H>(grid, stream, b, f, p, d_tab, st.sketch, smask, table, table + CN_CLASSES * CN_BINS, r);           \
		}                                                                                                                            \
		break
					switch (f.hash_num) {
						CN_LAUNCH(1);
						CN_LAUNCH(2);
						CN_LAUNCH(3);
						CN_LAUNCH(4);
						CN_LAUNCH(5);
						CN_LAUNCH(6);
						CN_LAUNCH(7);
						CN_LAUNCH(8);
					default:
						if (why) {
							*why = "cn_finish: 1 to 8 hashes";
						}
						return NTEDIT_E_UNSUPPORTED;
					}
#undef CN_LAUNCH
					CN_TRY(hipGetLastError(), "cn_finish");
				}
				row_base += b.n_entries;
			}
			CN_TRY(hipEventRecord(ev[2 * pass + 1], stream), "cn_finish");
			if (pass == 0) {
				hipLaunchKernelGGL(k_cn_nonzero, dim3(1024), dim3(256), 0, stream, (const u64*)st.sketch, counters / 8, table + (CN_CLASSES + 1) * CN_BINS);
				CN_TRY(hipGetLastError(), "cn_finish");
			}
		}
	}
	std::vector<u64> host(words);
	CN_TRY(hipMemcpyAsync(host.data(), st.d_out, words * 8, hipMemcpyDeviceToHost, stream), "cn_finish");
	CN_TRY(hipStreamSynchronize(stream), "cn_finish");
	for (int which = 0; which < 2; which++) {
		const u64* t = host.data() + (size_t)which * CN_SIDE_WORDS;
		st.table[which].assign(t, t + CN_SIDE_WORDS);
		const u64* r = host.data() + 2 * CN_SIDE_WORDS + (which ? row_words[0] : 0);
		st.rows[which].assign(r, r + row_words[which]);
		st.nonzero[which] = t[(CN_CLASSES + 1) * CN_BINS];
		for (int pass = 0; pass < 2; pass++) {
			float ms = 0.f;
			if (hipEventElapsedTime(&ms, st.evt[4 * which + 2 * pass], st.evt[4 * which + 2 * pass + 1]) != hipSuccess) {
				(void)hipGetLastError();
				ms = 0.f;
			}
			st.ms[2 * which + pass] = ms;
		}
	}
	st.counters = counters;
	st.finished = true;
	return 0;
}

} // namespace nte
