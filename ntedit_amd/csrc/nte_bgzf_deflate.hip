// nte_bgzf_deflate.hip -- gfx950 kernels and host glue of the BGZF writer: the edited draft leaves the GPU compressed.
// The encoder is nte_bgzf_deflate.h, written once for the kernel and for the serial host model
// (ntedit_hip_bgzf_deflate_model, below); the stages are listed in nte_bgzf_launch.h.
//
//   k_bz_deflate   one wavefront per block of 65,280 bytes, four blocks per workgroup of 256; no wave waits for another.
//                  The wave's tables and the bit writer's ring are its 8 KiB of LDS; the block is read three times
//                  (histogram, CRC-32, payload), the second and third time out of the caches; the member goes to the
//                  block's own 64 KiB slot as aligned words.  One size word per block, an ordinary store.
//
// Like nte_apply.hip this unit is outside KSRC and sees no context internals.
#include "nte_bgzf_launch.h"

#ifdef NTE_BGZF_PHASES
// the timing build (make bgzf_phases): lane 0 of every wave adds the ticks of the constant 100 MHz clock that each stage
// of dz_member took -- 0 histogram, 1 code lengths and header, 2 CRC-32, 3 headers written, 4 payload, 5 trailer
__device__ unsigned long long g_dz_phase[8];
#endif
#if defined(NTE_BGZF_PHASES) && defined(__HIP_DEVICE_COMPILE__)
#define DZ_PHASE_BEGIN() unsigned long long dz_t0_ = wall_clock64()
#define DZ_PHASE(i)                                      \
	do {                                                 \
		const unsigned long long now_ = wall_clock64();  \
		if (lane == 0) {                                 \
			atomicAdd(&g_dz_phase[i], now_ - dz_t0_);    \
		}                                                \
		dz_t0_ = now_;                                   \
	} while (0)
#endif
#include "nte_bgzf_deflate.h"
#include "nte_reads_internal.h"

#include <cstring>
#include <mutex>
#include <vector>

using namespace nte;
using namespace nte_bgzf;

namespace {

constexpr int DZ_TPB = 256;
constexpr int DZ_WAVES = DZ_TPB / 64;
constexpr u32 IMG_TILE = 16384; // image bytes per workgroup of k_fa_image
constexpr u32 DZ_STORED_BIT = 1u << 31;

static_assert(sizeof(DzTables) <= 8704, "a wave's tables: 16 waves in under 160 KiB of LDS");
static_assert(DZ_HEAD + DZ_STORED + DZ_BLOCK + DZ_TAIL <= DZ_SLOT, "a stored member fits its slot");

__global__ __launch_bounds__(DZ_TPB) void
k_bz_deflate(const u8* __restrict__ src, u64 n, u8* __restrict__ slots, u32* __restrict__ sizes, u32 n_blocks)
{
	__shared__ DzTables s_tables[DZ_WAVES];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const u32 m = blockIdx.x * DZ_WAVES + wave;
	if (m >= n_blocks) {
		return;
	}
	const u64 at = (u64)m * DZ_BLOCK;
	const u32 len = n - at < DZ_BLOCK ? (u32)(n - at) : DZ_BLOCK;
	u32 stored = 0;
	const u32 size = dz_member(src + at, len, slots + (u64)m * DZ_SLOT, &s_tables[wave], lane, 64, &stored);
	if (lane == 0) {
		sizes[m] = size | (stored ? DZ_STORED_BIT : 0u);
	}
}

// offs[i] = the bytes of the members before i, offs[n] = all; totals[0] = offs[n], totals[1] = stored members
__global__ __launch_bounds__(DZ_TPB) void
k_bz_scan(const u32* __restrict__ sizes, u32 n, u64* __restrict__ offs, u64* __restrict__ totals)
{
	__shared__ u64 s_sum[DZ_TPB];
	__shared__ u32 s_stored[DZ_TPB];
	const u32 per = (n + DZ_TPB - 1) / DZ_TPB;
	const u32 a = threadIdx.x * per < n ? threadIdx.x * per : n, e = a + per < n ? a + per : n;
	u64 sum = 0;
	u32 st = 0;
	for (u32 i = a; i < e; i++) {
		sum += sizes[i] & ~DZ_STORED_BIT;
		st += sizes[i] >> 31;
	}
	s_sum[threadIdx.x] = sum;
	s_stored[threadIdx.x] = st;
	__syncthreads();
	if (threadIdx.x == 0) {
		u64 run = 0;
		u32 all = 0;
		for (int t = 0; t < DZ_TPB; t++) {
			const u64 v = s_sum[t];
			s_sum[t] = run;
			run += v;
			all += s_stored[t];
		}
		offs[n] = run;
		totals[0] = run;
		totals[1] = all;
	}
	__syncthreads();
	u64 run = s_sum[threadIdx.x];
	for (u32 i = a; i < e; i++) {
		offs[i] = run;
		run += sizes[i] & ~DZ_STORED_BIT;
	}
}

// member m from its slot to dst + offs[m]: bytes up to the first aligned word of the destination, words, the rest
__global__ __launch_bounds__(DZ_TPB) void
k_bz_pack(const u8* __restrict__ slots, const u32* __restrict__ sizes, const u64* __restrict__ offs, u8* __restrict__ dst)
{
	const u32 m = blockIdx.x;
	const u32 size = sizes[m] & ~DZ_STORED_BIT;
	const u8* s = slots + (u64)m * DZ_SLOT;
	u8* d = dst + offs[m];
	u32 head = (u32)((4 - ((uintptr_t)d & 3)) & 3);
	head = head < size ? head : size;
	const u32 words = (size - head) >> 2, tail = head + 4 * words;
	if (threadIdx.x < head) {
		d[threadIdx.x] = s[threadIdx.x];
	}
	for (u32 w = threadIdx.x; w < words; w += DZ_TPB) {
		u32 v;
		memcpy(&v, s + head + 4 * w, 4);
		*(u32*)(d + head + 4 * w) = v;
	}
	if (tail + threadIdx.x < size) {
		d[tail + threadIdx.x] = s[tail + threadIdx.x];
	}
}

struct ImageArgs
{
	const u8* edited;
	const u64* img_off;  // n + 1: where an entry's '>' stands in the image
	const u64* name_off; // n + 1
	const u64* e_offs;   // n
	const u8* names;
	u32 n;
	u64 total;
	u8* dst;
};

// the entry that holds image byte p, among lo .. hi
__device__ __forceinline__ u32
image_entry(const u64* __restrict__ img_off, u32 lo, u32 hi, u64 p)
{
	while (lo < hi) {
		const u32 mid = lo + (hi - lo + 1) / 2;
		if (img_off[mid] <= p) {
			lo = mid;
		} else {
			hi = mid - 1;
		}
	}
	return lo;
}

__global__ __launch_bounds__(DZ_TPB) void
k_fa_image(const ImageArgs a)
{
	__shared__ u32 s_range[2];
	const u64 t0 = (u64)blockIdx.x * IMG_TILE;
	const u64 t1 = t0 + IMG_TILE < a.total ? t0 + IMG_TILE : a.total;
	if (threadIdx.x < 2) {
		s_range[threadIdx.x] = image_entry(a.img_off, 0, a.n - 1, threadIdx.x == 0 ? t0 : t1 - 1);
	}
	__syncthreads();
	const u32 e_lo = s_range[0], e_hi = s_range[1];
	for (u32 ch = threadIdx.x; ch < IMG_TILE / 16; ch += DZ_TPB) {
		const u64 p0 = t0 + (u64)ch * 16;
		if (p0 >= t1) {
			break;
		}
		const u64 p1 = p0 + 16 < t1 ? p0 + 16 : t1;
		u32 e = image_entry(a.img_off, e_lo, e_hi, p0);
		u64 begin = a.img_off[e], end = a.img_off[e + 1];
		u64 head = a.name_off[e + 1] - a.name_off[e] + 2;
		if (p1 - p0 == 16 && p1 <= end && p0 >= begin + head) { // sixteen bytes of one entry's bases
			const u8* s = a.edited + a.e_offs[e] + (p0 - begin - head);
			uint4 v;
			memcpy(&v, s, 16);
			*(uint4*)(a.dst + p0) = v;
			continue;
		}
		for (u64 p = p0; p < p1; p++) {
			while (p >= end) { // (an entry is three bytes or more, and img_off[n] = total > p)
				e++;
				begin = end;
				end = a.img_off[e + 1];
				head = a.name_off[e + 1] - a.name_off[e] + 2;
			}
			const u64 rel = p - begin;
			a.dst[p] = rel == 0 ? (u8)'>' : rel == head - 1 ? (u8)'\n' : rel < head ? a.names[a.name_off[e] + rel - 1] : a.edited[a.e_offs[e] + rel - head];
		}
	}
}

// ------------------------------------------------------------------ host side
struct Buf
{
	u8* p = nullptr;
	u64 cap = 0;
};

struct DeflateState
{
	const void* owner = nullptr;
	int device = -1;
	hipEvent_t ev[2] = { nullptr, nullptr };
	// device scratch, grow-only, released by bgzf_release
	Buf src, image, tabs, slots, sizes, offs, packed;
	u64* h_tot = nullptr; // page-locked: bytes, stored members
	u32 n_blocks = 0;     // of the last bgzf_encode
	u64 bytes = 0;
};

std::mutex g_deflate_mu;
std::vector<DeflateState*> g_deflate;

DeflateState*
deflate_state(const void* owner, bool create)
{
	std::lock_guard<std::mutex> lk(g_deflate_mu);
	for (DeflateState* s : g_deflate) {
		if (s->owner == owner) {
			return s;
		}
	}
	if (!create) {
		return nullptr;
	}
	DeflateState* s = new DeflateState();
	s->owner = owner;
	g_deflate.push_back(s);
	return s;
}

#define DZ_TRY(expr)                                                   \
	do {                                                               \
		hipError_t e_ = (expr);                                        \
		if (e_ != hipSuccess) {                                        \
			*why = std::string(#expr ": ") + hipGetErrorString(e_);    \
			return NTEDIT_E_DEVICE;                                    \
		}                                                              \
	} while (0)

int
ensure_device(DeflateState* s, int device, std::string* why)
{
	DZ_TRY(hipSetDevice(device));
	if (s->device >= 0) {
		if (s->device != device) { // (a context has one device; its buffers and events live there)
			*why = "bgzf_deflate: the owner's buffers are on another device";
			return NTEDIT_E_ARG;
		}
		return 0;
	}
	for (hipEvent_t& e : s->ev) {
		DZ_TRY(hipEventCreate(&e));
	}
	DZ_TRY(hipHostMalloc((void**)&s->h_tot, 2 * sizeof(u64), hipHostMallocDefault));
	s->device = device;
	return 0;
}

// *b to at least `need` bytes (the stream is drained before a buffer in use is let go; nothing is kept)
int
grow(hipStream_t stream, Buf* b, u64 need, std::string* why)
{
	if (need <= b->cap && b->p) {
		return 0;
	}
	if (b->p) {
		DZ_TRY(hipStreamSynchronize(stream));
		DZ_TRY(hipFree(b->p));
		b->p = nullptr;
		b->cap = 0;
	}
	const u64 want = (need + need / 8 + 4096) / 256 * 256;
	DZ_TRY(hipMalloc((void**)&b->p, want));
	b->cap = want;
	return 0;
}

u64
block_count(u64 n)
{
	return (n + DZ_BLOCK - 1) / DZ_BLOCK;
}

} // namespace

namespace nte {

int
bgzf_image(const void* owner, int device, hipStream_t s, const FaImage& im, const u8** d_image, u64* n_image, float* ms, std::string* why)
{
	DeflateState* st = deflate_state(owner, true);
	int rc = ensure_device(st, device, why);
	if (rc) {
		return rc;
	}
	*d_image = nullptr;
	*n_image = 0;
	*ms = 0.f;
	if (im.n == 0) {
		return 0;
	}
	// one upload: img_off u64[n + 1] | name_off u64[n + 1] | e_offs u64[n] | the names
	const u64 n = im.n, names_bytes = im.name_offs[n];
	std::vector<u64> tab(3 * n + 2);
	u64 at = 0;
	for (u64 i = 0; i < n; i++) {
		tab[i] = at;
		at += (im.name_offs[i + 1] - im.name_offs[i]) + 2 + (u64)im.e_lens[i] + 1;
		tab[n + 1 + i] = im.name_offs[i];
		tab[2 * n + 2 + i] = im.e_offs[i];
	}
	tab[n] = at;
	tab[2 * n + 1] = names_bytes;
	const u64 tab_bytes = tab.size() * 8;
	if ((rc = grow(s, &st->tabs, tab_bytes + names_bytes + 16, why)) || (rc = grow(s, &st->image, at + 16, why))) {
		return rc;
	}
	DZ_TRY(hipMemcpyAsync(st->tabs.p, tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
	if (names_bytes) {
		DZ_TRY(hipMemcpyAsync(st->tabs.p + tab_bytes, im.names, names_bytes, hipMemcpyHostToDevice, s));
	}
	ImageArgs a;
	a.edited = im.d_edited;
	a.img_off = (const u64*)st->tabs.p;
	a.name_off = a.img_off + n + 1;
	a.e_offs = a.name_off + n + 1;
	a.names = st->tabs.p + tab_bytes;
	a.n = im.n;
	a.total = at;
	a.dst = st->image.p;
	DZ_TRY(hipEventRecord(st->ev[0], s));
	hipLaunchKernelGGL(k_fa_image, dim3((unsigned)((at + IMG_TILE - 1) / IMG_TILE)), dim3(DZ_TPB), 0, s, a);
	DZ_TRY(hipGetLastError());
	DZ_TRY(hipEventRecord(st->ev[1], s));
	DZ_TRY(hipStreamSynchronize(s)); // (the host tables are let go)
	DZ_TRY(hipEventElapsedTime(ms, st->ev[0], st->ev[1]));
	*d_image = st->image.p;
	*n_image = at;
	return 0;
}

int
bgzf_encode(const void* owner, int device, hipStream_t s, const u8* d_src, u64 n, BgzfTotals* t, std::string* why)
{
	DeflateState* st = deflate_state(owner, true);
	int rc = ensure_device(st, device, why);
	if (rc) {
		return rc;
	}
	t->plain = n;
	t->bytes = 0;
	t->members = t->stored = 0;
	t->ms_deflate = 0.f;
	st->n_blocks = 0;
	st->bytes = 0;
	const u64 nb = block_count(n);
	if (nb == 0) {
		return 0;
	}
	if (nb > 0x7FFFFFFFull) {
		*why = "bgzf_deflate: more than 2^31 blocks";
		return NTEDIT_E_ARG;
	}
	if ((rc = grow(s, &st->slots, nb * DZ_SLOT, why)) || (rc = grow(s, &st->sizes, nb * 4, why)) || (rc = grow(s, &st->offs, (nb + 3) * 8, why))) {
		return rc;
	}
	u64* offs = (u64*)st->offs.p;
	DZ_TRY(hipEventRecord(st->ev[0], s));
	hipLaunchKernelGGL(k_bz_deflate, dim3((unsigned)((nb + DZ_WAVES - 1) / DZ_WAVES)), dim3(DZ_TPB), 0, s, d_src, n, st->slots.p, (u32*)st->sizes.p, (u32)nb);
	DZ_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_bz_scan, dim3(1), dim3(DZ_TPB), 0, s, (const u32*)st->sizes.p, (u32)nb, offs, offs + nb + 1);
	DZ_TRY(hipGetLastError());
	DZ_TRY(hipEventRecord(st->ev[1], s));
	DZ_TRY(hipMemcpyAsync(st->h_tot, offs + nb + 1, 2 * sizeof(u64), hipMemcpyDeviceToHost, s));
	DZ_TRY(hipStreamSynchronize(s));
	DZ_TRY(hipEventElapsedTime(&t->ms_deflate, st->ev[0], st->ev[1]));
	t->bytes = st->h_tot[0];
	t->members = (u32)nb;
	t->stored = (u32)st->h_tot[1];
	st->n_blocks = (u32)nb;
	st->bytes = t->bytes;
	return 0;
}

int
bgzf_fetch(const void* owner, hipStream_t s, void* host_dst, u64 bytes, float* ms_copy, std::string* why)
{
	DeflateState* st = deflate_state(owner, false);
	*ms_copy = 0.f;
	if (!st || bytes != st->bytes) {
		*why = "bgzf_deflate: nothing encoded of that size";
		return NTEDIT_E_ARG;
	}
	if (bytes == 0) {
		return 0;
	}
	int rc = grow(s, &st->packed, bytes, why);
	if (rc) {
		return rc;
	}
	DZ_TRY(hipEventRecord(st->ev[0], s));
	hipLaunchKernelGGL(k_bz_pack, dim3(st->n_blocks), dim3(DZ_TPB), 0, s, (const u8*)st->slots.p, (const u32*)st->sizes.p, (const u64*)st->offs.p, st->packed.p);
	DZ_TRY(hipGetLastError());
	DZ_TRY(hipMemcpyAsync(host_dst, st->packed.p, bytes, hipMemcpyDeviceToHost, s));
	DZ_TRY(hipEventRecord(st->ev[1], s));
	DZ_TRY(hipStreamSynchronize(s));
	DZ_TRY(hipEventElapsedTime(ms_copy, st->ev[0], st->ev[1]));
	return 0;
}

int
bgzf_upload(const void* owner, int device, hipStream_t s, const void* host_src, u64 n, const u8** d_src, std::string* why)
{
	DeflateState* st = deflate_state(owner, true);
	int rc = ensure_device(st, device, why);
	if (rc == 0) {
		rc = grow(s, &st->src, n + 16, why);
	}
	if (rc) {
		return rc;
	}
	if (n) {
		DZ_TRY(hipMemcpyAsync(st->src.p, host_src, n, hipMemcpyHostToDevice, s));
	}
	*d_src = st->src.p;
	return 0;
}

int
bgzf_reserve(const void* owner, int device, hipStream_t s, u64 max_image, u32 max_entries, std::string* why)
{
	DeflateState* st = deflate_state(owner, true);
	int rc = ensure_device(st, device, why);
	if (rc) {
		return rc;
	}
	const u64 nb = block_count(max_image) + 1, ne = max_entries ? max_entries : 1;
	if ((rc = grow(s, &st->image, max_image + 16, why)) || (rc = grow(s, &st->tabs, (3 * ne + 2) * 8 + ne * 64, why)) ||
	    (rc = grow(s, &st->slots, nb * DZ_SLOT, why)) || (rc = grow(s, &st->sizes, nb * 4, why)) || (rc = grow(s, &st->offs, (nb + 3) * 8, why)) ||
	    (rc = grow(s, &st->packed, max_image / 3 + nb * 64, why)) || (rc = grow(s, &st->src, 4096, why))) {
		return rc;
	}
	// one small entry through every kernel: their code objects are loaded
	DZ_TRY(hipMemsetAsync(st->src.p, 'A', 1024, s));
	DZ_TRY(hipMemsetAsync(st->src.p + 1023, '\n', 1, s));
	const u64 e_off = 0, name_offs[2] = { 0, 1 };
	const u32 e_len = 1023;
	const FaImage im = { st->src.p, &e_off, &e_len, 1, "w", name_offs };
	const u8* d_image = nullptr;
	u64 n_image = 0;
	float ms = 0.f;
	BgzfTotals t;
	u8 sink[256];
	if ((rc = bgzf_image(owner, device, s, im, &d_image, &n_image, &ms, why)) || (rc = bgzf_encode(owner, device, s, d_image, n_image, &t, why))) {
		return rc;
	}
	if (t.bytes > sizeof sink) {
		*why = "bgzf_deflate: the warm-up member is larger than expected";
		return NTEDIT_E_INTERNAL;
	}
	return bgzf_fetch(owner, s, sink, t.bytes, &ms, why);
}

void
bgzf_release(const void* owner)
{
	DeflateState* st = nullptr;
	{
		std::lock_guard<std::mutex> lk(g_deflate_mu);
		for (size_t i = 0; i < g_deflate.size(); i++) {
			if (g_deflate[i]->owner == owner) {
				st = g_deflate[i];
				g_deflate.erase(g_deflate.begin() + (long)i);
				break;
			}
		}
	}
	if (!st) {
		return;
	}
	if (st->device >= 0) {
		(void)hipSetDevice(st->device);
		for (Buf* b : { &st->src, &st->image, &st->tabs, &st->slots, &st->sizes, &st->offs, &st->packed }) {
			if (b->p) {
				(void)hipFree(b->p);
			}
		}
		for (hipEvent_t e : st->ev) {
			if (e) {
				(void)hipEventDestroy(e);
			}
		}
		if (st->h_tot) {
			(void)hipHostFree(st->h_tot);
		}
	}
	delete st;
}

} // namespace nte

extern "C" {

uint64_t
ntedit_hip_bgzf_bound(uint64_t n)
{
	return n + block_count(n) * (DZ_HEAD + DZ_STORED + DZ_TAIL);
}

const uint8_t*
ntedit_hip_bgzf_eof(uint32_t* n)
{
	if (n) {
		*n = (uint32_t)sizeof DZ_EOF;
	}
	return DZ_EOF;
}

// the serial model: the same header functions, one block after the other, one lane
int
ntedit_hip_bgzf_deflate_model(const void* src, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* n_out)
{
	if (!n_out || (n && !src) || (cap && !out)) {
		return nte_reads::set_error(nullptr, NTEDIT_E_ARG, "bgzf_deflate_model: bad argument");
	}
	DzTables* t = new DzTables();
	std::vector<uint32_t> slot(DZ_SLOT / 4);
	uint64_t total = 0;
	for (uint64_t at = 0; at < n; at += DZ_BLOCK) {
		const u32 len = n - at < DZ_BLOCK ? (u32)(n - at) : DZ_BLOCK;
		u32 stored = 0;
		const u32 size = dz_member((const u8*)src + at, len, (u8*)slot.data(), t, 0, 1, &stored);
		if (total + size <= cap) {
			memcpy(out + total, slot.data(), size);
		}
		total += size;
	}
	delete t;
	*n_out = total;
	if (total > cap) {
		return nte_reads::set_error(nullptr, NTEDIT_E_OVERFLOW, "bgzf_deflate_model: the buffer is too small");
	}
	return 0;
}

#ifdef NTE_BGZF_PHASES
// the timing build only: the stages' ticks since the last reset, summed over the waves
int
ntedit_hip_bgzf_phases(uint64_t* ticks8, int reset)
{
	unsigned long long h[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(h, HIP_SYMBOL(g_dz_phase), sizeof h) != hipSuccess) {
		return NTEDIT_E_DEVICE;
	}
	for (int i = 0; i < 8; i++) {
		ticks8[i] = h[i];
		h[i] = 0;
	}
	if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_dz_phase), h, sizeof h) != hipSuccess) {
		return NTEDIT_E_DEVICE;
	}
	return 0;
}
#endif

} // extern "C"
