// nte_reads_inflate.hip -- gfx950 kernels and C ABI of --gpu_parse on BGZF reads: the members of a bgzip file are
// shipped compressed, inflated and checked against their CRC-32 in HBM, and the inflated bytes handed to the parse
// kernels (nte_reads_parse.hip) without ever existing on the host.  The decoder is nte_bgzf_inflate.h, written once
// for the kernel and for the serial host model (ntedit_hip_reads_inflate_model, below).
//
//   k_bz_inflate      one wavefront per member, four members per workgroup of 256; no wave waits for another.  The
//                     wave's tables are its 3.6 KiB of LDS; the compressed bytes come from global memory through a 64-bit
//                     bit buffer; the output window is the member's own output in global memory.  The CRC-32 is fused:
//                     the wave that inflated the member has its bytes in the caches, each lane takes a contiguous piece,
//                     and the pieces are combined in GF(2).  One status word per member, an ordinary store.
//   k_bz_last_start   the chunk cut: over the line table of nte_reads_parse.hip, the last record start by the rule of
//                     last_record_start (host/chunk_feed.h), an atomic max over the lines; 0: none.
//
// Like nte_reads_parse.hip this unit is outside KSRC and sees no context internals: its state hangs off the context
// pointer, its scratch grows only and goes with ntedit_hip_sketch_free.  It works on the parse unit's two streams.
#include "nte_common.h"
#include "nte_bgzf_inflate.h"

#include "nte_reads_internal.h"
#include "nte_reads_unit.h"

#include "../host/bgzf_walk.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

using namespace nte;
using namespace nte_bgzf;
using namespace nte_unit;

namespace {

constexpr int BZ_TPB = 256;
constexpr int BZ_WAVES = BZ_TPB / 64;

static_assert(NTEDIT_INFLATE_BAD_BLOCK == BZ_BAD_BLOCK && NTEDIT_INFLATE_BAD_CODES == BZ_BAD_CODES && NTEDIT_INFLATE_BAD_DIST == BZ_BAD_DIST &&
                  NTEDIT_INFLATE_OUT_OVER == BZ_OUT_OVER && NTEDIT_INFLATE_IN_OVER == BZ_IN_OVER && NTEDIT_INFLATE_SHORT_OUT == BZ_SHORT_OUT &&
                  NTEDIT_INFLATE_LEFT_IN == BZ_LEFT_IN && NTEDIT_INFLATE_BAD_CRC == BZ_BAD_CRC && NTEDIT_INFLATE_BAD_STORED == BZ_BAD_STORED &&
                  NTEDIT_INFLATE_BAD_SYMBOL == BZ_BAD_SYMBOL,
              "the header names the decoder's reasons");
static_assert(sizeof(BzTables) <= 4096, "a wave's tables: 16 waves in well under 160 KiB of LDS");

typedef ntedit_hip_bgzf_member Member;

// the host has checked every member against n_comp and out_cap (members_fit)
__global__ __launch_bounds__(BZ_TPB) void
k_bz_inflate(const u8* __restrict__ comp, const Member* __restrict__ members, u32 n_members, u8* out, u32* __restrict__ status)
{
	__shared__ BzTables s_tables[BZ_WAVES];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const u32 m = blockIdx.x * BZ_WAVES + wave;
	if (m >= n_members) {
		return;
	}
	const Member mb = members[m];
	u8* dst = out + mb.out_off;
	u32 st = bz_inflate(comp + mb.in_off, mb.n_in, dst, mb.n_out, &s_tables[wave], lane, 64);
	if (st == BZ_OK) {
		BZ_SYNC(); // the member's bytes were stored by all lanes
		u32 term = bz_crc_term(dst, mb.n_out, lane, 64);
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			term ^= __shfl_xor(term, d, 64);
		}
		if (~term != mb.crc) {
			st = BZ_BAD_CRC;
		}
	}
	if (lane == 0) {
		status[m] = st;
	}
}

// One lane per line L >= 1 whose first byte lies inside the buffer: a record start when it starts with '>' (FASTA), or
// with '@' while line L + 2, inside the buffer, starts with '+' (FASTQ).  Line j exists with its first byte below n
// exactly when j < n_lines.  *cut = the largest such start; it stays 0 when there is none (line 0 is no candidate).
__global__ __launch_bounds__(BZ_TPB) void
k_bz_last_start(const u8* __restrict__ raw, const u32* __restrict__ line_end, u64 n_lines, int kind, u32* cut)
{
	const u64 line = (u64)blockIdx.x * BZ_TPB + threadIdx.x + 1;
	if (line >= n_lines) {
		return;
	}
	const u32 s = line_end[line - 1] + 1;
	bool start;
	if (kind == '>') {
		start = raw[s] == '>';
	} else {
		start = raw[s] == '@' && line + 2 < n_lines && raw[line_end[line + 1] + 1] == '+';
	}
	if (start) {
		atomicMax(cut, s);
	}
}

// ------------------------------------------------------------------ host side
struct InflateKeep // survives ntedit_hip_sketch_free
{
	ntedit_hip_reads_inflate_stats info = {};
};

// device scratch, grow-only, released by ntedit_hip_sketch_free
struct InflateScratch
{
	int device = -1;
	hipStream_t stream = nullptr, copy_stream = nullptr; // the parse unit's
	hipEvent_t ev[2] = { nullptr, nullptr }, copied[2] = { nullptr, nullptr };
	DevBuf comp[2], members[2];
	DevBuf raw[2]; // the inflated chunk (a carried tail, then the members) and the next one's
	int cur = 0;
	DevBuf status;
	u32* h_status = nullptr; // page-locked
	u64 h_status_cap = 0;
	u32* d_cut = nullptr;
	u32* h_cut = nullptr; // page-locked
};

typedef State<InflateKeep, InflateScratch> InflateState;
Registry<InflateState> g_inflate;

int
ensure_device(const ntedit_hip_ctx* c, InflateScratch* s)
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
	s->copy_stream = (hipStream_t)copy_stream;
	for (hipEvent_t& e : s->ev) {
		NTE_TRY(c, hipEventCreate(&e));
	}
	for (hipEvent_t& e : s->copied) {
		NTE_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
	}
	NTE_TRY(c, hipMalloc((void**)&s->d_cut, sizeof(u32)));
	NTE_TRY(c, hipHostMalloc((void**)&s->h_cut, sizeof(u32), hipHostMallocDefault));
	s->device = device;
	return 0;
}

// the entry of every call: the context's state, its device and the parse unit's streams
int
ready(const ntedit_hip_ctx* c, InflateState** state)
{
	*state = g_inflate.find(c, true);
	return ensure_device(c, &(*state)->scr);
}

// buf to at least `need` bytes, by this unit's sizing rule (a quarter and a MiB of slack), the first `keep` bytes kept
int
room(const ntedit_hip_ctx* c, InflateScratch* s, DevBuf* buf, u64 need, u64 keep = 0)
{
	return grow(c, s->stream, buf, need, (need + need / 4 + (1u << 20)) / 256 * 256, keep);
}

int
room_status(const ntedit_hip_ctx* c, InflateScratch* s, u64 n_members)
{
	int rc = room(c, s, &s->status, n_members * 4);
	if (rc == 0 && n_members > s->h_status_cap) {
		if (s->h_status) {
			NTE_TRY(c, hipHostFree(s->h_status));
			s->h_status = nullptr;
		}
		const u64 want = n_members + n_members / 4 + 1024;
		NTE_TRY(c, hipHostMalloc((void**)&s->h_status, want * 4, hipHostMallocDefault));
		s->h_status_cap = want;
	}
	return rc;
}

void
release_scratch(InflateScratch* s)
{
	if (s->device < 0) {
		return;
	}
	(void)hipSetDevice(s->device);
	for (hipStream_t st : { s->stream, s->copy_stream }) {
		if (st) {
			(void)hipStreamSynchronize(st);
		}
	}
	for (hipEvent_t e : { s->ev[0], s->ev[1], s->copied[0], s->copied[1] }) {
		if (e) {
			(void)hipEventDestroy(e);
		}
	}
	for (void* p : { (void*)s->comp[0].p, (void*)s->comp[1].p, (void*)s->members[0].p, (void*)s->members[1].p, (void*)s->raw[0].p,
	                 (void*)s->raw[1].p, (void*)s->status.p, (void*)s->d_cut }) {
		if (p) {
			(void)hipFree(p);
		}
	}
	for (void* p : { (void*)s->h_status, (void*)s->h_cut }) {
		if (p) {
			(void)hipHostFree(p);
		}
	}
	*s = InflateScratch();
}

// every member inside its buffers: what the kernel relies on
bool
members_fit(const Member* m, u64 n_members, u64 n_comp, u64 out_cap)
{
	for (u64 i = 0; i < n_members; i++) {
		if (m[i].in_off > n_comp || m[i].n_in > n_comp - m[i].in_off || m[i].out_off > out_cap || m[i].n_out > out_cap - m[i].out_off) {
			return false;
		}
	}
	return true;
}

// the members of d_comp (table d_members) into d_out, their statuses to s->h_status; the stream is drained
int
inflate_on_device(const ntedit_hip_ctx* c, InflateState* st, const u8* d_comp, const Member* d_members, u64 n_members, u8* d_out)
{
	InflateScratch* s = &st->scr;
	if (n_members == 0) {
		return 0;
	}
	int rc = room_status(c, s, n_members);
	if (rc) {
		return rc;
	}
	NTE_TRY(c, hipEventRecord(s->ev[0], s->stream));
	const unsigned blocks = (unsigned)((n_members + BZ_WAVES - 1) / BZ_WAVES);
	hipLaunchKernelGGL(k_bz_inflate, dim3(blocks), dim3(BZ_TPB), 0, s->stream, d_comp, d_members, (u32)n_members, d_out, (u32*)s->status.p);
	NTE_TRY(c, hipGetLastError());
	NTE_TRY(c, hipEventRecord(s->ev[1], s->stream));
	NTE_TRY(c, hipMemcpyAsync(s->h_status, s->status.p, n_members * 4, hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	float ms = 0;
	NTE_TRY(c, hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
	st->keep.info.ms_kernels += ms;
	return 0;
}

const char*
reason_text(u32 st)
{
	static const char* const names[] = { "ok",
		                                 "a block of type 3",
		                                 "a bad code set",
		                                 "a distance before the member's first byte",
		                                 "more output than ISIZE",
		                                 "the stream runs past the member's compressed bytes",
		                                 "less output than ISIZE",
		                                 "compressed bytes left over",
		                                 "CRC-32 mismatch",
		                                 "a stored block with a bad length",
		                                 "bits that are no code" };
	return st < sizeof names / sizeof names[0] ? names[st] : "unknown";
}

} // namespace

// what the pass loop of reads_pass.cpp needs beyond the public calls (nte_reads_internal.h says what each does)
namespace nte_reads {

void
inflate_release(const ntedit_hip_ctx* c)
{
	bam_release(c); // (nte_reads_bam.hip works on the same streams, behind this unit's chunks)
	InflateState* s = g_inflate.find(c, false);
	if (s) {
		release_scratch(&s->scr);
	}
}

ntedit_hip_reads_inflate_stats*
inflate_info(const ntedit_hip_ctx* c)
{
	return &g_inflate.find(c, true)->keep.info;
}

const char*
inflate_reason(uint32_t st)
{
	return reason_text(st);
}

int
inflate_copy_begin(const ntedit_hip_ctx* c, int which, const char* comp, uint64_t n_comp, const ntedit_hip_bgzf_member* members,
                   uint64_t n_members)
{
	InflateState* st;
	int rc = ready(c, &st);
	InflateScratch* s = &st->scr;
	if (rc == 0) {
		rc = room(c, s, &s->comp[which], n_comp);
	}
	if (rc == 0) {
		rc = room(c, s, &s->members[which], n_members * sizeof(Member));
	}
	if (rc) {
		return rc;
	}
	if (n_comp) {
		NTE_TRY(c, hipMemcpyAsync(s->comp[which].p, comp, n_comp, hipMemcpyHostToDevice, s->copy_stream));
	}
	if (n_members) {
		NTE_TRY(c, hipMemcpyAsync(s->members[which].p, members, n_members * sizeof(Member), hipMemcpyHostToDevice, s->copy_stream));
	}
	NTE_TRY(c, hipEventRecord(s->copied[which], s->copy_stream));
	return 0;
}

int
inflate_copy_wait(const ntedit_hip_ctx* c, int which)
{
	InflateState* s = g_inflate.find(c, false);
	if (s && s->scr.copied[which]) {
		NTE_TRY(c, hipEventSynchronize(s->scr.copied[which]));
	}
	return 0;
}

int
inflate_copied(const ntedit_hip_ctx* c, int which, uint64_t n_comp, const ntedit_hip_bgzf_member* members, uint64_t n_members,
               uint64_t tail, uint64_t n_out, const char** raw, uint64_t* bad, uint32_t* reason)
{
	InflateState* st;
	int rc = ready(c, &st);
	InflateScratch* s = &st->scr;
	if (rc == 0) {
		rc = room(c, s, &s->raw[s->cur], tail + n_out + 16, tail); // (a carried tail moves with the buffer)
	}
	if (rc) {
		return rc;
	}
	if (!members_fit(members, n_members, n_comp, n_out)) {
		return pfail(c, NTEDIT_E_ARG, "reads_inflate: a member outside its buffers");
	}
	NTE_TRY(c, hipEventSynchronize(s->copied[which]));
	*raw = (const char*)s->raw[s->cur].p;
	*bad = n_members;
	*reason = 0;
	rc = inflate_on_device(c, st, s->comp[which].p, (const Member*)s->members[which].p, n_members, s->raw[s->cur].p + tail);
	if (rc) {
		return rc;
	}
	for (uint64_t i = 0; i < n_members; i++) {
		if (s->h_status[i]) {
			*bad = i;
			*reason = s->h_status[i];
			break;
		}
	}
	st->keep.info.members += n_members;
	st->keep.info.comp_bytes += n_comp;
	st->keep.info.raw_bytes += n_out;
	return 0;
}

int
inflate_last_start(const ntedit_hip_ctx* c, const char* d_raw, uint64_t n, uint64_t* cut, uint32_t* broken)
{
	InflateState* st;
	int rc = ready(c, &st);
	if (rc) {
		return rc;
	}
	InflateScratch* s = &st->scr;
	*cut = 0;
	*broken = 0;
	if (n < 2) {
		return 0;
	}
	unsigned char kind = 0;
	NTE_TRY(c, hipMemcpyAsync(&kind, d_raw, 1, hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	if (kind != '>' && kind != '@') {
		*cut = n; // (unclean anyway, as RawProducer has it)
		return 0;
	}
	NTE_TRY(c, hipEventRecord(s->ev[0], s->stream));
	const uint32_t* line_end = nullptr;
	uint64_t n_lines = 0;
	if ((rc = nte_reads::parse_lines(c, (const unsigned char*)d_raw, n, &line_end, &n_lines, broken)) != 0) {
		return rc;
	}
	if (*broken) {
		return 0;
	}
	NTE_TRY(c, hipMemsetAsync(s->d_cut, 0, sizeof(u32), s->stream));
	if (n_lines > 1) {
		const unsigned blocks = (unsigned)((n_lines - 1 + BZ_TPB - 1) / BZ_TPB);
		hipLaunchKernelGGL(k_bz_last_start, dim3(blocks), dim3(BZ_TPB), 0, s->stream, (const u8*)d_raw, line_end, n_lines, (int)kind, s->d_cut);
		NTE_TRY(c, hipGetLastError());
	}
	NTE_TRY(c, hipEventRecord(s->ev[1], s->stream));
	NTE_TRY(c, hipMemcpyAsync(s->h_cut, s->d_cut, sizeof(u32), hipMemcpyDeviceToHost, s->stream));
	NTE_TRY(c, hipStreamSynchronize(s->stream));
	float ms = 0;
	NTE_TRY(c, hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
	st->keep.info.ms_kernels += ms;
	*cut = *s->h_cut;
	return 0;
}

int
inflate_carry(const ntedit_hip_ctx* c, uint64_t cut, uint64_t total)
{
	InflateScratch* s = &g_inflate.find(c, true)->scr;
	const int other = s->cur ^ 1;
	const uint64_t tail = total - cut;
	int rc = room(c, s, &s->raw[other], tail + 16);
	if (rc) {
		return rc;
	}
	if (tail) {
		NTE_TRY(c, hipMemcpyAsync(s->raw[other].p, s->raw[s->cur].p + cut, tail, hipMemcpyDeviceToDevice, s->stream));
	}
	s->cur = other;
	return 0;
}

} // namespace nte_reads

extern "C" {

int
ntedit_hip_reads_inflate_info(ntedit_hip_ctx* c, ntedit_hip_reads_inflate_stats* st)
{
	if (!c || !st) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_inflate_info: bad argument") : NTEDIT_E_ARG;
	}
	*st = g_inflate.find(c, true)->keep.info;
	return 0;
}

int
ntedit_hip_reads_inflate_device(ntedit_hip_ctx* c, const void* comp, uint64_t n_comp, int on_device, const ntedit_hip_bgzf_member* members,
                                uint64_t n_members, void* out_device, uint64_t out_cap, uint32_t* status)
{
	if (!c || !status || (n_members && (!members || !comp)) || (out_cap && !out_device) || n_members > 0xFFFFFFFFull ||
	    (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE)) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_inflate_device: bad argument") : NTEDIT_E_ARG;
	}
	if (!members_fit(members, n_members, n_comp, out_cap)) {
		return pfail(c, NTEDIT_E_ARG, "reads_inflate_device: a member outside comp[0 .. n_comp) or out[0 .. out_cap)");
	}
	InflateState* st;
	int rc = ready(c, &st);
	if (rc || n_members == 0) {
		return rc;
	}
	InflateScratch* s = &st->scr;
	const u8* d_comp = (const u8*)comp;
	if (on_device == NTEDIT_HIP_BASES_HOST) {
		if ((rc = room(c, s, &s->comp[0], n_comp)) != 0) {
			return rc;
		}
		if (n_comp) {
			NTE_TRY(c, hipMemcpyAsync(s->comp[0].p, comp, n_comp, hipMemcpyHostToDevice, s->stream));
		}
		d_comp = s->comp[0].p;
	}
	if ((rc = room(c, s, &s->members[0], n_members * sizeof(Member))) != 0) {
		return rc;
	}
	NTE_TRY(c, hipMemcpyAsync(s->members[0].p, members, n_members * sizeof(Member), hipMemcpyHostToDevice, s->stream));
	if ((rc = inflate_on_device(c, st, d_comp, (const Member*)s->members[0].p, n_members, (u8*)out_device)) != 0) {
		return rc;
	}
	memcpy(status, s->h_status, n_members * 4);
	return 0;
}

// the serial model: the same header functions, one member after the other, the CRC over 64 pieces as the wave takes it
int
ntedit_hip_reads_inflate_model(const void* comp, uint64_t n_comp, const ntedit_hip_bgzf_member* members, uint64_t n_members, void* out,
                               uint64_t out_cap, uint32_t* status)
{
	if (!status || (n_members && (!members || !comp)) || (out_cap && !out)) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_inflate_model: bad argument");
	}
	if (!members_fit(members, n_members, n_comp, out_cap)) {
		return pfail(nullptr, NTEDIT_E_ARG, "reads_inflate_model: a member outside comp[0 .. n_comp) or out[0 .. out_cap)");
	}
	BzTables* t = new BzTables();
	for (uint64_t i = 0; i < n_members; i++) {
		const Member& m = members[i];
		u8* dst = (u8*)out + m.out_off;
		u32 st = bz_inflate((const u8*)comp + m.in_off, m.n_in, dst, m.n_out, t, 0, 1);
		if (st == BZ_OK) {
			u32 crc = 0;
			for (u32 lane = 0; lane < 64; lane++) {
				crc ^= bz_crc_term(dst, m.n_out, lane, 64);
			}
			if (~crc != m.crc) {
				st = BZ_BAD_CRC;
			}
		}
		status[i] = st;
	}
	delete t;
	return 0;
}

// the member walk itself is host/bgzf_walk.h, which the chunk feeders (host/chunk_feed.h) call too
int
ntedit_hip_bgzf_walk(const void* bytes, uint64_t n, ntedit_hip_bgzf_member* members, uint64_t cap, uint64_t* n_members, uint64_t* consumed)
{
	if ((n && !bytes) || (cap && !members) || !n_members || !consumed) {
		return pfail(nullptr, NTEDIT_E_ARG, "bgzf_walk: bad argument");
	}
	return nte_host::bgzf_walk(bytes, n, members, cap, n_members, consumed);
}

int
ntedit_hip_reads_last_start_device(ntedit_hip_ctx* c, const void* buf, uint64_t n, int on_device, uint64_t* cut)
{
	if (!c || !cut || (n && !buf) || n >= (1ull << 31) || (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) ||
	    (on_device == NTEDIT_HIP_BASES_DEVICE && ((uintptr_t)buf & 15))) {
		return c ? pfail(c, NTEDIT_E_ARG, "reads_last_start_device: bad argument") : NTEDIT_E_ARG;
	}
	InflateState* st;
	int rc = ready(c, &st);
	if (rc) {
		return rc;
	}
	InflateScratch* s = &st->scr;
	const char* d_buf = (const char*)buf;
	if (on_device == NTEDIT_HIP_BASES_HOST) {
		if ((rc = room(c, s, &s->raw[s->cur], n + 16)) != 0) {
			return rc;
		}
		if (n) {
			NTE_TRY(c, hipMemcpyAsync(s->raw[s->cur].p, buf, n, hipMemcpyHostToDevice, s->stream));
		}
		d_buf = (const char*)s->raw[s->cur].p;
	}
	uint32_t broken = 0;
	uint64_t at = 0;
	if ((rc = nte_reads::inflate_last_start(c, d_buf, n, &at, &broken)) != 0) {
		return rc;
	}
	if (broken) {
		return pfail(c, NTEDIT_E_ARG, "reads_last_start_device: more than one line per 8 bytes");
	}
	*cut = at ? at : NTEDIT_READS_NO_START;
	return 0;
}

} // extern "C"
