// nte_api.hip -- implementation of the C ABI in include/ntedit_hip.h.
// Host side of the library: context / buffer management on one MI355X,
// kernel launches on the context's HIP stream, HIP-event timing, and the glue
// to the host renderer.  No CPU compute path exists here: every entry point
// that needs the GPU fails with NTEDIT_E_DEVICE when there is none.
#include "nte_kernels.hip"
#include "nte_settle.h"
#include "nte_apply.h"
#include "nte_bgzf_launch.h"
#include "nte_track.h"
#include "nte_cn.h"

#include "../../include/ntedit_hip.h"
#include "../host/batch_layout.h"
#include "../host/bfio.h"
#include "../host/params.h"
#include "../host/render.h"
#include "../host/resolve.h"

#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sched.h>
#include <string>
#include <vector>

using namespace nte;

namespace {

struct DevBuf
{
	void* p = nullptr;
	size_t cap = 0;
};

struct DevFilter
{
	u8* data = nullptr;
	u64 nbytes = 0;
	u32 hash_num = 0, k = 0;
	bool counting = false, owned = false, set = false;
};

} // namespace

// page-locked host buffer (D2H at PCIe speed, no zero-fill); recycled through the context
static std::atomic<unsigned> g_host_threads(0); // ntedit_hip_set_host_threads()

// contexts that are alive: a result that outlives its context (a garbage-collected binding may free them in
// any order) must not hand its buffers back to a pool that is gone
static std::mutex g_live_mu;
static std::vector<const void*> g_live_ctx;

static bool
ctx_alive(const void* c)
{
	std::lock_guard<std::mutex> lk(g_live_mu);
	for (const void* p : g_live_ctx) {
		if (p == c) {
			return true;
		}
	}
	return false;
}

struct PinBuf
{
	void* p = nullptr;
	size_t cap = 0;
};

// the two HIP events around a timed piece of work on one stream (ensure_events creates them on first use)
struct EventPair
{
	hipEvent_t begin = nullptr, end = nullptr;
};

// A window that has been waited for, in ms: the one reader of HIP-event times for figures that are only reported: 0, and the
// runtime's last error left clear, where the events cannot say (never recorded, or the runtime refuses).
static float
elapsed_ms(hipEvent_t begin, hipEvent_t end)
{
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, begin, end) != hipSuccess) {
		(void)hipGetLastError();
		return 0.f;
	}
	return ms;
}
static float elapsed_ms(const EventPair& p) { return elapsed_ms(p.begin, p.end); }

namespace {

int ensure(ntedit_hip_ctx* c, DevBuf& b, size_t bytes);

void
release(DevBuf& b)
{
	if (b.p) {
		(void)hipFree(b.p);
	}
	b.p = nullptr;
	b.cap = 0;
}

void
destroy_event(hipEvent_t e)
{
	if (e) {
		(void)hipEventDestroy(e);
	}
}

void
destroy_event(const EventPair& p)
{
	destroy_event(p.begin);
	destroy_event(p.end);
}

void
release_all(std::initializer_list<DevBuf*> bufs, std::initializer_list<const EventPair*> windows)
{
	for (DevBuf* b : bufs) {
		release(*b);
	}
	for (const EventPair* w : windows) {
		destroy_event(*w);
	}
}

// ---- The reports behind the device applier, one state struct each (helpers and entry points: nte_api_reports.inc): its device
// buffers, its windows (created by the first call that times one), its switch, the last call's figures.  size*() are the only
// place a buffer's size is written: the stage passes the batch's values, ntedit_hip_reserve its estimates.
struct ApplyReport // the device applier and the QV counts (nte_apply.hip)
{
	DevBuf ev, place, range, contig, tabs, pieces, bitmap, rows;
	DevBuf edited; // (under pin_mu: a result that is freed hands it back from another thread)
	// the applier, and per side of the draft (0 the batch, 1 the edited bases) the plain screening and the QV count
	EventPair window[1], screen[2], count[2];
	ntedit_hip_apply_stats last = { 0.f, 0.f, 0.f, 0, 0, 0 };
	// before launch_apply_plan: an event's summary and place, per entry its event range, its contig record and the tables
	// (tabs: out_offs u64[nc] | piece_base u64[nc + 1] | totals u64[3] | status (8 bytes) | out_lens u32[nc])
	int size_plan(ntedit_hip_ctx* c, u64 events, u64 nc)
	{
		int rc;
		if ((rc = ensure(c, ev, (size_t)(events + 1) * sizeof(ApplyEvent))) || (rc = ensure(c, place, (size_t)(events + 1) * sizeof(ApplyPlace))) ||
		    (rc = ensure(c, range, nc * 8)) || (rc = ensure(c, contig, nc * sizeof(ApplyContig)))) {
			return rc;
		}
		return ensure(c, tabs, nc * 8 + (nc + 1) * 8 + 32 + nc * 4);
	}
	// once the plan's totals are known: the edited bases (eb: wherever they are held just now) and the piece table
	int size_write(ntedit_hip_ctx* c, DevBuf& eb, u64 edited_bytes, u64 n_pieces)
	{
		const int rc = ensure(c, eb, (size_t)((edited_bytes + 15) / 16 * 16 + 64));
		return rc ? rc : ensure(c, pieces, (size_t)(n_pieces + 1) * sizeof(ApplyPiece));
	}
	// before either side is assessed: the QV rows (none for ntedit_hip_track_extract), a plain bitmap for the larger side
	int size_assess(ntedit_hip_ctx* c, u64 positions, u64 entries)
	{
		const int rc = ensure(c, rows, (size_t)entries * sizeof(QvRow));
		return rc ? rc : ensure(c, bitmap, (size_t)((positions + 63) / 64 + 8) * 8);
	}
	void release() { release_all({ &ev, &place, &range, &contig, &tabs, &pieces, &bitmap, &rows, &edited }, { window, screen, screen + 1, count, count + 1 }); }
};

struct TrackReport // the interval extractor (nte_track.hip)
{
	DevBuf tiles, recs, upto, totals;
	EventPair window[2]; // the count and scan, the emit
	ntedit_hip_track_stats last = { { 0.f, 0.f }, { 0, 0 }, { 0, 0 } };
	// the tiles' counts and the totals for a bitmap of `positions`; the records and their side array for `intervals`
	int size(ntedit_hip_ctx* c, u64 positions, u64 intervals)
	{
		int rc;
		if ((rc = ensure(c, tiles, (size_t)track_tiles(positions) * sizeof(TrackTile))) || (rc = ensure(c, totals, 64)) ||
		    (rc = ensure(c, recs, (size_t)intervals * sizeof(TrackInterval)))) {
			return rc;
		}
		return ensure(c, upto, (size_t)intervals * 4);
	}
	void release() { release_all({ &tiles, &recs, &upto, &totals }, { window, window + 1 }); }
};

struct SpectrumReport // the k-mer spectrum (k_spectrum; ntedit_hip_set_spectrum)
{
	bool on = false;
	DevBuf buf; // [which][256] bins, then [which][n_entries][3] rows
	EventPair window[2]; // per side
	ntedit_hip_spectrum_stats last = { { 0.f, 0.f }, { 0, 0 } };
	static size_t bytes(u64 entries) { return (2 * (size_t)SPECTRUM_BINS + 2 * (size_t)entries * 3) * 8; }
	unsigned long long* bins(int which) const { return (unsigned long long*)buf.p + (size_t)which * SPECTRUM_BINS; }
	unsigned long long* rows(int which, u32 n_entries) const { return bins(2) + (size_t)which * n_entries * 3; }
	void release() { release_all({ &buf }, { window, window + 1 }); }
};

// linear counting of the draft's present k-mers (k_mark; ntedit_hip_shared_*): two mark arrays of the PRIMARY filter's size,
// before and after; they go when the slot gets another filter (drop_filter)
struct SharedReport
{
	DevBuf marks[2];
	u64 bytes = 0;                 // the filter's byte size the marks were made for (0: none)
	u64 calls = 0;                 // k_mark launches since the last reset
	float ms[2] = { 0.f, 0.f };    // their HIP-event time, per array
	EventPair window[2];           // per array
	void release_marks()           // (the events stay: drop_filter, ntedit_hip_shared_free)
	{
		release_all({ marks, marks + 1 }, {});
		bytes = calls = 0;
		ms[0] = ms[1] = 0.f;
	}
	void release() { release_all({ marks, marks + 1 }, { window, window + 1 }); }
};

struct BgzfReport // the BGZF writer (nte_bgzf_deflate.hip): the header lines of the next polish call, the last call's figures
{
	std::vector<std::string> fa_names;
	bool fa_names_set = false;
	ntedit_hip_bgzf_stats last = { 0.f, 0.f, 0.f, 0, 0, 0, 0 };
	std::vector<PinBuf> pool; // page-locked buffers for the members, apart from pin_pool (under pin_mu): filled by reserve
	void release()
	{
		for (PinBuf& pb : pool) {
			(void)hipHostFree(pb.p);
		}
		pool.clear();
	}
};

struct Reports
{
	ApplyReport ap;
	TrackReport tr;
	SpectrumReport sp;
	SharedReport sh;
	BgzfReport bz;
	void release() { ap.release(), tr.release(), sp.release(), sh.release(), bz.release(); } // (ntedit_hip_destroy)
};

} // namespace

struct ntedit_hip_ctx
{
	int device = 0;
	hipStream_t stream = nullptr;
	hipStream_t stream2 = nullptr; // event extraction + machine of the chunk pipeline
	std::vector<hipEvent_t> chunk_ev; // 2 per chunk on `stream` (screen begin / end)
	std::vector<hipEvent_t> h2d_ev;   // one per host-to-device piece of a host-resident batch
	std::vector<hipEvent_t> bin_ev;   // 3 per record chunk of the binned screening (start, partitioned, probed)
	u32 bin_chunks_last = 0;          // chunks of the last binned screening (0: the direct kernel ran)
	u64 h2d_piece_bytes = 0;          // > 0: the batch is arriving from the host in pieces of this size on stream2
	u64 h2d_pieces = 0;               //      (h2d_ev[i] = piece i is in HBM); the binned screening waits chunk by chunk
	DevFilter filt[2];
	ntedit_hip_params hp;
	DevParams dp;
	bool dp_valid = false;
	u64* d_tab = nullptr;
	u32 tab_k = 0;
	std::string err;
	float last_ms = 0.f;
	hipEvent_t ev[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
	hipEvent_t ev_assess[2] = { nullptr, nullptr };
	hipEvent_t ev_settle[2] = { nullptr, nullptr }; // around a k_settle launch
	ntedit_hip_settle_stats settle_last = { 0, 0, 0.f }; // ntedit_hip_settle_info(): the last polish call
	DevBuf packed; // a batch as it crossed PCIe in the packed form (NTEDIT_HIP_BASES_PACKED), before k_unpack
	DevBuf runmap; // the absent bitmap minus the positions that cannot do anything (k_assess)
	DevBuf candmap; // -s 1 on a plain filter: 4 bits per position, the first-probe bits of its substitution candidates (k_wc_scatter_b<3, ., 1>)
	DevBuf seq, bitmap, block_counts, block_offsets, events, first_chunk, arena, counters, deferred;
	DevBuf ws_nodes, ws_ov_pos, ws_ov_chr, ws_prev, ws_lps, ws_win;
	DevBuf offs, lens;
	DevBuf bin_records, bin_fill, bin_ctl, bin_ovf, bin_state; // the binned screening: records, run fills, probe control words, overflow list, chunk flags
	struct BinRange
	{
		u64 begin, end;  // k-mer starts of one record chunk
		bool recovered;  // its overflow list ran out and the direct kernel has screened it again
		bool gate;       // a chunk of the candidate map (-s 1): "screened again" = its part of the map set to unknown
	};
	std::vector<BinRange> bin_ranges; // the record chunks of the current call, in launch order (bin_state's flags)
	std::vector<u32> bin_flags_host;
	u32 bin_chunks_direct = 0;        // chunks of the current call the direct kernel had to screen again
	u64 bin_ovf_entries = 0;          // overflow entries handed out in the current call (as of the last bin_recover)
	hipStream_t stream_copy = nullptr; // H2D pieces of a host batch that is polished in pipeline chunks (stream2 runs the event machine then)
	struct Tuning                     // ntedit_hip_set_tuning(): test / tuning knobs, none of which can change a result
	{
		u32 screen_mode = 0;     // overrides params.screen_mode when not 0
		u64 bin_chunk = 0;       // k-mer starts per record chunk of the binned screening (tests: several chunks)
		u32 bin_cap_percent = 0; // run capacity in percent of the expected records (tests: force the overflow list)
		u64 bin_ovf_cap = 0;     // entries of the overflow list (tests: a list that runs out; 0: an eighth of the chunk's records)
		u32 bin_fallback = 0;    // 1: the direct kernel whatever the sizes (as "screen_mode" 1; kept for callers of round 5)
		u32 force_xcc = 0;       // x + 1: every probe wavefront pretends to run on XCD x (tests)
		u32 bin_timing = 0;      // per-stage times of the binned screening on stderr
		u64 chunk_bytes = 0;     // pipeline chunk size (tests: many chunks)
		u64 h2d_piece = ~0ULL;   // bytes per host-to-device piece (~0: default)
		u32 inline_tries = ~0u;  // candidates of an indel sweep the deferring launch tries itself (~0: default)
		u32 assess = ~0u;        // k_assess before the event machine: 0 never, 1 always, ~0: with -s 1 and with counting filters
		u32 machine_cfg = ~0u;   // 0: always the general instantiation of the machine kernels (~0: the most specific one)
		u32 lanes = ~0u;         // DevParams::lanes (~0: default)
		u32 defer_run = ~0u;     // DevParams::defer_run (~0: default)
		u32 defer_fail = ~0u;    // DevParams::defer_fail (~0: default)
		u32 defer_fail_snv = ~0u; // DevParams::defer_fail_snv (~0: default)
		u32 h2d_fixed_schedule = 0; // a batch arriving in pieces: round 3's chunk schedule (1, 3, 8 pieces, the rest) instead of chunks by arrival
		u32 candmap = 0;         // the candidate map of -s 1 (nte_bin_wc.inc MODE 1): 1 = whenever the configuration allows it (measured slower: off)
		u32 snv_wave = 0;        // -s 1 with the run map: the events go to the wavefront-per-event launch (experiment)
		u32 no_rounds = 0, no_early_copy = 0;
		u32 force_rounds = 0;     // event rounds whatever the number of events (tests: small inputs)
		u64 arena_chunks = 0;     // chunks of the edit-record arena in the first attempt (tests: one that runs out; 0: by batch size)
		u32 settle = ~0u;         // k_settle in front of the thread-per-event launch: 0 never, 1 wherever it applies, ~0: auto
		u32 bin_scatter = 0;      // partition kernel: 0 barrier-phased (k_wc_scatter_b), 1 barrier-free (k_wc_scatter)
		u32 probe_parts_log2 = ~0u; // probe stage: slices probed in 2^x parts (~0: by slice size)
		u32 bin_slice_log2 = 0;   // log2 of the slots of a filter slice (0: 2 MiB), doubled until the partition kernel has rings for all slices (tests: many slices of a small filter)
		u32 bin_wide_min_run = 0; // records a (slice, workgroup) pair must expect for more than 1024 slices (0: WCB_WIDE_MIN_RUN; tests: both sides of the rule on a small batch)
		u32 bin_ring = 0;         // k_wc_scatter_b: 8 = the wide layout (8-slot rings) whatever the slices, 16 = never (1024 slices at most), 0: wide beyond 1024 slices
	} tune;
	DevBuf ev_cover, ev_before, ev_flags, ev_list, ev_bmax; // event rounds
	DevBuf ev_rest; // the events of a round k_settle declined (nte_settle.hip)
	u32 apply_flags = 0; // ntedit_hip_set_apply()
	Reports rep;
	CnStore cn; // the spectrum by copy number (nte_cn.hip): the switch is the store's state; both sides stay in HBM until ntedit_hip_cn_finish
	u32 cu_count = 256;
	size_t lds_per_block = 160 * 1024;
	double alloc_ms = 0.0;            // host time spent in hipFree + hipMalloc of the grow-only buffers (ensure())
	u32 alloc_calls = 0;
	std::vector<PinBuf> pin_pool;
	std::mutex pin_mu;
};

struct ntedit_hip_result
{
	ntedit_hip_ctx* owner = nullptr;
	PinBuf arena_buf;      // arena copy (Items)
	size_t arena_items = 0;
	PinBuf first_buf;      // per-event first chunk, then compacted in place to ev_first
	size_t n_ev_first = 0;
	ntedit_hip_stats st;
	nte_host::RenderStats rst;
	int snv = 0; // -s of the parameters the batch was polished with
	u32 part_margin = 0; // k + max deletions + slack of those parameters (RenderOptions::part_margin)
	// ntedit_hip_result_edits(): built on first use
	bool edits_built = false;
	std::vector<ntedit_hip_edit> edits;
	std::string edit_pool;
	// the applier's output (NTEDIT_HIP_APPLY_*): the edited bases in HBM, their table, the QV rows
	u32 apply_flags = 0;
	int device = 0;
	DevBuf edited;
	u64 edited_bytes = 0;
	std::vector<uint64_t> e_offs;
	std::vector<uint32_t> e_lens;
	std::vector<ntedit_hip_qv_row> qv;
	// NTEDIT_HIP_APPLY_BGZF: the batch's _edited.fa text as BGZF members, page-locked
	PinBuf bgzf_buf;
	u64 bgzf_bytes = 0, bgzf_plain = 0;
	u32 bgzf_members = 0;
	// NTEDIT_HIP_APPLY_TRACK: the intervals before and after (malloc)
	ntedit_hip_track_interval* track[2] = { nullptr, nullptr };
	u64 track_n[2] = { 0, 0 };
	// ntedit_hip_set_spectrum: the bins before and after, a depth row per entry
	bool spectrum = false;
	std::vector<uint64_t> sp_bins;
	std::vector<ntedit_hip_depth_row> depth;
	~ntedit_hip_result()
	{
		free(track[0]);
		free(track[1]);
	}
};

namespace {

int
fail(ntedit_hip_ctx* c, int code, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (c) {
		c->err = buf;
	}
	return code;
}

#define HIP_TRY(ctx, expr)                                                                       \
	do {                                                                                         \
		hipError_t e_ = (expr);                                                                  \
		if (e_ != hipSuccess) {                                                                  \
			return fail((ctx), NTEDIT_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_));         \
		}                                                                                        \
	} while (0)

int
ensure(ntedit_hip_ctx* c, DevBuf& b, size_t bytes)
{
	if (bytes <= b.cap) {
		return 0;
	}
	const auto t0 = std::chrono::steady_clock::now();
	if (b.p) {
		HIP_TRY(c, hipFree(b.p));
		b.p = nullptr;
		b.cap = 0;
	}
	size_t want = bytes + bytes / 8 + 256;
	HIP_TRY(c, hipMalloc(&b.p, want));
	b.cap = want;
	const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	c->alloc_ms += ms;
	c->alloc_calls++;
	if (ms > 1.0 && getenv("NTEDIT_HIP_DEBUG")) {
		fprintf(stderr, "[ntedit_hip] device buffer of %.1f MB: %.2f ms of hipFree + hipMalloc\n", want / 1e6, ms);
	}
	return 0;
}

// the events of a fixed array that do not exist yet (the arrays of the reports are filled by the first call that times one)
int
ensure_event(ntedit_hip_ctx* c, hipEvent_t& e)
{
	if (!e) {
		HIP_TRY(c, hipEventCreate(&e));
	}
	return 0;
}

int
ensure_event(ntedit_hip_ctx* c, EventPair& p)
{
	int rc = ensure_event(c, p.begin);
	return rc ? rc : ensure_event(c, p.end);
}

template<class E, size_t N>
int
ensure_events(ntedit_hip_ctx* c, E (&evs)[N])
{
	for (E& e : evs) {
		int rc = ensure_event(c, e);
		if (rc) {
			return rc;
		}
	}
	return 0;
}

// a list that grows with the batch (two events per pipeline chunk): at least `count` events
int
ensure_events(ntedit_hip_ctx* c, std::vector<hipEvent_t>& evs, size_t count)
{
	while (evs.size() < count) {
		hipEvent_t e;
		HIP_TRY(c, hipEventCreate(&e));
		evs.push_back(e);
	}
	return 0;
}

template<class E, size_t N>
void
destroy_events(E (&evs)[N])
{
	for (E& e : evs) {
		destroy_event(e);
	}
}

// the best fit for `bytes` among a pool's buffers, taken out of the pool (false: none holds that much); under pin_mu
bool
pool_best_fit(std::vector<PinBuf>& pool, size_t bytes, PinBuf* out)
{
	int best = -1;
	for (size_t i = 0; i < pool.size(); i++) {
		if (pool[i].cap >= bytes && (best < 0 || pool[i].cap < pool[best].cap)) {
			best = (int)i;
		}
	}
	if (best < 0) {
		return false;
	}
	*out = pool[best];
	pool.erase(pool.begin() + best);
	return true;
}

// a new page-locked buffer for `bytes`, with a quarter to spare
int
pin_alloc(ntedit_hip_ctx* c, size_t bytes, PinBuf* out)
{
	const size_t want = bytes + bytes / 4 + 4096;
	void* p = nullptr;
	HIP_TRY(c, hipHostMalloc(&p, want, hipHostMallocDefault));
	out->p = p;
	out->cap = want;
	return 0;
}

int
pin_take(ntedit_hip_ctx* c, size_t bytes, PinBuf* out)
{
	std::lock_guard<std::mutex> lk(c->pin_mu); // results are freed from other threads
	if (pool_best_fit(c->pin_pool, bytes, out)) {
		return 0;
	}
	// drop the oldest pooled buffer if the pool is getting large
	if (c->pin_pool.size() >= 4) {
		(void)hipHostFree(c->pin_pool.front().p);
		c->pin_pool.erase(c->pin_pool.begin());
	}
	return pin_alloc(c, bytes, out);
}

void
pin_give(ntedit_hip_ctx* c, PinBuf& b)
{
	if (!b.p) {
		return;
	}
	if (c && ctx_alive(c)) {
		std::lock_guard<std::mutex> lk(c->pin_mu);
		c->pin_pool.push_back(b);
	} else {
		(void)hipHostFree(b.p);
	}
	b.p = nullptr;
	b.cap = 0;
}

// The page-locked buffers of the BGZF members have a pool of their own: in pin_pool the best-fit rule would hand the
// buffers that ntedit_hip_reserve sized for the members to the arena copies, and a batch would pin a new one.
int
bgzf_pin_take(ntedit_hip_ctx* c, size_t bytes, PinBuf* out)
{
	{
		std::lock_guard<std::mutex> lk(c->pin_mu);
		if (pool_best_fit(c->rep.bz.pool, bytes, out)) {
			return 0;
		}
	}
	return pin_alloc(c, bytes, out);
}

void
bgzf_pin_give(ntedit_hip_ctx* c, PinBuf& b)
{
	if (!b.p) {
		return;
	}
	bool kept = false;
	if (c && ctx_alive(c)) {
		std::lock_guard<std::mutex> lk(c->pin_mu);
		std::vector<PinBuf>& pool = c->rep.bz.pool;
		if (pool.size() >= 3) { // (the smallest goes: the pool keeps what the largest batches need)
			size_t least = 0;
			for (size_t i = 1; i < pool.size(); i++) {
				if (pool[i].cap < pool[least].cap) {
					least = i;
				}
			}
			if (pool[least].cap < b.cap) {
				std::swap(pool[least], b);
			}
		} else {
			pool.push_back(b);
			kept = true;
		}
	}
	if (!kept) {
		(void)hipHostFree(b.p);
	}
	b.p = nullptr;
	b.cap = 0;
}

Filter
dev_filter(const DevFilter& f)
{
	Filter r;
	r.data = f.data;
	filter_set_size(r, f.counting ? f.nbytes : f.nbytes * 8); // counters vs bits
	r.hash_num = f.hash_num;
	r.counting = f.counting ? 1 : 0;
	return r;
}

int
refresh_params(ntedit_hip_ctx* c)
{
	const DevFilter& f = c->filt[0];
	if (!f.set) {
		return fail(c, NTEDIT_E_NOFILTER, "primary Bloom filter not set");
	}
	const DevFilter& r = c->filt[1];
	if (r.set) {
		if (r.k != f.k) {
			// ntedit.cpp:2581-2585
			return fail(
			    c,
			    NTEDIT_E_ARG,
			    "secondary Bloom filter k size (%u) is different than main Bloom filter k size (%u)",
			    r.k,
			    f.k);
		}
	}
	int rc = nte_host::make_dev_params(c->hp, f.k, f.hash_num, r.set, &c->dp, f.counting);
	if (rc) {
		return fail(c, rc, "unsupported parameter combination (k=%u h=%u)", f.k, f.hash_num);
	}
#ifdef NTE_ABLATION
	if (const char* e = getenv("NTEDIT_HIP_MACHINE_DEBUG")) {
		c->dp.debug_stop = (u32)atoi(e); // timing ablations; results are NOT valid (ablation build only)
	}
#endif
	auto tuned = [](u32 knob, u32& param) { // tuning / tests (any value gives the same results)
		if (knob != ~0u) {
			param = knob;
		}
	};
	tuned(c->tune.inline_tries, c->dp.inline_tries);
	tuned(c->tune.lanes, c->dp.lanes);
	tuned(c->tune.defer_run, c->dp.defer_run);
	tuned(c->tune.defer_fail, c->dp.defer_fail);
	tuned(c->tune.defer_fail_snv, c->dp.defer_fail_snv);
	if (!c->d_tab) {
		HIP_TRY(c, hipMalloc((void**)&c->d_tab, TAB_WORDS * sizeof(u64)));
	}
	if (c->tab_k != f.k) {
		u64 tab[TAB_WORDS];
		build_seed_tables(f.k, tab);
		HIP_TRY(c, hipMemcpy(c->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
		c->tab_k = f.k;
	}
	c->dp_valid = true;
	return 0;
}

#include "nte_api_screen.inc"

} // namespace

#include "nte_api_reports.inc"
#include "nte_api_filters.inc"
#include "nte_api_polish.inc"
#include "nte_api_apply.inc"
#include "nte_api_results.inc"
