// nte_api_polish.inc -- part of nte_api.hip: ntedit_hip_polish_batch in stages (plan, screening, run map, event rounds,
// collection of the edit records, resolution of parked events, the hand-off to the apply stage), and ntedit_hip_reserve.
// ---- ntedit_hip_polish_batch, in stages --------------------------------------------------------------------
// plan()              chunk plan (whole contigs per pipeline chunk), staging of the batch, grow-only buffers
// launch_screening()  stream A: step 1 for every k-mer of the batch (direct or binned; H2D pieces underneath)
// run_chunk_events()  stream B, per chunk: absent bitmap -> ordered event list -> the event machine in rounds
// collect()           edit records to page-locked host memory; events parked by the budget are resolved in serial
//                     order and re-run (host/resolve.h)
// finish()            timings
// apply()             returns at once unless a report is on; else hands the batch to the apply stage (nte_api_apply.inc: the
//                     device applier, the reports behind it, the interval extractor's host side, the BGZF hand-off)
namespace {

// k_settle runs on lists of at least this many events.  It costs a launch, a stream synchronisation and the read-back of
// the rest count, and a short list is bound by the latency of its slowest events either way: measured on the i.i.d.
// draft (k_settle on against off, ms per step) lists of 29 k / 59 k / 117 k events lose 0.39 / 0.39 / 0.30 ms, 292 k
// events in contigs of 100 kbp lose 0.15, 440 k gain 0.12 and 3.26 M gain 3.9: break-even at about 350 k (DESIGN.md 8,
// experiment 65)
#ifndef NTE_SETTLE_MIN_EVENTS
#define NTE_SETTLE_MIN_EVENTS 400000u
#endif
constexpr unsigned NTE_RESOLVE_ROUNDS = 6; // rounds of one-parked-event-per-contig re-runs before the re-runs are widened (collect())

struct PolishRun
{
	// the call
	ntedit_hip_ctx* c;
	const char* bases;
	u64 n;
	const uint64_t* offsets;
	const uint32_t* lens;
	u32 n_contigs;
	int on_device;
	ntedit_hip_result* r;
	const std::vector<std::string>* fa_names = nullptr; // NTEDIT_HIP_APPLY_BGZF: the entries' header lines

	// plan
	struct Chunk
	{
		u32 c0, c1; // contigs [c0, c1)
		u64 b0, b1; // byte range of those contigs (incl. their separators)
		u64 t0, t1; // screening tiles
	};
	std::vector<Chunk> chunks;
	size_t n_ch = 0;
	bool pipelined = false;
	u64 n_words = 0;
	const u8* d_seq = nullptr;
	u64* d_bitmap = nullptr;
	u64* d_runmap = nullptr;  // = d_bitmap unless k_assess runs
	bool use_assess = false;
	bool candmap_used = false; // -s 1: k_assess ran with the candidate map
	bool counts_fit = true;   // Machine::lane_counts_fit() for this configuration
	float ms_assess = 0.f;
	hipStream_t sA = nullptr; // screening
	hipStream_t sB = nullptr; // event extraction + event machine (and H2D pieces while the screening runs)
	u32 grid = 0;
	u64 grid_lo = 0;
	Filter f0;
	size_t screen_pad = 0;
	u64 h2d_piece = 0;
	bool h2d_overlap = false;
	u64 arena_chunks = 0;

	// one attempt (the batch is run again with more room when the arena or a rope window overflows)
	PinBuf early; // pass-1 edit records copied to the host while the sweeps run
	u64 early_chunks = 0;
	u32 h2d_launches = 0;
	u32 status = 0;
	u64 ev_total = 0, absent_total = 0, deferred_total = 0, skipped_total = 0;
	float ms_machine = 0.f;
	bool first_b = true;
	MachineArgs keep_a; // the last chunk's launch arguments (re-runs of parked events)
	// counters layout (bytes): [0] absent k-mers u64, [8] starts of the current chunk u64, [32] arena cursor u32,
	// [40] status u32, [44] deferred count u32, [52] parked events u32, [60] work counter u32, [64] round list length u32,
	// [72] rest list length u32 (k_settle)
	unsigned long long* d_counters = nullptr;
	u32 *d_arena_next = nullptr, *d_status = nullptr, *d_ndef = nullptr, *d_list_n = nullptr;

	PolishRun()
	{
		early.p = nullptr;
		early.cap = 0;
		memset(&keep_a, 0, sizeof keep_a);
	}

	// a failure from anywhere: nothing may leak (an early copy may still be in flight), *out stays null
	int bail(int code)
	{
		(void)hipDeviceSynchronize();
		pin_give(c, early);
		pin_give(c, r->arena_buf);
		pin_give(c, r->first_buf);
		delete r;
		r = nullptr;
		return code;
	}

	int plan();
	int begin_attempt();
	int launch_screening(int attempt);
	int launch_assess(u64 pos_begin, u64 pos_end, hipStream_t s = nullptr);
	void launch_wave_pass(MachineArgs a, const u32* list, u32 count);
	int extract_events(size_t j, u64* n_ev_out, u64** d_events_out, u32** d_first_out);
	int machine_setup(u64 n_ev, u64* d_events, u32* d_first, MachineArgs* out, u64* blocks_out, size_t* dyn_lds_out);
	int run_chunk_events(size_t j);
	int collect(bool* redo);
	int finish();
	int apply();
};

// what the apply stage (nte_api_apply.inc) reads from the polish of a batch
struct ApplyInput
{
	ntedit_hip_ctx* c;
	ntedit_hip_result* r;
	const u8* d_seq; // the batch in HBM: n bytes, n_words bitmap words, n_contigs entries (c->offs, c->lens)
	u64 n, n_words;
	u32 n_contigs;
	const u64* d_bitmap; // step 1's answer
	Filter f0;
	u64 n_events; // the events of the batch (c->arena, c->first_chunk; r->arena_items)
	const std::vector<std::string>* fa_names; // NTEDIT_HIP_APPLY_BGZF: the entries' header lines
};
int apply_stage(const ApplyInput& in);

int
PolishRun::plan()
{
	int rc;
	n_words = (n + 63) / 64;
	// A batch that arrives in host memory crosses PCIe in pieces while the pieces that are already in HBM are
	// being screened (SURVEY 8d "kernel region": host buffer in, edit records out).  Page-locked buffers
	// (ntedit_hip_host_alloc, or any hipHostMalloc / registered memory) copy asynchronously at link speed;
	// pageable ones are staged by the runtime, the overlap is the same.
	h2d_piece = 32ull << 20; // (3 Gbp host batch -> records: pieces of 128 / 64 / 32 MiB 139.5 / 137.2 / 136.3 ms; round 6)
	if (on_device == NTEDIT_HIP_BASES_PACKED) {
		h2d_piece = 128ull << 20; // (a packed piece is two copies and a k_unpack launch: 94 pieces of 32 MiB 154.3 ms, 24 of 128 MiB 137.5)
	}
	if (c->tune.h2d_piece != ~0ULL) { // tests / tuning: bytes per piece (0 = one copy up front)
		h2d_piece = c->tune.h2d_piece / SCREEN_TILE * SCREEN_TILE;
	}
	h2d_overlap = on_device != NTEDIT_HIP_BASES_DEVICE && h2d_piece > 0 && n > 2 * h2d_piece;
	if ((rc = stage_bases(c, bases, n, on_device, &d_seq, !h2d_overlap))) {
		return rc;
	}
	if ((rc = ensure(c, c->bitmap, (n_words + 8) * 8)) || (rc = ensure(c, c->counters, 256))) {
		return rc;
	}
	d_bitmap = (u64*)c->bitmap.p;
	d_runmap = d_bitmap;
	// (the words behind the batch: the machine's look-ahead -- defer_run -- may read up to 8 positions past the end, and
	// what it finds there decides which kernel runs an event)
	HIP_TRY(c, hipMemsetAsync(d_bitmap + n_words, 0, 8 * 8, c->stream));
	sA = c->stream;
	sB = c->stream2;
	if ((rc = upload_entries(c, sA, offsets, lens, n_contigs))) {
		return rc;
	}

	// ---- chunk plan: whole contigs, cut at SCREEN_TILE boundaries of the screening pass.
	// Chunk j's screening covers tiles [t0, t1) with t1 = ceil(end of its last contig / TILE),
	// so everything its events can touch has been screened when its screening launch ends.
	{
		const u64 total_tiles = (n + SCREEN_TILE - 1) / SCREEN_TILE;
		// Measured (3 Gbp, MI355X): overlapping the event machine of chunk j with the screening
		// of chunk j+1 does not pay -- both are bound by the L2-miss path, the machine kernels
		// just get slower (2 chunks 339 ms, 8 chunks 370 ms vs 331 ms for one) -- so the
		// default is a single chunk; the chunk pipeline stays available (and tested) for
		// bounded-memory operation.
		u64 target = n + 1;
		if (c->tune.chunk_bytes) { // tests: force many chunks
			target = c->tune.chunk_bytes;
		}
		u32 c0 = 0;
		u64 t_prev = 0;
		while (c0 < n_contigs) {
			u32 c1 = c0;
			const u64 b0 = offsets[c0];
			u64 b1 = b0;
			while (c1 < n_contigs && (c1 == c0 || offsets[c1] + lens[c1] + 1 - b0 <= target)) {
				b1 = c1 + 1 < n_contigs ? offsets[c1 + 1] : n;
				c1++;
			}
			Chunk ch;
			ch.c0 = c0;
			ch.c1 = c1;
			ch.b0 = c0 == 0 ? 0 : b0;
			ch.b1 = b1;
			ch.t0 = t_prev;
			ch.t1 = c1 == n_contigs ? total_tiles : (b1 + SCREEN_TILE - 1) / SCREEN_TILE;
			if (ch.t1 < ch.t0) {
				ch.t1 = ch.t0;
			}
			t_prev = ch.t1;
			chunks.push_back(ch);
			c0 = c1;
		}
	}
	n_ch = chunks.size();
	pipelined = n_ch > 1;
	if ((rc = ensure_events(c, c->chunk_ev, 2 * n_ch))) {
		return rc;
	}
	grid = c->dp.start_grid;
	grid_lo = 0;
	if (grid < 64) {
		for (u32 b = 0; b < 64; b += grid) {
			grid_lo |= 1ULL << b;
		}
	}
	f0 = dev_filter(c->filt[0]);
	// the run map (nte_assess.hip): where most absent positions cannot do anything -- every position is "absent" with
	// -s 1, a quarter of them with a counting filter and -p 2 -- they are taken out before the event machine sees them
	// (its per-lane step 2 keeps at most 32 counts: Machine::lane_counts_fit)
	counts_fit = !(c->dp.snv || c->dp.counting) || (c->dp.k - 1) / c->dp.jump + 1 <= 32;
	use_assess = n_ch == 1 && counts_fit && (c->tune.assess == 1 || (c->tune.assess == ~0u && (c->dp.snv || c->dp.counting)));
	if (use_assess) {
		if ((rc = ensure(c, c->runmap, (n_words + 8) * 8))) {
			return rc;
		}
		d_runmap = (u64*)c->runmap.p;
		// (k_assess writes the words of the batch; the machine's look-ahead may read a few positions past its end)
		HIP_TRY(c, hipMemsetAsync(d_runmap + n_words, 0, 8 * 8, c->stream));
	}
	// with more than one chunk the screening kernel is held to 2 workgroups per CU (its speed
	// is set by the L2-miss path, not by occupancy) so the machine kernels of the previous
	// chunk get wave slots, registers and LDS on every CU
	screen_pad = pipelined ? 44 * 1024 : 0;
	arena_chunks = n / 160 + 65536;
	if (arena_chunks * CHUNK_ITEMS * sizeof(Item) < c->arena.cap) {
		arena_chunks = c->arena.cap / (CHUNK_ITEMS * sizeof(Item));
	}
	if (c->tune.arena_chunks) { // tests: an arena that runs out (the batch is run again with four times as much)
		arena_chunks = c->tune.arena_chunks;
	}
	return 0;
}

int
PolishRun::begin_attempt()
{
	int rc;
	pin_give(c, early); // (streams are idle here)
	early_chunks = 0;
	if (arena_chunks > 0xFFFFFFF0ull) {
		return fail(c, NTEDIT_E_OVERFLOW, "edit-record arena exceeds 2^32 chunks");
	}
	if ((rc = ensure(c, c->arena, arena_chunks * CHUNK_ITEMS * sizeof(Item)))) {
		return rc;
	}
	HIP_TRY(c, hipMemsetAsync(c->counters.p, 0, 256, sA));
	if ((rc = bin_reset(c, sA))) {
		return rc;
	}
	HIP_TRY(c, hipStreamSynchronize(sA));
	d_counters = (unsigned long long*)c->counters.p;
	d_arena_next = (u32*)((char*)c->counters.p + 32);
	d_status = (u32*)((char*)c->counters.p + 40);
	d_ndef = (u32*)((char*)c->counters.p + 44);
	d_list_n = (u32*)((char*)c->counters.p + 64);
	h2d_launches = 0;
	status = 0;
	c->settle_last = ntedit_hip_settle_stats{ 0, 0, 0.f };
	ev_total = absent_total = deferred_total = skipped_total = 0;
	ms_machine = 0.f;
	first_b = true;
	return 0;
}

// stream A: every chunk's screening, back to back
int
PolishRun::launch_screening(int attempt)
{
	int rc;
	u32 slog_unused = 0, nsl_unused = 0;
	const bool binned = binned_applicable(c, f0, n, &slog_unused, &nsl_unused);
	if (binned && !pipelined) {
		// the record buffers of the binned screening, BEFORE the first event of the timeline: a buffer that has to grow
		// costs host time (a fresh 7 GB take 160 ms, 84 GB two seconds: the driver maps and clears the pages), and
		// that time belongs neither to the screening's event window nor, after ntedit_hip_reserve, to the call at all
		u64 chunk_unused = 0;
		if ((rc = binned_buffers(c, f0, n, nsl_unused, probe_parts_log2(c, f0, slog_unused), &chunk_unused))) {
			return rc;
		}
	}
	HIP_TRY(c, hipEventRecord(c->ev[0], sA));
	const u64 n_pieces = h2d_piece ? (n + h2d_piece - 1) / h2d_piece : 0;
	if (h2d_overlap && attempt == 0) {
		while (c->h2d_ev.size() < n_pieces) {
			hipEvent_t e;
			HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
			c->h2d_ev.push_back(e);
		}
	}
	hipStream_t s_copy = sB;
	auto copy_piece = [&](u64 j) -> hipError_t {
		const u64 o = j * h2d_piece, len = o + h2d_piece < n ? h2d_piece : n - o;
		if (on_device == NTEDIT_HIP_BASES_PACKED) {
			if (copy_packed_piece(c, bases, n, o, len, s_copy)) {
				return hipErrorUnknown;
			}
			return hipEventRecord(c->h2d_ev[j], s_copy);
		}
		hipError_t e = hipMemcpyAsync((char*)c->seq.p + o, bases + o, len, hipMemcpyHostToDevice, s_copy);
		return e != hipSuccess ? e : hipEventRecord(c->h2d_ev[j], s_copy);
	};
	if (!pipelined && h2d_overlap && attempt == 0 && !binned) {
		// direct kernel: piece j+1 is copied (stream B is idle until the screening is done) while piece j is
		// screened; the tiles of piece j read k-1 bases of piece j+1, so their launch waits for that copy
		HIP_TRY(c, hipEventRecord(c->chunk_ev[0], sA));
		HIP_TRY(c, copy_piece(0));
		const u64 tiles_per_piece = h2d_piece / SCREEN_TILE;
		const u64 total_tiles = (n + SCREEN_TILE - 1) / SCREEN_TILE;
		for (u64 j = 0; j < n_pieces; j++) {
			if (j + 1 < n_pieces) {
				HIP_TRY(c, copy_piece(j + 1));
			}
			HIP_TRY(c, hipStreamWaitEvent(sA, c->h2d_ev[j + 1 < n_pieces ? j + 1 : j], 0));
			const u64 t0 = j * tiles_per_piece;
			const u64 t1 = j + 1 < n_pieces ? t0 + tiles_per_piece : total_tiles;
			if ((rc = launch_screen_tiles<false>(c, sA, d_seq, n, f0, d_bitmap, n_words, t0, t1 - t0, 0))) {
				return rc;
			}
			h2d_launches++;
		}
		if ((rc = launch_assess(0, n))) {
			return rc;
		}
		HIP_TRY(c, hipEventRecord(c->chunk_ev[1], sA));
	} else if (!pipelined) {
		c->h2d_piece_bytes = 0;
		if (h2d_overlap && attempt == 0) {
			// the binned pipeline: all pieces are queued on stream B right away (page-locked memory: truly
			// asynchronous, at link speed) and every record chunk waits for its own bases only; a retry
			// finds the batch in HBM already
			for (u64 j = 0; j < n_pieces; j++) {
				HIP_TRY(c, copy_piece(j));
			}
			c->h2d_piece_bytes = h2d_piece;
			c->h2d_pieces = n_pieces;
		}
		HIP_TRY(c, hipEventRecord(c->chunk_ev[0], sA));
		rc = launch_screen<false>(c, d_seq, n, f0, d_bitmap, n_words);
		c->h2d_piece_bytes = 0;
		if (rc || (rc = launch_assess(0, n))) {
			return rc;
		}
		HIP_TRY(c, hipEventRecord(c->chunk_ev[1], sA));
	} else {
		c->h2d_piece_bytes = 0;
		if (h2d_overlap && attempt == 0) {
			// the pieces cross on a stream of their own (stream B runs the event machine of the chunks that are
			// through), every chunk's screening waits for its own bases
			if (!c->stream_copy) {
				HIP_TRY(c, hipStreamCreate(&c->stream_copy));
			}
			s_copy = c->stream_copy;
			HIP_TRY(c, hipStreamWaitEvent(s_copy, c->ev[0], 0)); // (behind whatever the earlier work on stream A still reads)
			for (u64 j = 0; j < n_pieces; j++) {
				HIP_TRY(c, copy_piece(j));
			}
			c->h2d_piece_bytes = h2d_piece;
			c->h2d_pieces = n_pieces;
		}
		u32 slog = 0, nsl = 0;
		const bool bin_chunks = binned_applicable(c, f0, n, &slog, &nsl);
		if (!bin_chunks) {
			c->bin_chunks_last = 0;
		}
		for (size_t j = 0; j < n_ch; j++) {
			HIP_TRY(c, hipEventRecord(c->chunk_ev[2 * j], sA));
			if (c->h2d_piece_bytes && !bin_chunks) {
				u64 piece = (chunks[j].t1 * SCREEN_TILE + SCREEN_TILE) / c->h2d_piece_bytes;
				piece = piece < n_pieces ? piece : n_pieces - 1;
				HIP_TRY(c, hipStreamWaitEvent(sA, c->h2d_ev[piece], 0));
			}
			if (bin_chunks) {
				// (the probe stage of chunk j+1 leaves room on the CUs for the event machine of chunk j)
				const u64 p0 = chunks[j].t0 * SCREEN_TILE, p1 = chunks[j].t1 * SCREEN_TILE;
				if (p1 > p0 && (rc = run_screen_binned(c, d_seq, n, f0, d_bitmap, n_words, slog, nsl, sA, p0, p1 < n ? p1 : n))) {
					return rc;
				}
			} else if ((rc = launch_screen_tiles<false>(
			                c, sA, d_seq, n, f0, d_bitmap, n_words, chunks[j].t0, chunks[j].t1 - chunks[j].t0, screen_pad))) {
				return rc;
			}
			HIP_TRY(c, hipEventRecord(c->chunk_ev[2 * j + 1], sA));
		}
		c->h2d_piece_bytes = 0;
	}
	HIP_TRY(c, hipEventRecord(c->ev[1], sA));
	return 0;
}

// stream A, behind the screening of [pos_begin, pos_end): the run map of those positions
int
PolishRun::launch_assess(u64 pos_begin, u64 pos_end, hipStream_t s)
{
	if (!use_assess || pos_end <= pos_begin) {
		return 0;
	}
	const bool again = s != nullptr; // (behind a recovered record chunk, on stream B: not timed a second time)
	if (!s) {
		s = sA;
	}
	AssessArgs a;
	a.seq = d_seq;
	a.n_bytes = n;
	a.bitmap = d_bitmap;
	a.runmap = d_runmap;
	a.tabs = c->d_tab;
	a.p = c->dp;
	a.bloom = f0;
	a.rep = c->filt[1].set ? dev_filter(c->filt[1]) : f0;
	a.pos_begin = pos_begin;
	a.pos_end = pos_end;
	const u64 tile = (u64)assess_tile();
	a.n_tiles = (pos_end - pos_begin + tile - 1) / tile;
	a.cand_map = nullptr;
	{
		// -s 1 on a plain filter (round 6): the first probes of every position's substitution candidates through the
		// partitioned pipeline (nte_bin_wc.inc MODE 1) instead of three random gathers per position inside k_assess
		u32 cslog = 0, cnsl = 0;
		if (!again && pos_begin == 0 && pos_end == n && candmap_applicable(c, f0, n, &cslog, &cnsl)) {
			int rc;
			const u64 cwords = (n * 4 + 63) / 64;
			if ((rc = ensure(c, c->candmap, (cwords + 8) * 8))) {
				return rc;
			}
			HIP_TRY(c, hipEventRecord(c->ev_assess[0], s));
			if ((rc = run_screen_binned(c, d_seq, n, f0, (u64*)c->candmap.p, cwords, cslog, cnsl, s, 0, n, true))) {
				return rc;
			}
			// (a chunk whose overflow list ran out: its part of the map becomes "unknown" -- before k_assess reads it)
			u32 recovered = 0;
			if ((rc = bin_recover(c, s, d_seq, n, f0, d_bitmap, n_words, 0, n, &recovered))) {
				return rc;
			}
			a.cand_map = (const u32*)c->candmap.p;
			candmap_used = true;
		}
	}
	const u64 cap = (u64)c->cu_count * 32;
	if (!again && !a.cand_map) {
		HIP_TRY(c, hipEventRecord(c->ev_assess[0], s));
	}
	if (again && candmap_used) {
		a.cand_map = (const u32*)c->candmap.p; // (the map does not depend on the screening that was repeated)
	}
	launch_k_assess((unsigned)(a.n_tiles < cap ? a.n_tiles : cap), s, a);
	HIP_TRY(c, hipGetLastError());
	if (!again) {
		HIP_TRY(c, hipEventRecord(c->ev_assess[1], s));
	}
	return 0;
}

// the wavefront-per-event kernel over a list of events of the current chunk
void
PolishRun::launch_wave_pass(MachineArgs a, const u32* list, u32 count)
{
	hipStream_t stream = sB;
	const u32 blocks_per_cu = 8;
	a.defer = 0;
	a.ev_list = list;
	a.n_events = count;
	a.win_bytes += 64; // (one shared window for the positions of 64 lanes, run_lanes)
	const u64 per_block = (u64)MACHINE_TPB / (u64)machine_wave_group();
	const u64 want2 = ((u64)count + per_block - 1) / per_block;
	const u64 cap2 = (u64)c->cu_count * blocks_per_cu;
	const u64 b2 = want2 < cap2 ? want2 : cap2;
	// the wave kernel runs few events per block: window and workspace both fit in LDS
	size_t dyn2 = a.win_in_lds ? (size_t)a.win_bytes * per_block : 0;
	const u64 Wn = a.p.node_window;
	const u64 w16 = (Wn + 15) & ~15ull;
	const u64 slab = Wn * 16 + w16 * 4 + w16 * 2 + w16 + w16;
	const u64 win_area = ((u64)a.win_bytes * per_block + 15) & ~15ull;
	if (win_area + slab * per_block <= 40 * 1024) {
		a.win_in_lds = 1;
		a.lds_ws_off = (u32)win_area;
		a.lds_slab = (u32)slab;
		dyn2 = (size_t)(win_area + slab * per_block);
	}
	(void)hipMemsetAsync(a.work_counter, 0, 4, stream);
	launch_k_machine_wave((unsigned)b2, dyn2, stream, a);
}

// stream B, chunk j, as soon as its screening is done: absent bitmap -> ordered event list (count, single-workgroup
// scan, write).  *n_ev_out = its events, written behind those of the earlier chunks (d_events / d_first).
int
PolishRun::extract_events(size_t j, u64* n_ev_out, u64** d_events_out, u32** d_first_out)
{
	int rc;
	*n_ev_out = 0;
	const Chunk& ch = chunks[j];
	HIP_TRY(c, hipStreamWaitEvent(sB, c->chunk_ev[2 * j + 1], 0));
	if (first_b) {
		HIP_TRY(c, hipEventRecord(c->ev[2], sB));
		first_b = false;
	}
	const u64 w0 = ch.b0 / 64, w1 = (ch.b1 + 63) / 64;
	const u64 n_sblocks = (w1 - w0 + ST_TPB - 1) / ST_TPB;
	if (n_sblocks == 0) {
		return 0;
	}
	if ((rc = ensure(c, c->block_counts, n_sblocks * 2 * 4)) || (rc = ensure(c, c->block_offsets, n_sblocks * 8))) { // (counts, absent k-mers)
		return rc;
	}
	unsigned long long h_counters[2] = { 0, 0 };
	for (int pass = 0;; pass++) {
		HIP_TRY(c, hipMemsetAsync((char*)c->counters.p + 8, 0, 8, sB));
		hipLaunchKernelGGL(
		    k_count_starts, dim3((unsigned)n_sblocks), dim3(ST_TPB), 0, sB, d_runmap, w0, w1, ch.b0, ch.b1, grid_lo, grid,
		    (u32*)c->block_counts.p, (const u64*)d_bitmap);
		hipLaunchKernelGGL(
		    k_scan_counts, dim3(1), dim3(1024), 0, sB, (const u32*)c->block_counts.p, n_sblocks,
		    (unsigned long long*)c->block_offsets.p, d_counters);
		HIP_TRY(c, hipMemcpyAsync(h_counters, d_counters, 16, hipMemcpyDeviceToHost, sB));
		if (pass == 0 && c->bin_chunks_last) {
			// Record chunks of this range whose overflow list ran out (a draft of very few distinct k-mers): their
			// part of the bitmap is void.  The direct kernel screens them again, here, BEFORE anything is made of the
			// bitmap -- the chunk, not the batch; the counts above are taken again.  (The flags come back with the
			// counters: one synchronisation in the ordinary case.)
			u32 recovered = 0;
			const u64 p0 = pipelined ? ch.t0 * SCREEN_TILE : 0, p1 = pipelined ? ch.t1 * SCREEN_TILE : n;
			if ((rc = bin_recover(c, sB, d_seq, n, f0, d_bitmap, n_words, p0, p1, &recovered))) {
				return rc;
			}
			if (recovered) {
				if ((rc = launch_assess(0, n, sB))) { // (the run map read the void bitmap)
					return rc;
				}
				continue;
			}
		}
		HIP_TRY(c, hipStreamSynchronize(sB));
		break;
	}
	const u64 n_ev = h_counters[1];
	absent_total = h_counters[0];
	if (n_ev == 0) {
		return 0;
	}
	if (ev_total + n_ev > 0xFFFFFFF0ull) {
		return fail(c, NTEDIT_E_OVERFLOW, "more than 2^32 events in one batch");
	}
	// grow-only buffers; (re)allocation happens on the first batches only
	if (ev_total + n_ev > c->events.cap / 8 || ev_total + n_ev > c->first_chunk.cap / 4) {
		// keep what earlier chunks wrote: allocate bigger buffers and copy
		const u64 want = (ev_total + n_ev) * 2 + 1024;
		DevBuf ne, nf;
		if ((rc = ensure(c, ne, want * 8)) || (rc = ensure(c, nf, want * 4))) {
			return rc;
		}
		if (ev_total) {
			HIP_TRY(c, hipMemcpyAsync(ne.p, c->events.p, ev_total * 8, hipMemcpyDeviceToDevice, sB));
			HIP_TRY(c, hipMemcpyAsync(nf.p, c->first_chunk.p, ev_total * 4, hipMemcpyDeviceToDevice, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
		}
		release(c->events);
		release(c->first_chunk);
		c->events = ne;
		c->first_chunk = nf;
	}
	if ((rc = ensure(c, c->deferred, n_ev * 4))) {
		return rc;
	}
	u64* d_events = (u64*)c->events.p + ev_total;
	u32* d_first = (u32*)c->first_chunk.p + ev_total;
	hipLaunchKernelGGL(
	    k_write_starts, dim3((unsigned)n_sblocks), dim3(ST_TPB), 0, sB, d_runmap, w0, w1, ch.b0, ch.b1, grid_lo, grid,
	    (const unsigned long long*)c->block_offsets.p, d_events);
	*n_ev_out = n_ev;
	*d_events_out = d_events;
	*d_first_out = d_first;
	return 0;
}

// the machine's launch arguments and per-thread workspace for a chunk of n_ev events
int
PolishRun::machine_setup(u64 n_ev, u64* d_events, u32* d_first, MachineArgs* out, u64* blocks_out, size_t* dyn_lds_out)
{
	int rc;
	const u64 max_threads = (u64)c->cu_count * 2048;
	u64 threads = n_ev < max_threads ? n_ev : max_threads;
	const u64 blocks = (threads + MACHINE_TPB - 1) / MACHINE_TPB;
	threads = blocks * MACHINE_TPB;
	const u64 W = c->dp.node_window;
	if ((rc = ensure(c, c->ws_nodes, threads * W * sizeof(Node))) || (rc = ensure(c, c->ws_ov_pos, threads * W * 4)) ||
	    (rc = ensure(c, c->ws_ov_chr, threads * W)) || (rc = ensure(c, c->ws_prev, threads * W)) ||
	    (rc = ensure(c, c->ws_lps, threads * W * 2))) {
		return rc;
	}
	MachineArgs a;
	a.seq = d_seq;
	a.n_bytes = n;
	a.offsets = (const u64*)c->offs.p;
	a.lens = (const u32*)c->lens.p;
	a.n_contigs = n_contigs;
	a.bitmap = d_bitmap;
	a.runmap = d_runmap;
	a.events = d_events;
	a.n_events = n_ev;
	a.tabs = c->d_tab;
	a.p = c->dp;
	a.bloom = f0;
	a.rep = c->filt[1].set ? dev_filter(c->filt[1]) : f0;
	a.ws_nodes = (Node*)c->ws_nodes.p;
	a.ws_ov_pos = (u32*)c->ws_ov_pos.p;
	a.ws_ov_chr = (u8*)c->ws_ov_chr.p;
	a.ws_prev = (u8*)c->ws_prev.p;
	a.ws_lps = (int16_t*)c->ws_lps.p;
	a.win_bytes = 2 * c->dp.k + c->dp.max_deletions + 8 + 32; // Machine::win_bytes() + slack
	a.win_in_lds = (size_t)a.win_bytes * MACHINE_TPB <= 40 * 1024 ? 1 : 0;
	a.ws_win = nullptr;
	if (!a.win_in_lds) {
		if ((rc = ensure(c, c->ws_win, threads * (a.win_bytes + 64)))) { // (+ 64: the wavefront-per-event launch, launch_wave_pass)
			return rc;
		}
		a.ws_win = (u8*)c->ws_win.p;
	}
	const size_t dyn_lds = a.win_in_lds ? (size_t)a.win_bytes * MACHINE_TPB : 0;
	a.arena = (Item*)c->arena.p;
	a.arena_next = d_arena_next;
	a.arena_chunks = (u32)arena_chunks;
	a.first_chunk = d_first;
	a.status = d_status;
	a.lds_ws_off = 0;
	a.lds_slab = 0;
	a.defer = 1;
	a.ev_list = nullptr;
	a.deferred = (u32*)c->deferred.p;
	a.n_deferred = d_ndef;
	a.n_unfinished = (u32*)((char*)c->counters.p + 52);
	a.work_counter = (u32*)((char*)c->counters.p + 60);
	if (n_ch != 1) {
		a.p.event_budget = 0; // (parked events are re-run per batch: single-chunk batches only)
	}
	a.cfg = c->tune.machine_cfg != ~0u ? c->tune.machine_cfg : machine_cfg_pick(a);
	*out = a;
	*blocks_out = blocks;
	*dyn_lds_out = dyn_lds;
	return 0;
}

// stream B, chunk j: its events through the event machine, in rounds
int
PolishRun::run_chunk_events(size_t j)
{
	int rc;
	const Chunk& ch = chunks[j];
	u64 n_ev = 0;
	u64* d_events = nullptr;
	u32* d_first = nullptr;
	if ((rc = extract_events(j, &n_ev, &d_events, &d_first)) || n_ev == 0) {
		return rc;
	}
	MachineArgs a;
	u64 blocks = 0;
	size_t dyn_lds = 0;
	if ((rc = machine_setup(n_ev, d_events, d_first, &a, &blocks, &dyn_lds))) {
		return rc;
	}

	// ---- rounds (see "event rounds" in nte_kernels.hip): primaries, then the secondaries their
	// primary's run does not overtake, then -- practically never -- whatever a verification rejects.
	// SNV mode runs everything in one round.
	// Rounds pay when the events outnumber the machine's threads several times over (3 Gbp: 4.4 M events, 42 ms against 55
	// in one round); a small batch is bound by the latency of its slowest events, which every round pays again
	// (375 Mbp, 0.44 M events: 9.0 ms in rounds, 7.0 ms in one; break-even at 1.8 M events).
	const bool rounds = !c->dp.snv && n_ev < 0xFFFFFF00ull && !c->tune.no_rounds &&
	                    (c->tune.force_rounds || n_ev >= (u64)c->cu_count * 8192);
	u32* d_list = nullptr;
	u64* d_before = nullptr;
	u64* d_bmax = nullptr;
	const u32 n32 = (u32)n_ev;
	const u32 sel_blocks = (n32 + EVR_TPB - 1) / EVR_TPB;
	const u32 pm_blocks = (n32 + 1023) / 1024;
	a.ev_cover = nullptr;
	a.ev_flags = nullptr;
	// k_settle in front of the thread-per-event launches: where settle_event() restates the machine (nte_settle.h)
	// (no list of a batch is longer than n_ev: a batch below the minimum needs no rest list)
	const bool settle = c->tune.settle != 0 && settle_applicable(a.p, a.bloom) && !c->filt[1].set && n_ev < 0xFFFFFF00ull &&
	                    (c->tune.settle == 1 || n_ev >= NTE_SETTLE_MIN_EVENTS);
	if (settle && (rc = ensure(c, c->ev_rest, n_ev * 4))) {
		return rc;
	}
	if (rounds) {
		if ((rc = ensure(c, c->ev_cover, n_ev * 8)) || (rc = ensure(c, c->ev_before, n_ev * 8)) ||
		    (rc = ensure(c, c->ev_flags, n_ev)) || (rc = ensure(c, c->ev_list, n_ev * 4)) ||
		    (rc = ensure(c, c->ev_bmax, (size_t)pm_blocks * 8 + 8))) {
			return rc;
		}
		a.ev_cover = (u64*)c->ev_cover.p;
		a.ev_flags = (u8*)c->ev_flags.p;
		d_list = (u32*)c->ev_list.p;
		d_before = (u64*)c->ev_before.p;
		d_bmax = (u64*)c->ev_bmax.p;
		HIP_TRY(c, hipMemsetAsync(a.ev_cover, 0, n_ev * 8, sB));
	}
	HIP_TRY(c, hipEventRecord(c->ev[3], sB));
	u32 n_def = 0;
	float p2_ms = 0.f;
	// one round = pass 1 over a list of events (indel sweeps postponed), pass 2 over the postponed ones
	auto run_round = [&](const u32* list, u32 count, bool first_round) -> int {
		if (count == 0) {
			return 0;
		}
		MachineArgs ra = a;
		ra.ev_list = list;
		ra.n_events = count;
		if (a.p.snv && a.p.lanes && a.p.mode == 0 && !a.p.mask && (!use_assess || c->tune.snv_wave) && counts_fit) {
			// -s 1: every position of every event is assessed, there is nothing a thread-per-event pass could settle
			// more cheaply -- all events go to the wavefront-per-event launch, 64 positions at a time (run_lanes)
			HIP_TRY(c, hipEventRecord(c->ev[5], sB));
			launch_wave_pass(ra, list, count);
			HIP_TRY(c, hipGetLastError());
			HIP_TRY(c, hipEventRecord(c->ev[2], sB));
			u32 h_t[4] = { 0, 0, 0, 0 };
			HIP_TRY(c, hipMemcpyAsync(h_t, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			status = h_t[2];
			const float t = elapsed_ms(c->ev[5], c->ev[2]);
			p2_ms += t;
			return 0;
		}
		HIP_TRY(c, hipMemsetAsync(d_ndef, 0, 4, sB));
		if (settle && (c->tune.settle == 1 || count >= NTE_SETTLE_MIN_EVENTS)) {
			// the plain substitution events of the list, settled by lanes that all ask the same question (nte_settle.hip);
			// the thread-per-event launch runs what is left
			u32* d_rest = (u32*)c->ev_rest.p;
			u32* d_nrest = (u32*)((char*)c->counters.p + 72);
			HIP_TRY(c, hipMemsetAsync(d_nrest, 0, 4, sB));
			HIP_TRY(c, hipEventRecord(c->ev_settle[0], sB));
			const u64 sw = ((u64)count + MACHINE_TPB - 1) / MACHINE_TPB, scap = (u64)c->cu_count * 16;
			launch_k_settle((unsigned)(sw < scap ? sw : scap), sB, ra, d_rest, d_nrest);
			HIP_TRY(c, hipGetLastError());
			HIP_TRY(c, hipEventRecord(c->ev_settle[1], sB));
			u32 n_rest = 0;
			HIP_TRY(c, hipMemcpyAsync(&n_rest, d_nrest, 4, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			const float t = elapsed_ms(c->ev_settle[0], c->ev_settle[1]);
			c->settle_last.ms += t;
			c->settle_last.events_seen += count;
			c->settle_last.events_settled += count - n_rest;
			ra.ev_list = d_rest;
			ra.n_events = n_rest;
		}
		if (ra.n_events) {
			HIP_TRY(c, hipMemsetAsync(ra.work_counter, 0, 4, sB));
			const u64 want = ((u64)ra.n_events + MACHINE_TPB - 1) / MACHINE_TPB;
			launch_k_machine_thread((unsigned)(want < blocks ? want : blocks), dyn_lds, sB, ra);
			HIP_TRY(c, hipGetLastError());
		}
		u32 h_tail[4] = { 0, 0, 0, 0 };
		HIP_TRY(c, hipMemcpyAsync(h_tail, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost, sB));
		HIP_TRY(c, hipEventRecord(c->ev[5], sB));
		HIP_TRY(c, hipStreamSynchronize(sB));
		const u32 nd = h_tail[3];
		n_def += nd;
		status = h_tail[2];
		if (first_round && nd > 0 && status == 0 && n_ch == 1 && !c->tune.no_early_copy) {
			// everything pass 1 wrote is final (later launches only append chunks): start moving it
			// to the host on the other stream while the sweeps run
			early_chunks = h_tail[0] < arena_chunks ? h_tail[0] : arena_chunks;
			const u64 room = early_chunks + (u64)nd * 3 + 4096;
			int prc = pin_take(c, room * CHUNK_ITEMS * sizeof(Item) + 16, &early);
			if (prc) {
				return prc;
			}
			if (early_chunks) {
				HIP_TRY(c, hipMemcpyAsync(early.p, c->arena.p, early_chunks * CHUNK_ITEMS * sizeof(Item), hipMemcpyDeviceToHost, sA));
			}
		}
		if (nd > 0 && status == 0) {
			MachineArgs a2 = ra;
#ifdef NTE_ABLATION
			if (const char* dbg = getenv("NTEDIT_HIP_PASS2_DEBUG")) {
				a2.p.debug_stop = (u32)atoi(dbg); // timing ablations; results are NOT valid (ablation build only)
			}
#endif
			launch_wave_pass(a2, (const u32*)c->deferred.p, nd);
			HIP_TRY(c, hipGetLastError());
			HIP_TRY(c, hipEventRecord(c->ev[2], sB));
			HIP_TRY(c, hipMemcpyAsync(h_tail, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			status = h_tail[2];
			const float t = elapsed_ms(c->ev[5], c->ev[2]);
			p2_ms += t;
		}
		return 0;
	};
	u32 n_A = n32, n_B = 0, n_C = 0;
	if (!rounds) {
		if ((rc = run_round(nullptr, n32, true))) {
			return rc;
		}
	} else {
		const u32 gap = c->dp.k + 16;
		auto list_count = [&](u32* out) -> int {
			HIP_TRY(c, hipMemcpyAsync(out, d_list_n, 4, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			return 0;
		};
		auto prefix_max = [&]() {
			hipLaunchKernelGGL(k_ev_prefix_max_1, dim3(pm_blocks), dim3(1024), 0, sB, (const u64*)a.ev_cover, n32, d_before, d_bmax);
			hipLaunchKernelGGL(k_ev_prefix_max_2, dim3(pm_blocks), dim3(1024), 0, sB, n32, d_before, (const u64*)d_bmax);
		};
		auto select = [&](int mode, u32* count) -> int {
			prefix_max();
			HIP_TRY(c, hipMemsetAsync(d_list_n, 0, 4, sB));
			if (mode == 0) {
				hipLaunchKernelGGL(k_ev_select<0>, dim3(sel_blocks), dim3(EVR_TPB), 0, sB, (const u64*)d_events, n32,
				                   (const u64*)a.ev_cover, (const u64*)d_before, a.ev_flags, d_first, d_list, d_list_n);
			} else {
				hipLaunchKernelGGL(k_ev_select<1>, dim3(sel_blocks), dim3(EVR_TPB), 0, sB, (const u64*)d_events, n32,
				                   (const u64*)a.ev_cover, (const u64*)d_before, a.ev_flags, d_first, d_list, d_list_n);
			}
			return list_count(count);
		};
		HIP_TRY(c, hipMemsetAsync(d_list_n, 0, 4, sB));
		hipLaunchKernelGGL(k_ev_primaries, dim3(sel_blocks), dim3(EVR_TPB), 0, sB, (const u64*)d_events, n32, gap, a.ev_flags, d_list, d_list_n);
		if ((rc = list_count(&n_A)) || (rc = run_round(d_list, n_A, true))) {
			return rc;
		}
		if (status == 0 && n_A < n32) {
			if ((rc = select(0, &n_B)) || (rc = run_round(d_list, n_B, false))) {
				return rc;
			}
			// (a run of round B that reaches a primary: that primary's secondaries cannot be taken for overtaken)
			u32 n_v = 0;
			for (int guard = 0; status == 0 && guard < 64; guard++) {
				if ((rc = select(1, &n_v))) {
					return rc;
				}
				if (n_v == 0) {
					break;
				}
				n_C += n_v;
				if ((rc = run_round(d_list, n_v, false))) {
					return rc;
				}
			}
		}
	}
	HIP_TRY(c, hipGetLastError());
	keep_a = a;
	HIP_TRY(c, hipEventRecord(c->ev[4], sB));
	u32 h_tail[4] = { 0, 0, 0, 0 };
	HIP_TRY(c, hipMemcpyAsync(h_tail, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost, sB));
	HIP_TRY(c, hipStreamSynchronize(sB));
	status = h_tail[2];
	deferred_total += n_def;
	skipped_total += rounds ? (u64)n32 - n_A - n_B - n_C : 0;
	const float p_all = elapsed_ms(c->ev[3], c->ev[4]);
	ms_machine += p_all;
	if (getenv("NTEDIT_HIP_DEBUG")) {
		fprintf(
		    stderr,
		    "[ntedit_hip] chunk %zu/%zu contigs %u-%u events %llu (round A %u, B %u, C %u; %llu skipped as overtaken) sweeps %u "
		    "machine %.3f ms (sweep launches %.3f ms) arena %u status %u window %u\n",
		    j + 1, n_ch, ch.c0, ch.c1, (unsigned long long)n_ev, n_A, n_B, n_C,
		    (unsigned long long)(rounds ? (u64)n32 - n_A - n_B - n_C : 0), n_def, p_all, p2_ms, h_tail[0], status, c->dp.node_window);
		if (c->settle_last.events_seen) {
			fprintf(stderr, "[ntedit_hip] k_settle: %llu of %llu events settled in %.3f ms\n", (unsigned long long)c->settle_last.events_settled,
			        (unsigned long long)c->settle_last.events_seen, c->settle_last.ms);
		}
		unsigned long long pr[64];
		machine_wave_profile(pr);
		const unsigned long long tg = machine_thread_gathers() + settle_gathers(); // (k_settle counts into the thread launches' figure)
		if (pr[15] || tg) {
			fprintf(stderr, "[ntedit_hip] machine filter gathers (profile build): thread-per-event launches %llu, wavefront-per-event launches %llu\n", tg, pr[15]);
		}
		for (int wv = 0; wv < 2; wv++) {
			// (profile build) the longest events of this chunk's launches: where they start, when they ran, what they covered
			static std::vector<unsigned long long> lg(4 * 8192);
			const unsigned nl = machine_evlog(wv != 0, lg.data(), 8192);
			if (!nl) {
				continue;
			}
			std::vector<unsigned> order(nl);
			unsigned long long t_min = ~0ULL, t_max = 0;
			for (unsigned q = 0; q < nl; q++) {
				order[q] = q;
				t_min = lg[4 * q + 1] < t_min ? lg[4 * q + 1] : t_min;
				t_max = lg[4 * q + 2] > t_max ? lg[4 * q + 2] : t_max;
			}
			std::sort(order.begin(), order.end(), [&](unsigned x, unsigned y) { return lg[4 * x + 2] - lg[4 * x + 1] > lg[4 * y + 2] - lg[4 * y + 1]; });
			fprintf(stderr, "[ntedit_hip] %s-per-event launches: %u events of more than 2^22 ticks, logged span %llu ticks; the longest (position: ticks, begin after the first logged begin, positions covered, flags, positions walked / failing):",
			        wv ? "wavefront" : "thread", nl, t_max - t_min);
			for (unsigned q = 0; q < nl && q < 16; q++) {
				const unsigned long long* e = &lg[4 * order[q]];
				fprintf(stderr, " %llu: %llu +%llu %llu 0x%llx %llu/%llu;", e[0], e[2] - e[1], e[1] - t_min, e[3] & 0xFFFFFFull, (e[3] >> 24) & 0xFF, (e[3] >> 32) & 0xFFFF, e[3] >> 48);
			}
			fprintf(stderr, "\n");
		}
		if (pr[8]) {
			fprintf(stderr, "[ntedit_hip] wave-kernel events by duration (log2 cycles: count):");
			for (int b = 0; b < 32; b++) {
				if (pr[32 + b]) {
					fprintf(stderr, " %d:%llu", b, pr[32 + b]);
				}
			}
			fprintf(stderr, "; longest %llu cycles, most positions in one event %llu\n", pr[13], pr[14]);
			fprintf(stderr, "[ntedit_hip] wave-kernel phase cycles/event (n=%llu): seed %llu presence %llu first-miss %llu later-miss %llu advance %llu loop %llu housekeeping %llu flush %llu; positions/event %.1f failing %.1f\n",
			    pr[8], pr[0] / pr[8], pr[1] / pr[8], pr[2] / pr[8], pr[3] / pr[8], pr[4] / pr[8], pr[5] / pr[8], pr[6] / pr[8], pr[7] / pr[8],
			    (double)pr[9] / (double)pr[8], (double)pr[10] / (double)pr[8]);
			fprintf(stderr, "[ntedit_hip]   inside failing positions: window %llu step-2 %llu substitutions (lanes: the lanes' own phases) %llu indel sweeps %llu apply %llu; advance: stride %llu roll %llu; lane batches/event %.2f lanes/batch %.1f\n",
			    pr[16] / pr[8], pr[17] / pr[8], pr[18] / pr[8], pr[20] / pr[8], pr[19] / pr[8], pr[21] / pr[8], pr[22] / pr[8],
			    (double)pr[11] / (double)pr[8], pr[11] ? (double)pr[12] / (double)pr[11] : 0.0);
		}
	}
	ev_total += n_ev;
	return 0;
}

// edit records to the host; *redo = the batch has to be run again with more room
int
PolishRun::collect(bool* redo)
{
	int rc;
	*redo = false;
	u32 h_tail[4] = { 0, 0, 0, 0 };
	HIP_TRY(c, hipMemcpy(h_tail, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost));
	const u64 used_chunks = h_tail[0] < arena_chunks ? h_tail[0] : arena_chunks;
	r->st.absent_kmers = absent_total;
	r->st.events = ev_total;
	r->st.events_deferred = deferred_total;
	r->arena_items = (size_t)used_chunks * CHUNK_ITEMS;
	u64 have = 0; // chunks already on the host
	if (early.p && early.cap >= r->arena_items * sizeof(Item) + 16) {
		r->arena_buf = early;
		early.p = nullptr;
		early.cap = 0;
		have = early_chunks;
	} else {
		pin_give(c, early);
		if ((rc = pin_take(c, r->arena_items * sizeof(Item) + 16, &r->arena_buf))) {
			return rc;
		}
	}
	if ((rc = pin_take(c, ev_total * 4 + 16, &r->first_buf))) {
		return rc;
	}
	if (used_chunks > have) {
		const size_t off = (size_t)have * CHUNK_ITEMS * sizeof(Item);
		HIP_TRY(c, hipMemcpyAsync((char*)r->arena_buf.p + off, (char*)c->arena.p + off, r->arena_items * sizeof(Item) - off, hipMemcpyDeviceToHost, sB));
	}
	if (ev_total) {
		HIP_TRY(c, hipMemcpyAsync(r->first_buf.p, c->first_chunk.p, ev_total * 4, hipMemcpyDeviceToHost, sB));
	}
	HIP_TRY(c, hipStreamSynchronize(sB));
	// Events parked by the budget: decide, in serial order, which of them are applied, re-run
	// exactly those to completion, carry on behind them (host/resolve.h).  Nothing to do in
	// the ordinary case.
	u32 n_unfinished = 0;
	HIP_TRY(c, hipMemcpy(&n_unfinished, (char*)c->counters.p + 52, 4, hipMemcpyDeviceToHost));
	if (n_unfinished && n_ch == 1) {
		nte_host::Resolver rs((const Item*)r->arena_buf.p, r->arena_items, (const u32*)r->first_buf.p, ev_total);
		std::vector<u32> rerun;
		if (!rs.start(rerun)) {
			return fail(c, NTEDIT_E_DEVICE, "malformed event records");
		}
		u64 have_chunks = used_chunks;
		unsigned rounds = 0;
		// The walk hands out one parked event per contig and round: the first one the serial order reaches.  That is
		// the cheapest plan when few events are parked (the ordinary case: a handful per 3 Gbp) or when the first
		// re-run covers its whole contig (a saturated filter), and a crawl when nearly everything is parked and
		// every run is short (a tiny budget: one launch per dependency level).  After NTE_RESOLVE_ROUNDS rounds the
		// re-runs are widened instead: ALL events still parked behind the waiting points at once, with a budget
		// that grows 16-fold per round (speculation again, bounded by that budget), until none is left.
		u32 wide_budget = keep_a.p.event_budget ? keep_a.p.event_budget : 1;
		while (!rerun.empty()) {
			const bool wide = rounds >= NTE_RESOLVE_ROUNDS;
			if (wide) {
				rerun.clear();
				rs.parked_behind(rerun);
				wide_budget = wide_budget < (1u << 26) ? wide_budget * 16u : 0u;
			}
			HIP_TRY(c, hipMemcpyAsync(c->deferred.p, rerun.data(), rerun.size() * 4, hipMemcpyHostToDevice, sB));
			MachineArgs ra = keep_a;
			ra.p.event_budget = wide ? wide_budget : 0;
			ra.ev_cover = nullptr; // (the rounds are over)
			ra.ev_flags = nullptr;
			launch_wave_pass(ra, (const u32*)c->deferred.p, (u32)rerun.size());
			HIP_TRY(c, hipGetLastError());
			u32 t2[4] = { 0, 0, 0, 0 };
			HIP_TRY(c, hipMemcpyAsync(t2, (char*)c->counters.p + 32, 16, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			if (t2[2]) {
				// a re-run ran out of arena / rope window: the whole batch again, with more room
				status = t2[2];
				*redo = true;
				pin_give(c, r->arena_buf);
				pin_give(c, r->first_buf);
				return 0;
			}
			const u64 now_chunks = t2[0] < arena_chunks ? t2[0] : arena_chunks;
			const size_t need = (size_t)now_chunks * CHUNK_ITEMS * sizeof(Item) + 16;
			if (r->arena_buf.cap < need) {
				PinBuf bigger;
				if ((rc = pin_take(c, need + need / 2, &bigger))) {
					return rc;
				}
				memcpy(bigger.p, r->arena_buf.p, (size_t)have_chunks * CHUNK_ITEMS * sizeof(Item));
				pin_give(c, r->arena_buf);
				r->arena_buf = bigger;
			}
			if (now_chunks > have_chunks) {
				const size_t off = (size_t)have_chunks * CHUNK_ITEMS * sizeof(Item);
				HIP_TRY(c, hipMemcpyAsync((char*)r->arena_buf.p + off, (char*)c->arena.p + off,
				                          (size_t)(now_chunks - have_chunks) * CHUNK_ITEMS * sizeof(Item), hipMemcpyDeviceToHost, sB));
			}
			HIP_TRY(c, hipMemcpyAsync(r->first_buf.p, c->first_chunk.p, ev_total * 4, hipMemcpyDeviceToHost, sB));
			HIP_TRY(c, hipStreamSynchronize(sB));
			have_chunks = now_chunks;
			r->arena_items = (size_t)now_chunks * CHUNK_ITEMS;
			rs.rebind((const Item*)r->arena_buf.p, r->arena_items, (const u32*)r->first_buf.p);
			rerun.clear();
			if (!rs.resume(rerun, wide) || ++rounds > 10000000u) {
				return fail(c, NTEDIT_E_DEVICE, "parked events could not be resolved");
			}
		}
		if (getenv("NTEDIT_HIP_DEBUG")) {
			fprintf(stderr, "[ntedit_hip] %u events parked by the budget, %u re-run round(s)\n", n_unfinished, rounds);
		}
	}
	return 0;
}

int
PolishRun::finish()
{
	HIP_TRY(c, hipEventRecord(c->ev[4], sB));
	HIP_TRY(c, hipStreamSynchronize(sB));
	// one entry per event, in position order; NONE32 = the event produced nothing (the renderer skips those)
	r->n_ev_first = ev_total;
	// timings: screening = sum of its launches (they may overlap machine kernels)
	float ms_screen = 0.f;
	const size_t n_scr = pipelined ? n_ch : 1;
	for (size_t j = 0; j < n_scr; j++) {
		const float t = elapsed_ms(c->chunk_ev[2 * j], c->chunk_ev[2 * j + 1]);
		ms_screen += t;
	}
	r->st.ms_screen = ms_screen;
	r->st.screen_launches = h2d_launches ? h2d_launches : (uint32_t)n_scr;
	if (!pipelined && !h2d_launches && c->bin_chunks_last && !candmap_used) {
		r->st.screen_binned = 1;
		r->st.screen_launches = c->bin_chunks_last;
		for (u32 q = 0; q < c->bin_chunks_last; q++) {
			const float tp = elapsed_ms(c->bin_ev[4 * q], c->bin_ev[4 * q + 1]), tq = elapsed_ms(c->bin_ev[4 * q + 2], c->bin_ev[4 * q + 3]);
			r->st.ms_partition += tp;
			r->st.ms_probe += tq;
		}
	}
	r->st.screen_chunks_direct = c->bin_chunks_direct;
	r->st.screen_overflow_records = c->bin_ovf_entries;
	r->st.events_skipped = (uint32_t)skipped_total;
	r->st.ms_machine = ms_machine;
	r->st.ms_extract = 0.f;
	if (use_assess) {
		r->st.ms_extract = elapsed_ms(c->ev_assess[0], c->ev_assess[1]); // (the run map, k_assess)
	}
	HIP_TRY(c, hipEventElapsedTime(&r->st.ms_total, c->ev[0], c->ev[4]));
	c->last_ms = ms_screen;
	return 0;
}

// The apply stage (nte_api_apply.inc), behind everything a plain call does: the streams are idle, the arena and the first-chunk
// table in HBM are what collect() copied (the re-runs of parked events write both on the device), c->bitmap still holds step
// 1's answer (k_assess writes a map of its own, c->runmap).  With no flag, no spectrum and no store on, nothing of it runs.
int
PolishRun::apply()
{
	r->apply_flags = c->apply_flags;
	r->device = c->device;
	if (!c->apply_flags && !c->rep.sp.on && c->cn.state == CN_OFF) {
		return 0;
	}
	const ApplyInput in = { c, r, d_seq, n, n_words, n_contigs, d_bitmap, f0, ev_total, fa_names };
	return apply_stage(in);
}

} // namespace

extern "C" int
ntedit_hip_polish_batch(
    ntedit_hip_ctx* c,
    const char* bases,
    uint64_t n,
    const uint64_t* offsets,
    const uint32_t* lens,
    uint32_t n_contigs,
    int on_device,
    ntedit_hip_result** out)
{
	if (!c || !out || (n && !bases) || (n_contigs && (!offsets || !lens)) || on_device < 0 || on_device > NTEDIT_HIP_BASES_PACKED) {
		return fail(c, NTEDIT_E_ARG, "polish_batch: bad argument");
	}
	*out = nullptr;
	HIP_TRY(c, hipSetDevice(c->device));
	int rc;
	if ((c->rep.sp.on || c->cn.state != CN_OFF) && (rc = spectrum_refuse(c, "polish_batch"))) {
		return rc; // (a plain filter, or none -- NTEDIT_E_ARG, ahead of the general answer below: before anything is polished)
	}
	if ((rc = refresh_params(c))) {
		return rc;
	}
	if ((c->apply_flags & NTEDIT_HIP_APPLY_SHARED) && (rc = shared_refuse(c, "polish_batch"))) {
		return rc; // (a counting filter: before anything is polished)
	}
	if ((c->apply_flags & NTEDIT_HIP_APPLY_BGZF) && (!c->rep.bz.fa_names_set || c->rep.bz.fa_names.size() != n_contigs)) {
		return fail(c, NTEDIT_E_ARG, "polish_batch: APPLY_BGZF needs the header line of every entry (ntedit_hip_set_fa_names): %u entries, %s",
		            n_contigs, c->rep.bz.fa_names_set ? "another number of names" : "no names");
	}
	if (const u32 bad = nte_host::first_layout_break(n, offsets, lens, n_contigs, true); bad != nte_host::LAYOUT_OK) {
		return fail(c, NTEDIT_E_ARG, "polish_batch: contig %u breaks the batch layout", bad);
	}
	std::vector<std::string> fa_names; // (the header lines serve this call alone: used up once its arguments are accepted)
	if (c->apply_flags & NTEDIT_HIP_APPLY_BGZF) {
		fa_names.swap(c->rep.bz.fa_names);
		c->rep.bz.fa_names_set = false;
	}
	ntedit_hip_result* r = new ntedit_hip_result();
	r->owner = c;
	memset(&r->st, 0, sizeof r->st);
	r->st.bases = n;
	r->snv = c->hp.snv ? 1 : 0;
	r->part_margin = c->dp.k + c->dp.max_deletions + 48; // (what an event may touch behind the end of its run)
	r->apply_flags = c->apply_flags;
	r->device = c->device;
	if (n == 0 || n_contigs == 0) {
		if (c->rep.sp.on) { // (nothing to count: zeros)
			r->spectrum = true;
			r->sp_bins.assign(2 * (size_t)SPECTRUM_BINS, 0);
			r->depth.assign(n_contigs, ntedit_hip_depth_row{ 0, 0, 0, 0, 0, 0 });
			c->rep.sp.last = ntedit_hip_spectrum_stats{};
		}
		*out = r;
		return 0;
	}
	PolishRun run;
	run.c = c;
	run.bases = bases;
	run.n = n;
	run.offsets = offsets;
	run.lens = lens;
	run.n_contigs = n_contigs;
	run.on_device = on_device;
	run.r = r;
	run.fa_names = &fa_names;
	if ((rc = run.plan())) {
		return run.bail(rc);
	}
	for (int attempt = 0;; attempt++) {
		if ((rc = run.begin_attempt()) || (rc = run.launch_screening(attempt))) {
			return run.bail(rc);
		}
		for (size_t j = 0; j < run.n_ch && run.status == 0; j++) {
			if ((rc = run.run_chunk_events(j))) {
				return run.bail(rc);
			}
		}
		if (hipStreamSynchronize(run.sA) != hipSuccess || hipStreamSynchronize(run.sB) != hipSuccess) {
			return run.bail(fail(c, NTEDIT_E_DEVICE, "stream synchronisation failed: %s", hipGetErrorString(hipGetLastError())));
		}
		if (run.status == 0) {
			bool redo = false;
			if ((rc = run.collect(&redo))) {
				return run.bail(rc);
			}
			if (!redo) {
				if ((rc = run.finish()) || (rc = run.apply())) {
					return run.bail(rc);
				}
				break;
			}
		}
		if (attempt >= 4) {
			return run.bail(fail(c, NTEDIT_E_OVERFLOW, "event machine ran out of room (status %u)", run.status));
		}
		if (run.status & EV_ARENA_FULL) {
			run.arena_chunks *= 4;
		}
		if (run.status & EV_OVERFLOW) {
			c->dp.node_window *= 2;
		}
	}
	*out = r;
	return 0;
}


// ---- ntedit_hip_reserve -------------------------------------------------------------------------------------
// Everything a context's FIRST batch pays on top of a warm one, paid here instead: the grow-only device buffers sized for
// batches of up to max_batch_bytes (hipMalloc of fresh memory runs at ~40 GB/s: 84 GB of screening records take two
// seconds, the 7 GB of a 250 Mbp batch 160 ms -- inside the call, unless they are here), the page-locked result
// buffers, and one small internal batch through the current filter(s) and parameters that loads the code objects of
// every kernel of the configuration, sets their attributes and makes the runtime allocate their scratch memory on the
// context's streams.  Nothing here can change a result: buffers only grow, the warm-up batch's result is dropped.
extern "C" int
ntedit_hip_reserve(ntedit_hip_ctx* c, uint64_t max_batch_bytes, uint32_t max_contigs, uint64_t events_hint, int on_device)
{
	if (!c || on_device < 0 || on_device > NTEDIT_HIP_BASES_PACKED) {
		return fail(c, NTEDIT_E_ARG, "reserve: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = refresh_params(c);
	if (rc) {
		return rc;
	}
	const u64 n = max_batch_bytes;
	if (n == 0) {
		return 0;
	}
	const Filter f0 = dev_filter(c->filt[0]);
	u32 slog = 0, nsl = 0;
	const bool binned = binned_applicable(c, f0, n, &slog, &nsl);
	// ---- warm-up: 256 KiB of pseudo-random bases (with a real filter nearly every k-mer is absent: events on the
	// start grid, the thread-per-event launch hands them to the wavefront-per-event launch), screened the way the
	// big batches will be, event rounds forced so that their kernels load too.  In contigs of a kilobase: whatever the
	// parameters make of a draft nothing is known about (-m 2 sweeps every candidate at every position, a tiny event
	// budget parks every event, ...), no run is longer than its contig.  A warm-up that runs out of room all the same
	// is not an error: the buffers below are what the call is for.
	{
		const u64 wn = 1u << 18;
		const u32 wc = 256;
		std::vector<char> buf(wn);
		std::vector<uint64_t> offs(wc);
		std::vector<uint32_t> lens(wc);
		u64 x = 0x9E3779B97F4A7C15ULL;
		for (u64 i = 0; i < wn; i++) {
			x = x * 6364136223846793005ULL + 1442695040888963407ULL;
			buf[i] = "ACGT"[(x >> 60) & 3];
		}
		for (u32 i = 0; i < wc; i++) {
			offs[i] = (u64)i * (wn / wc);
			lens[i] = (uint32_t)(wn / wc - 1);
			buf[offs[i] + lens[i]] = '\n';
		}
		ntedit_hip_result* wr = nullptr;
		{
			WarmupSwitches warmup(c, binned); // (the batch is no part of the draft: it leaves nothing in any report)
			rc = ntedit_hip_polish_batch(c, buf.data(), wn, offs.data(), lens.data(), wc, NTEDIT_HIP_BASES_HOST, &wr);
		}
		if (wr) {
			ntedit_hip_result_free(wr);
		}
		if (rc && rc != NTEDIT_E_OVERFLOW) {
			return rc;
		}
		if (rc) {
			c->err.clear(); // (a warm-up that ran out of room is not an error: nothing of it is kept)
		}
	}
	// ---- device buffers
	const u64 n_words = (n + 63) / 64;
	if (on_device != NTEDIT_HIP_BASES_DEVICE) {
		if ((rc = ensure(c, c->seq, n + 64))) {
			return rc;
		}
		if (on_device == NTEDIT_HIP_BASES_PACKED && (rc = ensure(c, c->packed, (size_t)((n + 31) / 32 * 16 + (n + 127) / 128 * 16)))) {
			return rc;
		}
	}
	if ((rc = ensure(c, c->bitmap, (n_words + 8) * 8)) || (rc = ensure(c, c->counters, 256)) ||
	    (rc = ensure(c, c->offs, (size_t)(max_contigs ? max_contigs : 1) * 8)) || (rc = ensure(c, c->lens, (size_t)(max_contigs ? max_contigs : 1) * 4))) {
		return rc;
	}
	if ((c->dp.snv || c->dp.counting) && (rc = ensure(c, c->runmap, (n_words + 8) * 8))) {
		return rc;
	}
	if (binned) {
		u64 chunk_unused = 0;
		if ((rc = binned_buffers(c, f0, n, nsl, probe_parts_log2(c, f0, slog), &chunk_unused))) {
			return rc;
		}
	}
	const u64 n_sblocks = (n_words + ST_TPB - 1) / ST_TPB;
	if ((rc = ensure(c, c->block_counts, n_sblocks * 2 * 4)) || (rc = ensure(c, c->block_offsets, n_sblocks * 8))) {
		return rc;
	}
	// events: what the bench workload's error rates give (one start per ~680 bases) with room to spare, or the caller's figure
	const u64 n_ev = events_hint ? events_hint : n / 400 + 4096;
	if (n_ev > c->events.cap / 8 || n_ev > c->first_chunk.cap / 4) {
		const u64 want = n_ev * 2 + 1024; // (as extract_events grows them)
		if ((rc = ensure(c, c->events, want * 8)) || (rc = ensure(c, c->first_chunk, want * 4))) {
			return rc;
		}
	}
	if ((rc = ensure(c, c->deferred, n_ev * 4))) {
		return rc;
	}
	if (c->tune.settle != 0 && settle_applicable(c->dp, f0) && !c->filt[1].set && (rc = ensure(c, c->ev_rest, n_ev * 4))) { // (k_settle's rest list)
		return rc;
	}
	if (n_ev >= (u64)c->cu_count * 8192) { // (event rounds)
		if ((rc = ensure(c, c->ev_cover, n_ev * 8)) || (rc = ensure(c, c->ev_before, n_ev * 8)) || (rc = ensure(c, c->ev_flags, n_ev)) ||
		    (rc = ensure(c, c->ev_list, n_ev * 4)) || (rc = ensure(c, c->ev_bmax, (size_t)((n_ev + 1023) / 1024) * 8 + 8))) {
			return rc;
		}
	}
	{
		const u64 arena_chunks = n / 160 + 65536;
		if ((rc = ensure(c, c->arena, arena_chunks * CHUNK_ITEMS * sizeof(Item)))) {
			return rc;
		}
		const u64 max_threads = (u64)c->cu_count * 2048;
		u64 threads = n_ev < max_threads ? n_ev : max_threads;
		threads = (threads + MACHINE_TPB - 1) / MACHINE_TPB * MACHINE_TPB;
		const u64 W = c->dp.node_window;
		if ((rc = ensure(c, c->ws_nodes, threads * W * sizeof(Node))) || (rc = ensure(c, c->ws_ov_pos, threads * W * 4)) ||
		    (rc = ensure(c, c->ws_ov_chr, threads * W)) || (rc = ensure(c, c->ws_prev, threads * W)) || (rc = ensure(c, c->ws_lps, threads * W * 2))) {
			return rc;
		}
		const u64 win_bytes = 2 * (u64)c->dp.k + c->dp.max_deletions + 8 + 32;
		if (win_bytes * MACHINE_TPB > 40 * 1024 && (rc = ensure(c, c->ws_win, threads * (win_bytes + 64)))) {
			return rc;
		}
	}
	if (c->apply_flags || c->rep.sp.on || c->cn.state != CN_OFF) {
		// (assumptions about a draft, not sizes: the edited bases and the longer side n + n / 64 + 4096, two pieces per event
		// and entry, about as many intervals as events; the sizes themselves are the reports': their structs in nte_api.hip)
		const u64 n_after = n + n / 64 + 4096, n_entries = max_contigs ? max_contigs : 1;
		Reports& rep = c->rep;
		if ((rc = rep.ap.size_plan(c, n_ev, n_entries)) || (rc = rep.ap.size_write(c, rep.ap.edited, n_after, 2 * n_ev + 2 * (u64)max_contigs + 1024))) {
			return rc;
		}
		if ((c->apply_flags & (NTEDIT_HIP_APPLY_QV | NTEDIT_HIP_APPLY_SHARED | NTEDIT_HIP_APPLY_TRACK)) && (rc = rep.ap.size_assess(c, n_after, n_entries))) {
			return rc;
		}
		if ((c->apply_flags & NTEDIT_HIP_APPLY_TRACK) && (rc = rep.tr.size(c, n_after, n_ev))) {
			return rc;
		}
		if (rep.sp.on && (rc = ensure(c, rep.sp.buf, SpectrumReport::bytes(n_entries)))) {
			return rc;
		}
		if (c->apply_flags & NTEDIT_HIP_APPLY_BGZF) { // (the image: the edited bases, and per entry '>', a header line, '\n')
			std::string why;
			const u64 image = n_after + n_entries * 64;
			if ((rc = bgzf_reserve(c, c->device, c->stream, image, max_contigs, &why))) {
				return fail(c, rc, "reserve: %s", why.c_str());
			}
			// two results hold members at a time: the one a writer is writing out and the one being polished
			PinBuf z[2];
			rc = bgzf_pin_take(c, (size_t)(image / 3), &z[0]);
			rc = rc ? rc : bgzf_pin_take(c, (size_t)(image / 3), &z[1]);
			bgzf_pin_give(c, z[0]); // (an empty one is ignored)
			bgzf_pin_give(c, z[1]);
			if (rc) {
				return rc;
			}
		}
	}
	// ---- page-locked result buffers (an event's records are about one 128-byte chunk; the pool hands out the best fit)
	{
		const size_t want[3] = { (size_t)(n_ev + n_ev / 4 + 4096) * CHUNK_ITEMS * sizeof(Item) + 16, (size_t)(n_ev + n_ev / 4) * 4 + 16,
			                     (size_t)(n_ev + n_ev / 2 + 4096) * CHUNK_ITEMS * sizeof(Item) + 16 };
		PinBuf taken[3];
		for (int i = 0; i < 3 && !rc; i++) {
			rc = pin_take(c, want[i], &taken[i]);
		}
		for (PinBuf& b : taken) {
			pin_give(c, b); // (an empty one is ignored)
		}
		if (rc) {
			return rc;
		}
	}
	HIP_TRY(c, hipDeviceSynchronize());
	return 0;
}
