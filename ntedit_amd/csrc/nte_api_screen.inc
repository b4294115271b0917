// nte_api_screen.inc -- part of nte_api.hip (inside its anonymous namespace): launches of the screening kernels -- direct
// (k_screen) and L2-partitioned (nte_bin_wc.inc + k_bin_probe) --, staging of a batch in HBM (bytes, or the packed form),
// PlainScreen and WarmupSwitches.  (The reports' helpers -- marks, spectrum -- are in nte_api_reports.inc.)
bool binned_applicable(const ntedit_hip_ctx* c, const Filter& f, u64 n, u32* slice_log2, u32* n_slices);
bool candmap_applicable(const ntedit_hip_ctx* c, const Filter& f, u64 n, u32* slice_log2, u32* n_slices);
int bin_reset(ntedit_hip_ctx* c, hipStream_t stream);
int bin_recover(ntedit_hip_ctx* c, hipStream_t stream, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words, u64 p0, u64 p1, u32* recovered);
int run_screen_binned(ntedit_hip_ctx* c, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words, u32 slog, u32 n_slices, hipStream_t stream = nullptr, u64 pos_begin = 0, u64 pos_end = ~0ULL, bool gate = false);

// Launches k_screen over tiles [first_tile, first_tile + n_tiles) of the batch on `stream`.
// lds_pad > 0 lowers the kernel's occupancy (its speed does not depend on it: it is bound by
// the L2-miss path from 2 workgroups per CU upwards) so that k_machine can share the CUs.
template<bool INSERT>
int
launch_screen_tiles(
    ntedit_hip_ctx* c,
    hipStream_t stream,
    const u8* d_seq,
    u64 n,
    const Filter& f,
    u64* d_bitmap,
    u64 n_words,
    u64 first_tile,
    u64 n_tiles,
    size_t lds_pad)
{
	if (n_tiles == 0) {
		return 0;
	}
	if (n_tiles > 0x7FFFFFFFull) {
		return fail(c, NTEDIT_E_ARG, "batch too large");
	}
	dim3 grid((unsigned)n_tiles), block(SCREEN_TPB);
	const bool pow2 = f.mask != 0;
#define NTE_LAUNCH(H)                                                                            \
	do {                                                                                         \
		if (pow2) {                                                                              \
			hipLaunchKernelGGL(                                                                  \
			    (k_screen<H, true, INSERT>), grid, block, lds_pad, stream, d_seq, n, f, c->dp,   \
			    c->d_tab, d_bitmap, n_words, first_tile);                                        \
		} else {                                                                                 \
			hipLaunchKernelGGL(                                                                  \
			    (k_screen<H, false, INSERT>), grid, block, lds_pad, stream, d_seq, n, f, c->dp,  \
			    c->d_tab, d_bitmap, n_words, first_tile);                                        \
		}                                                                                        \
	} while (0)
#define NTE_CASE(H) case H: NTE_LAUNCH(H); break;
	switch (f.hash_num) {
		NTE_CASE(1) NTE_CASE(2) NTE_CASE(3) NTE_CASE(4) NTE_CASE(5)
	default:
		NTE_LAUNCH(0);
		break;
	}
#undef NTE_CASE
#undef NTE_LAUNCH
	HIP_TRY(c, hipGetLastError());
	return 0;
}

template<bool INSERT>
int
launch_screen(ntedit_hip_ctx* c, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words)
{
	const u64 blocks = (n + SCREEN_TILE - 1) / SCREEN_TILE;
	if (blocks == 0) {
		return 0;
	}
	if (!INSERT) {
		u32 slog = 0, n_slices = 0;
		if (binned_applicable(c, f, n, &slog, &n_slices)) {
			return run_screen_binned(c, d_seq, n, f, d_bitmap, n_words, slog, n_slices);
		}
		c->bin_chunks_last = 0;
	}
	return launch_screen_tiles<INSERT>(c, c->stream, d_seq, n, f, d_bitmap, n_words, 0, blocks, 0);
}

// One screening of a whole buffer on the context's stream: the previous call's record chunks are forgotten, the n bytes at
// d_seq are screened into d_bitmap -- between `begin` and `end` where the caller times it --, record chunks that lost probes
// are screened again (bin_recover: the stream is waited for where the binned pipeline ran).  Whether the screening is a plain
// one (PlainScreen) is the caller's business.
int
screen_whole(ntedit_hip_ctx* c, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words, hipEvent_t begin = nullptr, hipEvent_t end = nullptr)
{
	int rc;
	if ((rc = bin_reset(c, c->stream))) {
		return rc;
	}
	if (begin) {
		HIP_TRY(c, hipEventRecord(begin, c->stream));
	}
	if ((rc = launch_screen<false>(c, d_seq, n, f, d_bitmap, n_words))) {
		return rc;
	}
	if (end) {
		HIP_TRY(c, hipEventRecord(end, c->stream));
	}
	u32 recovered = 0;
	return bin_recover(c, c->stream, d_seq, n, f, d_bitmap, n_words, 0, n, &recovered);
}

// -s 0 semantics for the screenings of a scope: with -s 1 k_screen marks every k-mer of accepted bases, which is not the
// filter's answer (the QV counts, the completeness marks)
struct PlainScreen
{
	ntedit_hip_ctx* c;
	int hp_snv;
	u32 dp_snv;
	explicit PlainScreen(ntedit_hip_ctx* c_) : c(c_), hp_snv(c_->hp.snv), dp_snv(c_->dp.snv)
	{
		c->hp.snv = 0;
		c->dp.snv = 0;
	}
	~PlainScreen()
	{
		c->hp.snv = hp_snv;
		c->dp.snv = dp_snv;
	}
};

// The switches of a scope that polishes ntedit_hip_reserve's warm-up batch, put back when it ends.  Tuning: screened the way
// the big batches will be, event rounds forced so that their kernels load too.  Reports: the batch is no part of the draft,
// so it leaves no completeness marks (SHARED becomes QV, which runs the same screenings), no spectrum and nothing in the draft
// store (k_spectrum's code object loads with the library's others), and it has no names (BGZF is off: the writer has a warm-up
// of its own); if that leaves no flag although something was on, APPLY_EDITED runs the applier's kernels.
struct WarmupSwitches
{
	ntedit_hip_ctx* c;
	ntedit_hip_ctx::Tuning tune;
	u32 apply_flags;
	bool spectrum_on;
	int cn_state;
	WarmupSwitches(ntedit_hip_ctx* c_, bool binned) : c(c_), tune(c_->tune), apply_flags(c_->apply_flags), spectrum_on(c_->rep.sp.on), cn_state(c_->cn.state)
	{
		if (binned) {
			c->tune.screen_mode = 2;
		}
		c->tune.force_rounds = 1;
		c->tune.no_rounds = 0;
		u32 flags = apply_flags & ~NTEDIT_HIP_APPLY_BGZF;
		if (flags & NTEDIT_HIP_APPLY_SHARED) {
			flags = (flags & ~NTEDIT_HIP_APPLY_SHARED) | NTEDIT_HIP_APPLY_QV;
		}
		const bool something_on = apply_flags || spectrum_on || cn_state != CN_OFF;
		c->apply_flags = !flags && something_on ? NTEDIT_HIP_APPLY_EDITED : flags;
		c->rep.sp.on = false;
		c->cn.state = CN_OFF;
	}
	~WarmupSwitches()
	{
		c->tune = tune;
		c->apply_flags = apply_flags;
		c->rep.sp.on = spectrum_on;
		c->cn.state = cn_state;
	}
};

// ---- L2-partitioned ("binned") screening; see nte_kernels.hip / nte_bin_wc.inc
// screen_mode 1 forces the direct gather kernel, 2 the binned pipeline (tests run it on small inputs); 0 picks:
// the binned pipeline pays when the filter is far larger than the L2s (the direct kernel then runs at the
// fabric's ~51 G requests/s) and the batch is large enough to fill the persistent partition kernel.
// slices of the partitioned pipeline for filter f and a batch of n positions (bits_per_pos: 1 for the screening, 4 for the
// candidate map of -s 1); false: beyond what the record format / the LDS can do
// slices the partition kernel that will run has rings for: the barrier-phased kernel of the screening takes 2048 in its
// wide layout; the barrier-free kernel ("bin_scatter" 1), the candidate map and a forced 16-slot ring ("bin_ring" 16) 1024
u32
wc_max_slices(const ntedit_hip_ctx* c, bool gate)
{
	return gate || c->tune.bin_scatter == 1 || c->tune.bin_ring == 16 ? (u32)WC_MAX_SLICES : (u32)WCB_WIDE_SLICES;
}

// k_wc_scatter_b's wide layout (8-slot rings, 32-bit state words): beyond 1024 slices, or when asked for ("bin_ring" 8)
bool
wc_wide(const ntedit_hip_ctx* c, u32 n_slices, bool gate)
{
	return !gate && c->tune.bin_scatter != 1 && c->tune.bin_ring != 16 && (n_slices > (u32)WC_MAX_SLICES || c->tune.bin_ring == 8);
}

bool
binned_geometry(const ntedit_hip_ctx* c, const Filter& f, u64 n, u32 bits_per_pos, u32* slice_log2, u32* n_slices)
{
	if (f.hash_num == 0) {
		return false;
	}
	// slices of 2 MiB of filter (2^24 bit slots, 2^21 counters) while the partition kernel has rings for all of them -- up
	// to 4 GiB with the default kernel: half of an XCD's L2 for the slice, the rest for its record stream and the bitmap --;
	// beyond that the slices double until they are few enough, and the probe stage walks those beyond 4 MiB in parts of 4 MiB
	// (probe_parts_log2)
	const bool gate = bits_per_pos != 1;
	u64 max_slices = wc_max_slices(c, gate);
	// (More than 1,024 slices pay when the runs are long.  Measured at a 4 GiB filter, h = 3: 3 Gbp, runs of 17 k records,
	// 127 -> 122 ms per step; 375 Mbp, 2.1 k, no difference; 250 Mbp of counters, 1.4 k, 42.9 -> 43.5: the probe stage walks a
	// run in steps of 512 records and every slice switch has a fixed cost.  Below 4 k records per run: the 1,024 of before.)
	const u64 min_run = c->tune.bin_wide_min_run ? c->tune.bin_wide_min_run : WCB_WIDE_MIN_RUN;
	if (!c->tune.bin_slice_log2 && c->tune.bin_ring != 8 && n * f.hash_num < min_run * WCB_WIDE_SLICES * c->cu_count &&
	    max_slices > (u64)WC_MAX_SLICES) {
		max_slices = WC_MAX_SLICES;
	}
	u32 slog = f.counting ? 21 : 24;
	if (c->tune.bin_slice_log2) { // tests: many slices of a small filter
		slog = c->tune.bin_slice_log2 < 8 ? 8 : (c->tune.bin_slice_log2 < 30 ? c->tune.bin_slice_log2 : 30);
	}
	u64 ns = (f.bits + (1ULL << slog) - 1) >> slog;
	while (ns > max_slices) {
		slog++;
		ns = (f.bits + (1ULL << slog) - 1) >> slog;
	}
	// (the LDS of the kernel that will run: k_wc_scatter's grows with k, k_wc_scatter_b's holds the codes of any k)
	const size_t lds = c->tune.bin_scatter == 1 && !gate ? wc_lds_bytes(c->dp.k) + 1024 : WCB_LDS_BYTES + WCB_LDS_STATIC;
	if (slog > (f.counting ? 27u : 30u) || n * bits_per_pos >= (1ULL << (63 - slog)) || lds > c->lds_per_block) {
		return false; // (beyond 128 GiB of filter: the direct kernel)
	}
	*slice_log2 = slog;
	*n_slices = (u32)ns;
	return true;
}

bool
binned_applicable(const ntedit_hip_ctx* c, const Filter& f, u64 n, u32* slice_log2, u32* n_slices)
{
	u32 mode = c->tune.screen_mode ? c->tune.screen_mode : c->hp.screen_mode;
	// (-s 1 has no screening probes at all: k_screen only marks the k-mers of accepted bases)
	if (mode == 1 || c->tune.bin_fallback || f.hash_num == 0 || f.hash_num > 5 || c->hp.snv) {
		return false;
	}
	if (!binned_geometry(c, f, n, 1, slice_log2, n_slices)) {
		return false;
	}
	if (mode == 2) {
		return true;
	}
	return f.bits >= (f.counting ? 1ULL << 27 : 1ULL << 30) && n >= (1ULL << 26); // auto: filters >= 128 MiB, batches >= 64 Mbases
}

// the candidate map of -s 1 (nte_bin_wc.inc MODE 1): plain filter, the gate's first question first (not -m 2 / -a)
bool
candmap_applicable(const ntedit_hip_ctx* c, const Filter& f, u64 n, u32* slice_log2, u32* n_slices)
{
	if (!c->dp.snv || c->dp.counting || f.counting || c->dp.mode == 2 || c->dp.mask || c->tune.candmap == 0 || c->tune.bin_scatter == 1) {
		return false;
	}
	if (!binned_geometry(c, f, n, 4, slice_log2, n_slices)) {
		return false;
	}
	// Off unless asked for ("candmap" 1).  Measured (250 Mbp, 512 MiB filter, -s 1) once k_assess ran in two phases: the
	// map's partition + probe passes take 9.7 ms (77 G records/s) and save k_assess 7.6 of its 19.0 ms -- the kernel
	// gathers at the random-gather ceiling by then, and the partitioned pipeline is 1.5 x that, not 8 x: 27.9 against
	// 25.9 ms per step.  Kept (and tested) for what it is: the first probe of a dense, dependent probe sequence moved
	// onto the L2-partitioned pipeline, exact, a loss at these rates.
	return c->tune.candmap == 1;
}

// ---- record chunks whose overflow list ran out (k_ovf_check) --------------------------------------------------
// c->bin_state (device): [0..1] overflow entries handed out since the last reset, [BIN_LOST_FLAGS + i] = record chunk i of
// this call lost probes; c->bin_ranges[i] = that chunk's k-mer starts.  A lost chunk's part of the bitmap is void until
// bin_recover() has screened it again with the direct kernel -- the chunk, not the batch, and nothing is remembered: the
// next batch starts on the partitioned pipeline again.
constexpr u32 BIN_MAX_CHUNKS = 16384;

// before the first screening launch of a call (polish_batch attempt, screen): forget the previous call's chunks
int
bin_reset(ntedit_hip_ctx* c, hipStream_t stream)
{
	c->bin_ranges.clear();
	c->bin_chunks_last = 0;
	c->bin_chunks_direct = 0;
	c->bin_ovf_entries = 0;
	if (c->bin_state.p) {
		HIP_TRY(c, hipMemsetAsync(c->bin_state.p, 0, (BIN_LOST_FLAGS + BIN_MAX_CHUNKS) * 4, stream));
	}
	return 0;
}

// After the screening of positions [p0, p1) has been waited for on `stream` (or is ordered before it): reads the
// chunk flags (synchronises `stream`) and screens every lost chunk inside [p0, p1) again with k_screen, on `stream`.
// *recovered = chunks re-screened by this call.
int
bin_recover(ntedit_hip_ctx* c, hipStream_t stream, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words, u64 p0, u64 p1, u32* recovered)
{
	*recovered = 0;
	const size_t nr = c->bin_ranges.size();
	if (!c->bin_state.p || nr == 0) {
		return 0;
	}
	c->bin_flags_host.resize(BIN_LOST_FLAGS + nr);
	HIP_TRY(c, hipMemcpyAsync(c->bin_flags_host.data(), c->bin_state.p, (BIN_LOST_FLAGS + nr) * 4, hipMemcpyDeviceToHost, stream));
	HIP_TRY(c, hipStreamSynchronize(stream));
	c->bin_ovf_entries = (u64)c->bin_flags_host[0] | ((u64)c->bin_flags_host[1] << 32);
	for (size_t i = 0; i < nr; i++) {
		auto& r = c->bin_ranges[i];
		if (!c->bin_flags_host[BIN_LOST_FLAGS + i] || r.recovered || r.begin < p0 || r.begin >= p1) {
			continue;
		}
		if (r.gate) {
			// the candidate map of these positions: "unknown" for every candidate -- k_assess asks the filter itself
			const u64 b0 = r.begin / 2, b1 = (r.end + 1) / 2; // (4 bits per position)
			HIP_TRY(c, hipMemsetAsync((char*)c->candmap.p + b0, 0xFF, b1 - b0, stream));
		} else {
			const u64 t0 = r.begin / SCREEN_TILE, t1 = (r.end + SCREEN_TILE - 1) / SCREEN_TILE;
			int rc = launch_screen_tiles<false>(c, stream, d_seq, n, f, d_bitmap, n_words, t0, t1 - t0, 0);
			if (rc) {
				return rc;
			}
		}
		r.recovered = true;
		c->bin_chunks_direct++;
		(*recovered)++;
		if (getenv("NTEDIT_HIP_DEBUG")) {
			fprintf(stderr, "[ntedit_hip] record chunk %zu (k-mer starts %llu-%llu): its overflow list ran out, %s\n",
			        i, (unsigned long long)r.begin, (unsigned long long)r.end, r.gate ? "candidate map set to unknown" : "screened again with the direct kernel");
		}
	}
	return 0;
}

// parts a slice is probed in (k_bin_probe): slices beyond 4 MiB of filter -- 2^25 bit slots, 2^22 counters -- in parts of 4 MiB
u32
probe_parts_log2(const ntedit_hip_ctx* c, const Filter& f, u32 slog)
{
	const u32 base = f.counting ? 22u : 25u;
	u32 plog = slog > base ? slog - base : 0u;
	if (c->tune.probe_parts_log2 != ~0u) { // tests / tuning
		plog = c->tune.probe_parts_log2;
	}
	return plog < slog - 12 ? plog : slog - 12;
}

// geometry of one record chunk: runs of `cap` records, one per (slice, partition workgroup) pair

struct WcPlan
{
	u32 n_wg;
	u32 cap;
	u64 n_wtiles;
	u64 record_bytes;
	bool short_runs; // the runs cannot hold what the pairs expect (WC_MAX_RUN): the chunk has to be smaller
};

WcPlan
plan_wc(const ntedit_hip_ctx* c, u64 kmers, u32 hash_num, u32 n_slices, bool gate = false)
{
	WcPlan w;
	w.n_wtiles = (kmers + WC_WTILE - 1) / WC_WTILE;
	// the tile a workgroup of the kernel that will run walks at a time, in wavefront tiles: k_wc_scatter_b's WCB_TILE, or one
	// wavefront tile per wavefront of k_wc_scatter (a workgroup below that would idle wavefronts)
	const u64 per_wg_tiles = !gate && c->tune.bin_scatter == 1 ? (u64)WC_WAVES : (u64)WCB_TILE / WC_WTILE;
	u64 n_wg = (w.n_wtiles + per_wg_tiles - 1) / per_wg_tiles;
	if (n_wg > c->cu_count) {
		n_wg = c->cu_count; // persistent workgroups, one per CU (the rings take nearly all of a CU's LDS)
	}
	if (n_wg == 0) {
		n_wg = 1;
	}
	w.n_wg = (u32)n_wg;
	// records a pair can expect: the k-mer starts of its workgroup's wavefront tiles, h probes each, spread evenly
	// over the slices (the hash values of DISTINCT k-mers are uniform); 6 sigma + a group on top, and a sixteenth for
	// what is not distinct but spread out all the same (a satellite family that makes up 3 % of a genome sends its
	// probes to ~500 slices: +3 % for those).  What exceeds the run (few k-mers repeated over and over: simple-sequence
	// arrays) goes to the overflow list.  Only the used part of a run is ever read: the slack costs address space.
	const u64 tiles_per_wg = (w.n_wtiles + (u64)w.n_wg * per_wg_tiles - 1) / ((u64)w.n_wg * per_wg_tiles) * per_wg_tiles;
	const double mean = (double)tiles_per_wg * WC_WTILE * hash_num / (double)n_slices;
	double cap = mean + mean / 16.0 + 6.0 * sqrt(mean) + 64.0;
	if (c->tune.bin_cap_percent) {
		cap = mean * c->tune.bin_cap_percent / 100.0 + 8.0; // tests: force the overflow path
	}
	u64 capi = ((u64)cap + WC_GROUP - 1) / WC_GROUP * WC_GROUP;
	const u64 max_run = gate ? WCB_MAX_RUN : c->tune.bin_scatter == 1 ? WC_MAX_RUN : wc_wide(c, n_slices, false) ? WCB_WIDE_MAX_RUN : WCB_MAX_RUN;
	w.short_runs = !c->tune.bin_cap_percent && capi > max_run;
	if (capi > max_run) {
		capi = max_run; // (what does not fit goes through the overflow list)
	}
	w.cap = (u32)capi;
	w.record_bytes = (u64)n_slices * w.n_wg * w.cap * 8;
	return w;
}

// the candidate map of -s 1 (k_wc_scatter_b<3, POW2, 1>)
template<bool POW2>
int
launch_wc_gate(ntedit_hip_ctx* c, hipStream_t stream, const WcArgs& w)
{
	HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wc_scatter_b<3, POW2, 1>),
	                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)WCB_LDS_BYTES));
	hipLaunchKernelGGL((k_wc_scatter_b<3, POW2, 1>), dim3(w.n_wg), dim3(WCB_TPB), WCB_LDS_BYTES, stream, w);
	return 0;
}

template<int H, bool POW2>
int
launch_wc(ntedit_hip_ctx* c, hipStream_t stream, const WcArgs& w)
{
	// (the rings of the kernel that runs must cover the slices: binned_geometry and this agree on the kernel)
	const bool wide = wc_wide(c, w.b.n_slices, false);
	if (w.b.n_slices > (wide ? (u32)WCB_WIDE_SLICES : (u32)WC_MAX_SLICES)) {
		return fail(c, NTEDIT_E_ARG, "binned screening: %u slices are more than the partition kernel has rings for", w.b.n_slices);
	}
	// (per device: the attribute belongs to the function ON the current device)
	if (c->tune.bin_scatter == 1) {
		const size_t lds = wc_lds_bytes(w.b.p.k);
		HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wc_scatter<H, POW2>),
		                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		hipLaunchKernelGGL((k_wc_scatter<H, POW2>), dim3(w.n_wg), dim3(WC_TPB), lds, stream, w);
	} else if (wide) {
		HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wc_scatter_b<H, POW2, 0, true>),
		                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)WCB_LDS_BYTES));
		hipLaunchKernelGGL((k_wc_scatter_b<H, POW2, 0, true>), dim3(w.n_wg), dim3(WCB_TPB), WCB_LDS_BYTES, stream, w);
	} else {
		HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_wc_scatter_b<H, POW2>),
		                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)WCB_LDS_BYTES));
		hipLaunchKernelGGL((k_wc_scatter_b<H, POW2>), dim3(w.n_wg), dim3(WCB_TPB), WCB_LDS_BYTES, stream, w);
	}
	return 0;
}

int
run_wc_partition(ntedit_hip_ctx* c, hipStream_t stream, const WcArgs& w, bool gate = false)
{
	const bool pow2 = w.b.f.mask != 0;
	if (gate) {
		return pow2 ? launch_wc_gate<true>(c, stream, w) : launch_wc_gate<false>(c, stream, w);
	}
	switch (w.b.f.hash_num) {
	case 1:
		return pow2 ? launch_wc<1, true>(c, stream, w) : launch_wc<1, false>(c, stream, w);
	case 2:
		return pow2 ? launch_wc<2, true>(c, stream, w) : launch_wc<2, false>(c, stream, w);
	case 3:
		return pow2 ? launch_wc<3, true>(c, stream, w) : launch_wc<3, false>(c, stream, w);
	case 4:
		return pow2 ? launch_wc<4, true>(c, stream, w) : launch_wc<4, false>(c, stream, w);
	default:
		return pow2 ? launch_wc<5, true>(c, stream, w) : launch_wc<5, false>(c, stream, w);
	}
}

// The device buffers of the binned screening of `span` k-mer starts: records, run fills, control words, overflow list
// (grow-only; ntedit_hip_reserve sizes them ahead of the first batch).  *chunk_out = k-mer starts per record chunk.
// Record chunks: the whole range at once when its records take no more than 40 % of the HBM that is free right
// now (3 Gbp at h = 3: 74.5 GB), else as few equal chunks as that allows.  (Partitioning chunk j + 1 while chunk j is
// probed, on two streams with two record buffers, was built and measured in round 3: the sum of the stages' own times
// -- both lean on the L2 -- and was taken out again; DESIGN.md 8, experiment 9.)
// Overflow entries per record chunk: an eighth of the chunk's records (3 % of a genome in simple-sequence arrays are 3 %
// of its records, nearly all of which overflow), at least 4 M (a block per partition wavefront is 1 M).
constexpr u32 WC_OVF_MIN = 1u << 22;
u32
ovf_capacity(const ntedit_hip_ctx* c, u64 kmers, u32 hash_num)
{
	u64 cap = kmers * hash_num / 8;
	if (c->tune.bin_ovf_cap) { // tests: a list that runs out
		cap = c->tune.bin_ovf_cap;
	} else if (cap < WC_OVF_MIN) {
		cap = WC_OVF_MIN;
	}
	return (u32)(cap < WC_OVF_MAX_CAP ? cap : WC_OVF_MAX_CAP);
}

int
binned_buffers(ntedit_hip_ctx* c, const Filter& f, u64 span, u32 n_slices, u32 plog, u64* chunk_out, u32 records_per_kmer = 0)
{
	const u32 hn = records_per_kmer ? records_per_kmer : f.hash_num;
	const u64 unit = (u64)WC_WTILE * WC_WAVES;
	u64 parts = 1;
	{
		size_t free_b = 0, total_b = 0;
		u64 room = ~0ULL;
		if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
			room = (u64)(free_b + c->bin_records.cap + c->bin_ovf.cap) / 5 * 2;
		}
		auto bytes_of = [&](u64 kmers, bool* short_runs) {
			const WcPlan pl = plan_wc(c, kmers, hn, n_slices, records_per_kmer != 0);
			*short_runs = pl.short_runs;
			return pl.record_bytes + (u64)ovf_capacity(c, kmers, hn) * sizeof(WcOvf);
		};
		bool short_runs = false;
		for (;;) {
			const u64 need = bytes_of((span + parts - 1) / parts, &short_runs);
			if (parts >= 4096 || (need <= room && !short_runs)) {
				break;
			}
			parts++;
		}
		if (bytes_of((span + parts - 1) / parts, &short_runs) > room) {
			return fail(c, NTEDIT_E_DEVICE, "not enough device memory for the screening records");
		}
	}
	u64 chunk = ((span + parts - 1) / parts + unit - 1) / unit * unit;
	if (c->tune.bin_chunk) { // tests: force several chunks
		const u64 v = c->tune.bin_chunk / unit * unit;
		if (v >= unit && v < chunk) {
			chunk = v;
		}
	}
	const WcPlan plan0 = plan_wc(c, span < chunk ? span : chunk, hn, n_slices, records_per_kmer != 0);
	const size_t ctl_words = CTL_WORK + ((size_t)n_slices << plog) + 1;
	int rc;
	if (!c->bin_state.p) {
		if ((rc = ensure(c, c->bin_state, (BIN_LOST_FLAGS + BIN_MAX_CHUNKS) * 4))) {
			return rc;
		}
		HIP_TRY(c, hipMemset(c->bin_state.p, 0, (BIN_LOST_FLAGS + BIN_MAX_CHUNKS) * 4));
	}
	if ((rc = ensure(c, c->bin_records, plan0.record_bytes)) || (rc = ensure(c, c->bin_fill, (size_t)n_slices * plan0.n_wg * 4)) ||
	    (rc = ensure(c, c->bin_ctl, (ctl_words + 8 + n_slices) * 4)) || // (+ the overflow counter's words, + longest[])
	    (rc = ensure(c, c->bin_ovf, (size_t)ovf_capacity(c, span < chunk ? span : chunk, hn) * sizeof(WcOvf)))) {
		return rc;
	}
	*chunk_out = chunk;
	return 0;
}

int
run_screen_binned(ntedit_hip_ctx* c, const u8* d_seq, u64 n, const Filter& f, u64* d_bitmap, u64 n_words, u32 slog, u32 n_slices, hipStream_t stream, u64 pos_begin, u64 pos_end, bool gate)
{
	// gate: d_bitmap is the candidate map of -s 1 (4 bits per position: first-probe bits of its three substitution
	// candidates), the records are those of k_wc_scatter_b<3, POW2, 1>, the probe stage ORs the bits that are SET
	const u32 hn = gate ? 3u : f.hash_num;
	const u32 bshift = gate ? 2u : 0u; // bits per position, as a shift
	if (!stream) {
		stream = c->stream;
	}
	if (pos_end > n) {
		pos_end = n;
	}
	const u64 span = pos_end - pos_begin;
	const u64 unit = (u64)WC_WTILE * WC_WAVES; // chunk sizes: whole workgroup rounds (also a multiple of 16 bytes)
	const bool arriving = !gate && c->h2d_piece_bytes && span >= 4 * c->h2d_piece_bytes;
	u64 chunk = 0;
	int rc;
	const u32 plog = probe_parts_log2(c, f, slog);
	const size_t n_units = (size_t)n_slices << plog; // (slice, part) pairs of the probe stage
	if ((rc = binned_buffers(c, f, span, n_slices, plog, &chunk, gate ? 3u : 0u))) {
		return rc;
	}
	const size_t ctl_words = CTL_WORK + n_units + 1;
	{
		// the probe stage ORs into the bitmap: clear the words of the range first
		const u64 w0 = (pos_begin << bshift) / 64, w1 = ((pos_end << bshift) + 63) / 64 < n_words ? ((pos_end << bshift) + 63) / 64 : n_words;
		HIP_TRY(c, hipMemsetAsync(d_bitmap + w0, 0, (w1 - w0) * 8, stream));
	}
	// Chunk boundaries.  A batch in HBM: chunks of `chunk` k-mer starts (one, as a rule).  A batch that is still crossing
	// PCIe (round 6): every chunk is WHAT HAS ARRIVED when the chunk before it is through -- the host waits for that chunk's
	// last kernel, asks the copy events how far the batch has come, and launches the next chunk over all of it; it waits
	// for a piece only when nothing new is there.  The chunk sizes follow the ratio of the two rates by themselves (a
	// link faster than the screening: few chunks that grow; a slower one: the screening trails the copy by one piece),
	// where the fixed schedule of rounds 3-5 -- one piece, three, eight, the rest -- waited 17 ms of a 3 Gbp batch for
	// pieces that had not arrived and screened a fifth of it in chunks too small for the probe stage's fixed cost.
	const bool by_arrival = arriving && !c->tune.h2d_fixed_schedule;
	std::vector<u64> cuts;
	if (!by_arrival) {
		u64 at = pos_begin, step = chunk;
		if (arriving) {
			step = c->h2d_piece_bytes / unit * unit;
			step = step < unit ? unit : step;
		}
		while (at < pos_end) {
			u64 len = step < chunk ? step : chunk;
			if (arriving && pos_end - at < len + len / 2) {
				len = pos_end - at < chunk ? pos_end - at : chunk; // (no small rest)
			}
			at = at + len < pos_end ? at + len : pos_end;
			cuts.push_back(at);
			if (arriving) {
				step = step * 3 < chunk ? step * 3 : chunk;
			}
		}
	}
	// pieces of the batch known to be in HBM (leading ones), as a position
	u64 pieces_in = 0;
	auto arrived_upto = [&](bool wait_for_more) -> u64 {
		while (pieces_in < c->h2d_pieces) {
			hipError_t q = hipEventQuery(c->h2d_ev[pieces_in]);
			if (q == hipSuccess) {
				pieces_in++;
				wait_for_more = false; // (one more is enough)
				continue;
			}
			if (q != hipErrorNotReady) {
				(void)hipGetLastError();
				return ~0ULL;
			}
			if (!wait_for_more) {
				break;
			}
			if (hipEventSynchronize(c->h2d_ev[pieces_in]) != hipSuccess) {
				return ~0ULL;
			}
		}
		return pieces_in >= c->h2d_pieces ? n : pieces_in * c->h2d_piece_bytes;
	};
	const size_t ev_base = 4 * (size_t)c->bin_chunks_last; // (a call that screens in several ranges -- pipeline chunks -- keeps counting)
	u32 chunk_no = 0;
	for (u64 begin = pos_begin; begin < pos_end; chunk_no++) {
		u64 end;
		if (by_arrival) {
			// the chunk's bases and the k - 1 behind its end (a tile of slack) must be in HBM
			u64 have = arrived_upto(false);
			for (;;) {
				if (have == ~0ULL) {
					return fail(c, NTEDIT_E_DEVICE, "host-to-device copy failed");
				}
				end = have >= n ? pos_end : (have > SCREEN_TILE ? (have - SCREEN_TILE) / unit * unit : 0);
				end = end > pos_end ? pos_end : end;
				// (not less than a piece at a time, unless it is the rest)
				if (end > begin && (end == pos_end || end - begin >= c->h2d_piece_bytes / 2)) {
					break;
				}
				have = arrived_upto(true);
			}
			if (end - begin > chunk) {
				end = begin + chunk;
			}
		} else {
			end = cuts[chunk_no];
		}
		if (c->bin_ranges.size() + 1 > BIN_MAX_CHUNKS) {
			return fail(c, NTEDIT_E_ARG, "binned screening: more than %u record chunks in one call", BIN_MAX_CHUNKS);
		}
		while (c->bin_ev.size() < ev_base + 4 * (size_t)(chunk_no + 1)) {
			hipEvent_t e;
			HIP_TRY(c, hipEventCreate(&e));
			c->bin_ev.push_back(e);
		}
		const WcPlan plan = plan_wc(c, end - begin, hn, n_slices, gate);
		// (the buffer was sized for the largest chunk; a chunk gets what its own size asks for)
		u32 ovf_cap = ovf_capacity(c, end - begin, hn);
		if ((u64)ovf_cap * sizeof(WcOvf) > c->bin_ovf.cap) {
			ovf_cap = (u32)(c->bin_ovf.cap / sizeof(WcOvf));
		}
		u32* d_ctl = (u32*)c->bin_ctl.p;
		u32* d_ovf_count = d_ctl + ctl_words;
		u32* d_longest = d_ctl + ctl_words + 8; // [n_slices]: zeroed with ctl[], the partition kernel's drain fills it
		WcArgs w;
		w.b.seq = d_seq;
		w.b.n = n;
		w.b.chunk_begin = begin;
		w.b.chunk_end = end;
		w.b.f = f;
		w.b.p = c->dp;
		w.b.tabs = c->d_tab;
		w.b.n_slices = n_slices;
		w.b.slice_log2 = slog;
		w.b.records = (u64*)c->bin_records.p;
		w.fill = (u32*)c->bin_fill.p;
		w.longest = d_longest;
		w.ovf = (WcOvf*)c->bin_ovf.p;
		w.ovf_count = d_ovf_count;
		w.ovf_cap = ovf_cap;
		w.n_wg = plan.n_wg;
		w.cap = plan.cap;
		w.n_wtiles = plan.n_wtiles;
		w.wcodes = (u32)wc_codes_bytes(c->dp.k);
		w.cand32 = gate ? (u32*)d_bitmap : nullptr;
		hipEvent_t* tev = &c->bin_ev[ev_base + 4 * (size_t)chunk_no];
		if (c->h2d_piece_bytes) {
			// the chunk's bases (+ the k-1 behind its end) must have arrived
			u64 piece = (end + SCREEN_TILE) / c->h2d_piece_bytes;
			if (piece >= c->h2d_pieces) {
				piece = c->h2d_pieces - 1;
			}
			HIP_TRY(c, hipStreamWaitEvent(stream, c->h2d_ev[piece], 0));
		}
		HIP_TRY(c, hipMemsetAsync(d_ctl, 0, (ctl_words + 8 + n_slices) * 4, stream));
		HIP_TRY(c, hipEventRecord(tev[0], stream));
		if ((rc = run_wc_partition(c, stream, w, gate))) {
			return rc;
		}
		HIP_TRY(c, hipEventRecord(tev[1], stream));
		HIP_TRY(c, hipEventRecord(tev[2], stream));
		ProbeArgs pa;
		pa.filter = f.data;
		pa.records = (const u64*)c->bin_records.p;
		pa.fill = (const u32*)c->bin_fill.p;
		pa.longest = d_longest;
		pa.n_slices = n_slices;
		pa.slog = slog;
		pa.n_wg = plan.n_wg;
		pa.cap = plan.cap;
		pa.ctl = d_ctl;
		pa.absent32 = (u32*)d_bitmap;
		pa.force_xcc = c->tune.force_xcc ? c->tune.force_xcc - 1 : PROBE_XCC_ANY;
		pa.counting = f.counting;
		pa.count_lo = c->dp.min_thr > 1 ? c->dp.min_thr : 1;
		pa.plog = plog;
		pa.mark_present = gate ? 1u : 0u;
		hipLaunchKernelGGL(k_bin_probe, dim3(c->cu_count * (2048 / PROBE_TPB)), dim3(PROBE_TPB), 0, stream, pa);
		hipLaunchKernelGGL(k_ovf_probe, dim3(c->cu_count * 8), dim3(256), 0, stream, f.data, (const WcOvf*)c->bin_ovf.p, (const u32*)d_ovf_count, ovf_cap, slog,
		                   (u32*)d_bitmap, (u32)f.counting, pa.count_lo, pa.mark_present);
		// overflow entries that did not fit are lost probes: the chunk's flag is looked at (bin_recover) before anything
		// reads its part of the bitmap
		{
			ntedit_hip_ctx::BinRange br;
			br.begin = begin;
			br.end = end;
			br.recovered = false;
			br.gate = gate;
			hipLaunchKernelGGL(k_ovf_check, dim3(1), dim3(1), 0, stream, (const u32*)d_ovf_count, ovf_cap, (u32*)c->bin_state.p, (u32)c->bin_ranges.size());
			c->bin_ranges.push_back(br);
		}
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipEventRecord(tev[3], stream));
		if (by_arrival && end < pos_end) {
			HIP_TRY(c, hipEventSynchronize(tev[3])); // (the next chunk is what has arrived by now)
		}
		if (c->tune.bin_timing) {
			HIP_TRY(c, hipStreamSynchronize(stream));
			const float t_part = elapsed_ms(tev[0], tev[1]), t_probe = elapsed_ms(tev[2], tev[3]);
			u32 ovf_n = 0;
			(void)hipMemcpy(&ovf_n, d_ovf_count, 4, hipMemcpyDeviceToHost);
			fprintf(stderr, "[ntedit_hip] binned chunk %llu k-mers, %u slices of 2^%u bits (rings of %u) probed in %u part(s), %u x %u-record runs per slice (%.2f GB), %u overflow records: partition %.3f ms, probe %.3f ms (stages timed alone)\n",
			        (unsigned long long)(end - begin), n_slices, slog, c->tune.bin_scatter == 1 || !wc_wide(c, n_slices, gate) ? (u32)WC_CAP : (u32)WCB_WIDE_CAP, 1u << plog, plan.n_wg, plan.cap, plan.record_bytes / 1e9, ovf_n, t_part, t_probe);
		}
		begin = end;
	}
	c->bin_chunks_last += chunk_no;
	return 0;
}

// bytes [o, o + len) of a batch that arrives in the packed form (o a multiple of 128, or the whole batch): its codes and
// case bits cross PCIe, k_unpack turns them into bytes of c->seq -- all on `stream`
int
copy_packed_piece(ntedit_hip_ctx* c, const char* packed, u64 n, u64 o, u64 len, hipStream_t stream)
{
	const u64 codes_bytes = (n + 31) / 32 * 16;
	const u64 end = o + len;
	const u64 c0 = o / 2, c1 = end == n ? codes_bytes : end / 2;
	const u64 s0 = o / 8, s1 = end == n ? (n + 127) / 128 * 16 : end / 8;
	HIP_TRY(c, hipMemcpyAsync((char*)c->packed.p + c0, packed + c0, c1 - c0, hipMemcpyHostToDevice, stream));
	HIP_TRY(c, hipMemcpyAsync((char*)c->packed.p + codes_bytes + s0, packed + codes_bytes + s0, s1 - s0, hipMemcpyHostToDevice, stream));
	const u64 g0 = o / 16, g1 = (end + 15) / 16; // (c->seq has 64 bytes of slack behind the batch)
	const u64 blocks = (g1 - g0 + 255) / 256;
	hipLaunchKernelGGL(k_unpack, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, (const u8*)c->packed.p,
	                   (const u8*)c->packed.p + codes_bytes, (u8*)c->seq.p, g0, g1 - g0);
	HIP_TRY(c, hipGetLastError());
	return 0;
}

// copies (or adopts) the batch into HBM; returns the device pointer
int
stage_bases(ntedit_hip_ctx* c, const char* bases, u64 n, int on_device, const u8** out, bool copy = true)
{
	if (on_device == NTEDIT_HIP_BASES_DEVICE) {
		if ((uintptr_t)bases & 15) {
			return fail(c, NTEDIT_E_ARG, "device `bases` must be 16-byte aligned");
		}
		*out = (const u8*)bases;
		return 0;
	}
	int rc = ensure(c, c->seq, n + 64);
	if (rc) {
		return rc;
	}
	if (on_device == NTEDIT_HIP_BASES_PACKED) {
		// the packed form: codes + case bits to HBM, k_unpack writes the byte batch (in pieces: copy_packed_piece)
		if ((rc = ensure(c, c->packed, (size_t)((n + 31) / 32 * 16 + (n + 127) / 128 * 16)))) {
			return rc;
		}
		if (copy && (rc = copy_packed_piece(c, bases, n, 0, n, c->stream))) {
			return rc;
		}
	} else if (copy) {
		HIP_TRY(c, hipMemcpyAsync(c->seq.p, bases, n, hipMemcpyHostToDevice, c->stream));
	}
	*out = (const u8*)c->seq.p;
	return 0;
}

