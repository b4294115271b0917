// nte_api_reports.inc -- part of nte_api.hip: the reports behind the device applier (their state structs: nte_api.hip; the stage
// that runs them: nte_api_apply.inc).  First what they share, in the anonymous namespace; then, at file scope, report by report
// the helpers (static) and the C entry points (with the linkage include/ntedit_hip.h declares).
namespace {

// A batch as a stand-alone call (or the polish) gets it: n bytes of bases in host or device memory, the entries in host
// memory.  The calls share these pieces, not a sequence: each keeps its own order of refusals.
struct BatchArg
{
	const void* bases;
	u64 n;
	int on_device;
	const uint64_t* offs;
	const uint32_t* lens;
	u32 n_entries;
	// "<who>: bad argument" (also where the caller's own arguments are not `ok`), "<who>: bases must be host or device bytes"
	int check(ntedit_hip_ctx* c, const char* who, bool ok) const
	{
		if (!c || !ok || (n && !bases) || (n_entries && (!offs || !lens))) {
			return fail(c, NTEDIT_E_ARG, "%s: bad argument", who);
		}
		if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
			return fail(c, NTEDIT_E_ARG, "%s: bases must be host or device bytes", who);
		}
		return 0;
	}
	// entries that may abut (host/batch_layout.h)
	int layout(ntedit_hip_ctx* c, const char* who) const
	{
		const u32 bad = nte_host::first_layout_break(n, offs, lens, n_entries, false);
		return bad == nte_host::LAYOUT_OK ? 0 : fail(c, NTEDIT_E_ARG, "%s: entry %u breaks the batch layout", who, bad);
	}
};

// the entries of a batch into c->offs and c->lens, queued on `stream`
int
upload_entries(ntedit_hip_ctx* c, hipStream_t stream, const uint64_t* offs, const uint32_t* lens, u32 n_entries)
{
	int rc;
	if ((rc = ensure(c, c->offs, (size_t)n_entries * 8)) || (rc = ensure(c, c->lens, (size_t)n_entries * 4))) {
		return rc;
	}
	HIP_TRY(c, hipMemcpyAsync(c->offs.p, offs, (size_t)n_entries * 8, hipMemcpyHostToDevice, stream));
	HIP_TRY(c, hipMemcpyAsync(c->lens.p, lens, (size_t)n_entries * 4, hipMemcpyHostToDevice, stream));
	return 0;
}

thread_local std::string g_result_err; // ntedit_hip_result_last_error()

int
result_refuse(const ntedit_hip_result* r, int code, const char* fmt, ...)
{
	char buf[256];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_result_err = buf;
	if (code == NTEDIT_E_ARG && r && r->owner && ctx_alive(r->owner)) {
		r->owner->err = buf;
	}
	return code;
}

// The refusals the result accessors share, in their order: the arguments, then the switch the batch was polished with
// (`flag`: one of NTEDIT_HIP_APPLY_*, or 0 for the spectrum's switch).  0: the result has what is asked for.
int
result_check(const ntedit_hip_result* r, const char* who, bool args_ok, u32 flag)
{
	if (!r || !args_ok) {
		return result_refuse(r, NTEDIT_E_ARG, "%s: bad argument", who);
	}
	if (!flag) {
		return r->spectrum ? 0 : result_refuse(r, NTEDIT_E_ARG, "%s: the batch was polished with the spectrum switched off (ntedit_hip_set_spectrum)", who);
	}
	const char* name = flag == NTEDIT_HIP_APPLY_EDITED ? "EDITED" : flag == NTEDIT_HIP_APPLY_QV ? "QV" : flag == NTEDIT_HIP_APPLY_TRACK ? "TRACK" : "BGZF";
	return (r->apply_flags & flag) ? 0 : result_refuse(r, NTEDIT_E_ARG, "%s: the batch was polished without the APPLY_%s flag (ntedit_hip_set_apply)", who, name);
}

int
result_entries(const ntedit_hip_result* r, const char* who, size_t given, size_t held)
{
	return given == held ? 0 : result_refuse(r, NTEDIT_E_ARG, "%s: the batch had another number of entries", who);
}

} // namespace

// ------------------------------------------------------------------------------------------------ the applier, the QV rows
int
ntedit_hip_set_apply(ntedit_hip_ctx* c, uint32_t flags)
{
	if (!c || (flags & ~(NTEDIT_HIP_APPLY_EDITED | NTEDIT_HIP_APPLY_QV | NTEDIT_HIP_APPLY_SHARED | NTEDIT_HIP_APPLY_BGZF | NTEDIT_HIP_APPLY_TRACK))) {
		return fail(c, NTEDIT_E_ARG, "set_apply: unknown flag");
	}
	c->apply_flags = flags;
	return 0;
}

int
ntedit_hip_result_edited_device(const ntedit_hip_result* r, const char** dev_ptr, uint64_t* n_bytes, uint64_t* offsets_out, uint32_t* lens_out,
                                uint32_t n_contigs)
{
	int rc = result_check(r, "result_edited", dev_ptr && n_bytes, NTEDIT_HIP_APPLY_EDITED);
	if (rc || ((offsets_out || lens_out) && (rc = result_entries(r, "result_edited", n_contigs, r->e_offs.size())))) {
		return rc;
	}
	*dev_ptr = (const char*)r->edited.p;
	*n_bytes = r->edited_bytes;
	if (offsets_out && n_contigs) {
		memcpy(offsets_out, r->e_offs.data(), (size_t)n_contigs * 8);
	}
	if (lens_out && n_contigs) {
		memcpy(lens_out, r->e_lens.data(), (size_t)n_contigs * 4);
	}
	return 0;
}

int
ntedit_hip_result_edited(const ntedit_hip_result* r, char* host_buf, uint64_t cap, uint64_t* n_bytes, uint64_t* offsets_out, uint32_t* lens_out,
                         uint32_t n_contigs)
{
	const char* d = nullptr;
	uint64_t nb = 0;
	const int rc = ntedit_hip_result_edited_device(r, &d, &nb, offsets_out, lens_out, n_contigs);
	if (rc) {
		return rc;
	}
	if (n_bytes) {
		*n_bytes = nb;
	}
	if (nb > cap || (nb && !host_buf)) {
		return result_refuse(nullptr, NTEDIT_E_OVERFLOW, "result_edited: the buffer is too small");
	}
	if (nb && (hipSetDevice(r->device) != hipSuccess || hipMemcpy(host_buf, d, nb, hipMemcpyDeviceToHost) != hipSuccess)) {
		return result_refuse(nullptr, NTEDIT_E_DEVICE, "result_edited: the download failed");
	}
	return 0;
}

int
ntedit_hip_result_qv(const ntedit_hip_result* r, ntedit_hip_qv_row* rows, uint32_t n_contigs)
{
	int rc = result_check(r, "result_qv", !n_contigs || rows, NTEDIT_HIP_APPLY_QV);
	if (rc || (rc = result_entries(r, "result_qv", n_contigs, r->qv.size()))) {
		return rc;
	}
	if (n_contigs) {
		memcpy(rows, r->qv.data(), (size_t)n_contigs * sizeof(ntedit_hip_qv_row));
	}
	return 0;
}

int
ntedit_hip_apply_info(ntedit_hip_ctx* c, ntedit_hip_apply_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "apply_info: bad argument");
	}
	*st = c->rep.ap.last;
	return 0;
}

uint32_t
ntedit_hip_apply_tile(void)
{
	return APPLY_TILE;
}

// ------------------------------------------------------------------------------------------------ the intervals (nte_track.hip)
static_assert(sizeof(ntedit_hip_track_interval) == sizeof(TrackInterval) && sizeof(TrackInterval) == 16, "the records are copied as they stand");

// The interval extractor (nte_track.hip) over a bitmap and the entries of its batch, all in device memory, on stream s:
// count and scan, three words to the host, the record buffer sized from them, emit and finish, the records to host memory
// (malloc, *out; null for none; the caller's to free whatever is returned).  The stream is idle when it returns 0.  Crosses
// PCIe: four words and the records.
static int
track_run(ntedit_hip_ctx* c, hipStream_t s, const u64* d_bitmap, u64 n, const u64* d_offs, const u32* d_lens, u32 n_entries, u32 k, int which,
          ntedit_hip_track_interval** out, u64* n_out)
{
	int rc;
	TrackReport& tr = c->rep.tr;
	free(*out);
	*out = nullptr;
	*n_out = 0;
	tr.last.ms[which] = 0.f;
	tr.last.intervals[which] = tr.last.bases[which] = 0;
	const u64 n_tiles = track_tiles(n);
	if (n_tiles == 0 || n_entries == 0) {
		return 0;
	}
	if (n_tiles > 0x7FFFFFFFull) {
		return fail(c, NTEDIT_E_ARG, "track: batch too large");
	}
	if ((rc = ensure_events(c, tr.window)) || (rc = tr.size(c, n, 0))) {
		return rc;
	}
	const TrackArgs a = { d_bitmap, n, d_offs, d_lens, n_entries, k };
	TrackTile* tiles = (TrackTile*)tr.tiles.p;
	u64* totals = (u64*)tr.totals.p;
	u64 h_tot[4] = { 0, 0, 0, 0 };
	HIP_TRY(c, hipEventRecord(tr.window[0].begin, s));
	launch_track_count(s, a, tiles, totals);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(tr.window[0].end, s));
	HIP_TRY(c, hipMemcpyAsync(h_tot, totals, 32, hipMemcpyDeviceToHost, s));
	HIP_TRY(c, hipStreamSynchronize(s));
	if (h_tot[0] != h_tot[1] || h_tot[0] > h_tot[2]) {
		return fail(c, NTEDIT_E_INTERNAL, "track: %llu interval starts, %llu ends, %llu marked starts", (unsigned long long)h_tot[0],
		            (unsigned long long)h_tot[1], (unsigned long long)h_tot[2]);
	}
	float ms = elapsed_ms(tr.window[0]);
	const u64 n_recs = h_tot[0];
	if (n_recs) {
		if ((rc = tr.size(c, n, n_recs))) {
			return rc;
		}
		*out = (ntedit_hip_track_interval*)malloc((size_t)n_recs * sizeof(ntedit_hip_track_interval));
		if (!*out) {
			return fail(c, NTEDIT_E_OVERFLOW, "track: no host memory for %llu intervals", (unsigned long long)n_recs);
		}
		HIP_TRY(c, hipEventRecord(tr.window[1].begin, s));
		launch_track_emit(s, a, tiles, (TrackInterval*)tr.recs.p, (u32*)tr.upto.p, n_recs, totals);
		HIP_TRY(c, hipGetLastError());
		HIP_TRY(c, hipEventRecord(tr.window[1].end, s));
		HIP_TRY(c, hipMemcpyAsync(*out, tr.recs.p, (size_t)n_recs * sizeof(TrackInterval), hipMemcpyDeviceToHost, s));
		HIP_TRY(c, hipMemcpyAsync(h_tot, totals, 32, hipMemcpyDeviceToHost, s));
		HIP_TRY(c, hipStreamSynchronize(s));
		ms += elapsed_ms(tr.window[1]);
		*n_out = n_recs;
	}
	tr.last.ms[which] = ms;
	tr.last.intervals[which] = n_recs;
	tr.last.bases[which] = h_tot[3];
	return 0;
}

int
ntedit_hip_result_track(const ntedit_hip_result* r, int which, ntedit_hip_track_interval* out, uint64_t cap, uint64_t* n)
{
	const int rc = result_check(r, "result_track", n && which >= 0 && which <= 1 && (!cap || out), NTEDIT_HIP_APPLY_TRACK);
	if (rc) {
		return rc;
	}
	*n = r->track_n[which];
	if (*n > cap) {
		return result_refuse(nullptr, NTEDIT_E_OVERFLOW, "result_track: the buffer is too small");
	}
	if (*n) {
		memcpy(out, r->track[which], (size_t)*n * sizeof(ntedit_hip_track_interval));
	}
	return 0;
}

int
ntedit_hip_track_extract(ntedit_hip_ctx* c, const uint64_t* bitmap, uint64_t n_positions, const uint64_t* offs, const uint32_t* lens,
                         uint32_t n_entries, uint32_t k, ntedit_hip_track_interval* out, uint64_t cap, uint64_t* n)
{
	const BatchArg b = { bitmap, n_positions, NTEDIT_HIP_BASES_HOST, offs, lens, n_entries }; // (the bitmap takes the bases' place)
	int rc = b.check(c, "track_extract", n && (!cap || out));
	if (rc) {
		return rc;
	}
	*n = 0;
	if (k == 0 || k > TRACK_MAX_K) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "track_extract: k from 1 to %u", TRACK_MAX_K);
	}
	if ((rc = b.layout(c, "track_extract"))) {
		return rc;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	c->rep.tr.last = ntedit_hip_track_stats{ { 0.f, 0.f }, { 0, 0 }, { 0, 0 } };
	if (b.n == 0 || n_entries == 0) {
		return 0;
	}
	DevBuf& d_bitmap = c->rep.ap.bitmap;
	if ((rc = c->rep.ap.size_assess(c, n_positions, 0))) {
		return rc;
	}
	hipStream_t s = c->stream;
	HIP_TRY(c, hipMemcpyAsync(d_bitmap.p, bitmap, (size_t)((n_positions + 63) / 64) * 8, hipMemcpyHostToDevice, s));
	if ((rc = upload_entries(c, s, offs, lens, n_entries))) {
		return rc;
	}
	ntedit_hip_track_interval* recs = nullptr;
	u64 n_recs = 0;
	rc = track_run(c, s, (const u64*)d_bitmap.p, n_positions, (const u64*)c->offs.p, (const u32*)c->lens.p, n_entries, k, 0, &recs, &n_recs);
	if (rc) {
		(void)hipStreamSynchronize(s);
		free(recs);
		return rc;
	}
	*n = n_recs;
	if (n_recs > cap) {
		free(recs);
		return fail(c, NTEDIT_E_OVERFLOW, "track_extract: %llu intervals, the buffer has room for %llu", (unsigned long long)n_recs, (unsigned long long)cap);
	}
	if (n_recs) {
		memcpy(out, recs, (size_t)n_recs * sizeof(ntedit_hip_track_interval));
	}
	free(recs);
	return 0;
}

int
ntedit_hip_track_info(ntedit_hip_ctx* c, ntedit_hip_track_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "track_info: bad argument");
	}
	*st = c->rep.tr.last;
	return 0;
}

// ------------------------------------------------------------------------------------------------ the k-mer spectrum
// why the context cannot count a spectrum (0: it can)
static int
spectrum_refuse(ntedit_hip_ctx* c, const char* who)
{
	const DevFilter& f = c->filt[0];
	if (!f.set) {
		return fail(c, NTEDIT_E_ARG, "%s: no primary filter to take the k-mer spectrum from", who);
	}
	if (!f.counting) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "%s: the k-mer spectrum takes a counting primary filter; a plain filter's slots are bits", who);
	}
	if (f.k > (u32)SCREEN_MAXK || f.hash_num < 1 || f.hash_num > MAX_HASHES) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "%s: the k-mer spectrum takes k up to %d and 1 to %u hashes", who, SCREEN_MAXK, MAX_HASHES);
	}
	return 0;
}

// sp.buf for a call over n_entries entries, zeroed on `stream`; the events
static int
spectrum_begin(ntedit_hip_ctx* c, hipStream_t stream, u32 n_entries)
{
	SpectrumReport& sp = c->rep.sp;
	int rc;
	if ((rc = ensure_events(c, sp.window)) || (rc = ensure(c, sp.buf, SpectrumReport::bytes(n_entries)))) {
		return rc;
	}
	HIP_TRY(c, hipMemsetAsync(sp.buf.p, 0, SpectrumReport::bytes(n_entries), stream));
	c->rep.sp.last = ntedit_hip_spectrum_stats{};
	return 0;
}

// k_spectrum over a batch in device memory and its entries into launch `which`'s bins and rows and window, on `stream`
static int
launch_spectrum(ntedit_hip_ctx* c, hipStream_t stream, const u8* d_seq, u64 n, const Filter& f, const u64* d_offs, const u32* d_lens, u32 n_entries,
                int which, bool want_rows)
{
	const u64 blocks = (n + SCREEN_TILE - 1) / SCREEN_TILE;
	if (blocks > 0x7FFFFFFFull) {
		return fail(c, NTEDIT_E_ARG, "batch too large");
	}
	if (!f.counting || c->dp.k > (u32)SCREEN_MAXK || c->dp.k == 0) {
		return fail(c, NTEDIT_E_INTERNAL, "spectrum: not a counting filter, or k beyond the tile's halo");
	}
	unsigned long long* bins = c->rep.sp.bins(which);
	unsigned long long* rows = want_rows ? c->rep.sp.rows(which, n_entries) : nullptr;
	const EventPair& window = c->rep.sp.window[which];
	HIP_TRY(c, hipEventRecord(window.begin, stream));
	if (blocks && n_entries) {
		dim3 grid((unsigned)blocks), block(SCREEN_TPB);
		const bool pow2 = f.mask != 0;
#define NTE_LAUNCH(H)                                                                                                              \
	do {                                                                                                                           \
		if (pow2) {                                                                                                                \
			hipLaunchKernelGGL((k_spectrum<H, true>), grid, block, 0, stream, d_seq, n, f, c->dp, c->d_tab, d_offs, d_lens, n_entries, bins, rows);  \
		} else {                                                                                                                   \
			hipLaunchKernelGGL((k_spectrum<H, false>), grid, block, 0, stream, d_seq, n, f, c->dp, c->d_tab, d_offs, d_lens, n_entries, bins, rows); \
		}                                                                                                                          \
	} while (0)
#define NTE_CASE(H) case H: NTE_LAUNCH(H); break;
		switch (f.hash_num) {
			NTE_CASE(1) NTE_CASE(2) NTE_CASE(3) NTE_CASE(4) NTE_CASE(5) NTE_CASE(6) NTE_CASE(7) NTE_CASE(8)
		default:
			return fail(c, NTEDIT_E_UNSUPPORTED, "spectrum: 1 to %u hashes", MAX_HASHES);
		}
#undef NTE_CASE
#undef NTE_LAUNCH
		HIP_TRY(c, hipGetLastError());
	}
	HIP_TRY(c, hipEventRecord(window.end, stream));
	return 0;
}

// after `stream` has been waited for: the launch's time and, from its bins on the host, its k-mers
static void
spectrum_timed(ntedit_hip_ctx* c, int which, const uint64_t* bins)
{
	u64 total = 0;
	for (int i = 0; i < SPECTRUM_BINS; i++) {
		total += bins[i];
	}
	c->rep.sp.last.ms[which] = elapsed_ms(c->rep.sp.window[which]);
	c->rep.sp.last.kmers[which] = total;
}

int
ntedit_hip_set_spectrum(ntedit_hip_ctx* c, int on)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	c->rep.sp.on = on != 0;
	return 0;
}

int
ntedit_hip_result_spectrum(const ntedit_hip_result* r, int which, uint64_t bins[256])
{
	const int rc = result_check(r, "result_spectrum", bins && which >= 0 && which <= 1, 0);
	if (rc) {
		return rc;
	}
	memcpy(bins, r->sp_bins.data() + (size_t)which * SPECTRUM_BINS, SPECTRUM_BINS * 8);
	return 0;
}

int
ntedit_hip_result_depth(const ntedit_hip_result* r, ntedit_hip_depth_row* rows, uint32_t n_contigs)
{
	int rc = result_check(r, "result_depth", !n_contigs || rows, 0);
	if (rc || (rc = result_entries(r, "result_depth", n_contigs, r->depth.size()))) {
		return rc;
	}
	if (n_contigs) {
		memcpy(rows, r->depth.data(), (size_t)n_contigs * sizeof(ntedit_hip_depth_row));
	}
	return 0;
}

int
ntedit_hip_spectrum_count(ntedit_hip_ctx* c, const char* bases, uint64_t n, int on_device, const uint64_t* offs, const uint32_t* lens,
                          uint32_t n_entries, uint64_t* bins, uint64_t* rows)
{
	const BatchArg b = { bases, n, on_device, offs, lens, n_entries };
	int rc = b.check(c, "spectrum_count", bins != nullptr);
	if (rc) {
		return rc;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	// (the filter is refused before the layout is looked at)
	if ((rc = spectrum_refuse(c, "spectrum_count")) || (rc = refresh_params(c)) || (rc = b.layout(c, "spectrum_count"))) {
		return rc;
	}
	memset(bins, 0, SPECTRUM_BINS * 8);
	if (rows && n_entries) {
		memset(rows, 0, (size_t)n_entries * 24);
	}
	c->rep.sp.last = ntedit_hip_spectrum_stats{};
	if (b.n == 0 || n_entries == 0) {
		return 0;
	}
	hipStream_t s = c->stream;
	const u8* d_seq = nullptr;
	if ((rc = stage_bases(c, bases, n, on_device, &d_seq)) || (rc = spectrum_begin(c, s, n_entries)) || (rc = upload_entries(c, s, offs, lens, n_entries))) {
		return rc;
	}
	const Filter f0 = dev_filter(c->filt[0]);
	if ((rc = launch_spectrum(c, s, d_seq, n, f0, (const u64*)c->offs.p, (const u32*)c->lens.p, n_entries, 0, rows != nullptr))) {
		(void)hipStreamSynchronize(s);
		return rc;
	}
	HIP_TRY(c, hipMemcpyAsync(bins, c->rep.sp.bins(0), SPECTRUM_BINS * 8, hipMemcpyDeviceToHost, s));
	if (rows) {
		HIP_TRY(c, hipMemcpyAsync(rows, c->rep.sp.rows(0, n_entries), (size_t)n_entries * 24, hipMemcpyDeviceToHost, s));
	}
	HIP_TRY(c, hipStreamSynchronize(s));
	spectrum_timed(c, 0, bins);
	return 0;
}

int
ntedit_hip_spectrum_info(ntedit_hip_ctx* c, ntedit_hip_spectrum_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "spectrum_info: bad argument");
	}
	*st = c->rep.sp.last;
	return 0;
}

// ------------------------------------------------------------------------------------------------ the spectrum by copy number

int
ntedit_hip_set_cn(ntedit_hip_ctx* c, int on, uint64_t store_cap_bytes)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	cn_switch(c->cn, on != 0, store_cap_bytes);
	return 0;
}

int
ntedit_hip_cn_append(ntedit_hip_ctx* c, int which, const char* bases, uint64_t n, int on_device, const uint64_t* offs, const uint32_t* lens,
                     uint32_t n_entries)
{
	const BatchArg b = { bases, n, on_device, offs, lens, n_entries };
	int rc = b.check(c, "cn_append", which >= 0 && which <= 1);
	if (rc) {
		return rc;
	}
	if (c->cn.state == CN_OFF) { // (answered before the device is touched)
		return fail(c, NTEDIT_E_ARG, "cn_append: the copy numbers are switched off (ntedit_hip_set_cn)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	if ((rc = spectrum_refuse(c, "cn_append")) || (rc = b.layout(c, "cn_append"))) {
		return rc;
	}
	std::string why;
	if ((rc = cn_append(c->cn, which, c->stream, bases, n, offs, lens, n_entries, &why))) {
		return fail(c, rc, "%s", why.c_str());
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the caller's arrays are free again)
	return 0;
}

int
ntedit_hip_cn_finish(ntedit_hip_ctx* c, uint64_t sketch_counters)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	if (sketch_counters && ((sketch_counters & (sketch_counters - 1)) || sketch_counters < CN_FLOOR_COUNTERS || sketch_counters > CN_MAX_COUNTERS)) {
		return fail(c, NTEDIT_E_ARG, "cn_finish: the sketch takes a power of two of 2^20 to 2^36 counters (from 2^6 to force collisions), or 0 for the default");
	}
	switch (c->cn.state) {
	case CN_OFF:
		return fail(c, NTEDIT_E_ARG, "cn_finish: the copy numbers are switched off (ntedit_hip_set_cn)");
	case CN_OVER_CAP:
		return fail(c, NTEDIT_E_OVERFLOW, "cn_finish: the draft passed the store's cap of %llu bytes and the store was released", (unsigned long long)c->cn.cap);
	case CN_NO_MEMORY:
		return fail(c, NTEDIT_E_OVERFLOW, "cn_finish: the device had no memory for the draft and the store was released");
	default:
		break;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = spectrum_refuse(c, "cn_finish");
	if (rc || (rc = refresh_params(c))) {
		return rc;
	}
	std::string why;
	const u64 counters = sketch_counters ? sketch_counters : cn_default_counters(c->cn);
	if ((rc = cn_finish(c->cn, c->stream, dev_filter(c->filt[0]), c->dp, c->d_tab, counters, &why))) {
		return fail(c, rc, "%s", why.c_str());
	}
	return 0;
}

int
ntedit_hip_cn_table(ntedit_hip_ctx* c, int which, uint64_t* occ, uint64_t* w5)
{
	if (!c || which < 0 || which > 1 || !occ || !w5) {
		return fail(c, NTEDIT_E_ARG, "cn_table: bad argument");
	}
	if (!c->cn.finished) {
		return fail(c, NTEDIT_E_ARG, "cn_table: no results: ntedit_hip_set_cn, the batches, then ntedit_hip_cn_finish");
	}
	const u64* t = c->cn.table[which].data();
	memcpy(occ, t, (size_t)CN_CLASSES * CN_BINS * 8);
	memcpy(w5, t + CN_CLASSES * CN_BINS, (size_t)CN_BINS * 8);
	return 0;
}

int
ntedit_hip_cn_rows(ntedit_hip_ctx* c, int which, ntedit_hip_cn_row* rows, uint64_t n)
{
	if (!c || which < 0 || which > 1 || (n && !rows)) {
		return fail(c, NTEDIT_E_ARG, "cn_rows: bad argument");
	}
	if (!c->cn.finished) {
		return fail(c, NTEDIT_E_ARG, "cn_rows: no results: ntedit_hip_set_cn, the batches, then ntedit_hip_cn_finish");
	}
	if (n != c->cn.entries[which]) {
		return fail(c, NTEDIT_E_ARG, "cn_rows: the side holds %llu entries", (unsigned long long)c->cn.entries[which]);
	}
	static_assert(sizeof(ntedit_hip_cn_row) == CN_ROW_WORDS * 8, "a row is six words");
	if (n) {
		memcpy(rows, c->cn.rows[which].data(), (size_t)n * sizeof(ntedit_hip_cn_row));
	}
	return 0;
}

int
ntedit_hip_cn_info(ntedit_hip_ctx* c, ntedit_hip_cn_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "cn_info: bad argument");
	}
	const CnStore& s = c->cn;
	memset(st, 0, sizeof *st);
	st->state = (uint32_t)s.state;
	st->finished = s.finished ? 1 : 0;
	for (int w = 0; w < 2; w++) {
		st->batches[w] = s.side[w].size();
		st->bytes[w] = s.bytes[w];
		st->entries[w] = s.entries[w];
		st->nonzero[w] = s.nonzero[w];
	}
	st->cap = s.cap;
	st->counters = s.counters;
	for (int i = 0; i < 4; i++) {
		st->ms[i] = s.ms[i];
	}
	return 0;
}

int
ntedit_hip_cn_reset(ntedit_hip_ctx* c)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	cn_reset(c->cn);
	return 0;
}

int
ntedit_hip_cn_free(ntedit_hip_ctx* c)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	cn_free(c->cn);
	return 0;
}

// ------------------------------------------------------------------------------------------------ the BGZF writer
int
ntedit_hip_set_fa_names(ntedit_hip_ctx* c, const char* const* names, uint32_t n)
{
	if (!c || (n && !names)) {
		return fail(c, NTEDIT_E_ARG, "set_fa_names: bad argument");
	}
	for (uint32_t i = 0; i < n; i++) {
		if (!names[i]) {
			return fail(c, NTEDIT_E_ARG, "set_fa_names: name %u is NULL", i);
		}
	}
	c->rep.bz.fa_names.assign(names, names + n);
	c->rep.bz.fa_names_set = true;
	return 0;
}

int
ntedit_hip_result_fa_bgzf(const ntedit_hip_result* r, const uint8_t** host, uint64_t* n_bytes, uint64_t* n_plain, uint32_t* n_members)
{
	const int rc = result_check(r, "result_fa_bgzf", true, NTEDIT_HIP_APPLY_BGZF);
	if (rc) {
		return rc;
	}
	if (host) {
		*host = (const uint8_t*)r->bgzf_buf.p;
	}
	if (n_bytes) {
		*n_bytes = r->bgzf_bytes;
	}
	if (n_plain) {
		*n_plain = r->bgzf_plain;
	}
	if (n_members) {
		*n_members = r->bgzf_members;
	}
	return 0;
}

int
ntedit_hip_bgzf_deflate(ntedit_hip_ctx* c, const void* src, uint64_t n, int on_device, uint8_t* out, uint64_t cap, uint64_t* n_out)
{
	if (!c || !n_out || (n && !src) || (cap && !out) || (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE)) {
		return fail(c, NTEDIT_E_ARG, "bgzf_deflate: bad argument");
	}
	*n_out = 0;
	std::string why;
	BgzfTotals t;
	const u8* d_src = (const u8*)src;
	int rc = 0;
	if (on_device == NTEDIT_HIP_BASES_HOST && n) {
		rc = bgzf_upload(c, c->device, c->stream, src, n, &d_src, &why);
	}
	if (!rc) {
		rc = bgzf_encode(c, c->device, c->stream, d_src, n, &t, &why);
	}
	if (rc) {
		return fail(c, rc, "bgzf_deflate: %s", why.c_str());
	}
	*n_out = t.bytes;
	c->rep.bz.last = { 0.f, t.ms_deflate, 0.f, t.plain, t.bytes, t.members, t.stored };
	if (t.bytes > cap) {
		return fail(c, NTEDIT_E_OVERFLOW, "bgzf_deflate: the members take %llu bytes, the buffer has %llu", (unsigned long long)t.bytes, (unsigned long long)cap);
	}
	if ((rc = bgzf_fetch(c, c->stream, out, t.bytes, &c->rep.bz.last.ms_copy, &why))) {
		return fail(c, rc, "bgzf_deflate: %s", why.c_str());
	}
	return 0;
}

int
ntedit_hip_bgzf_info(ntedit_hip_ctx* c, ntedit_hip_bgzf_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "bgzf_info: bad argument");
	}
	*st = c->rep.bz.last;
	return 0;
}

// ------------------------------------------------------------------------------------------------ the completeness marks
// why the context cannot hold marks (0: it can)
static int
shared_refuse(ntedit_hip_ctx* c, const char* who)
{
	const DevFilter& f = c->filt[0];
	if (!f.set) {
		return fail(c, NTEDIT_E_ARG, "%s: no primary Bloom filter to measure completeness against", who);
	}
	if (f.counting) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "%s: completeness takes a plain primary filter; a counting filter's slots are counters", who);
	}
	if (f.k > QV_MAX_K) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "%s: the completeness marks take k up to %u", who, QV_MAX_K);
	}
	return 0;
}

static int
shared_zero(ntedit_hip_ctx* c)
{
	const size_t padded = (size_t)((c->rep.sh.bytes + 7) / 8 * 8);
	for (auto& m : c->rep.sh.marks) {
		HIP_TRY(c, hipMemsetAsync(m.p, 0, padded, c->stream));
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	c->rep.sh.calls = 0;
	c->rep.sh.ms[0] = c->rep.sh.ms[1] = 0.f;
	return 0;
}

static int
shared_begin(ntedit_hip_ctx* c, const char* who)
{
	int rc = shared_refuse(c, who);
	if (rc) {
		return rc;
	}
	if (c->rep.sh.bytes) {
		return 0; // (the marks of this filter: drop_filter releases them with it)
	}
	if ((rc = ensure_events(c, c->rep.sh.window))) {
		return rc;
	}
	// (whole 64-bit words, as the filter's own allocation: k_popcount reads words, k_mark ORs into 32-bit ones)
	const size_t padded = (size_t)((c->filt[0].nbytes + 7) / 8 * 8);
	for (auto& m : c->rep.sh.marks) {
		release(m);
		if (hipMalloc(&m.p, padded) != hipSuccess) {
			(void)hipGetLastError();
			c->rep.sh.release_marks();
			return fail(c, NTEDIT_E_DEVICE, "%s: no device memory for two mark arrays of %llu bytes", who, (unsigned long long)padded);
		}
		m.cap = padded;
	}
	c->rep.sh.bytes = c->filt[0].nbytes;
	if ((rc = shared_zero(c))) {
		c->rep.sh.release_marks();
	}
	return rc;
}

// k_mark over a batch and its absent bitmap into M[which], on `stream`, inside the window of that array
static int
launch_mark(ntedit_hip_ctx* c, hipStream_t stream, const u8* d_seq, u64 n, const Filter& f, const u64* d_bitmap, u64 n_words, int which)
{
	const u64 blocks = (n + SCREEN_TILE - 1) / SCREEN_TILE;
	if (blocks == 0) {
		return 0;
	}
	if (blocks > 0x7FFFFFFFull) {
		return fail(c, NTEDIT_E_ARG, "batch too large");
	}
	if (!c->rep.sh.bytes || c->rep.sh.bytes != c->filt[0].nbytes || f.counting) {
		return fail(c, NTEDIT_E_INTERNAL, "mark: the marks are not those of the primary filter");
	}
	u32* marks = (u32*)c->rep.sh.marks[which].p;
	HIP_TRY(c, hipEventRecord(c->rep.sh.window[which].begin, stream));
	if (f.mask) {
		hipLaunchKernelGGL((k_mark<true>), dim3((unsigned)blocks), dim3(SCREEN_TPB), 0, stream, d_seq, n, f, c->dp.k, c->d_tab, d_bitmap, n_words, marks);
	} else {
		hipLaunchKernelGGL((k_mark<false>), dim3((unsigned)blocks), dim3(SCREEN_TPB), 0, stream, d_seq, n, f, c->dp.k, c->d_tab, d_bitmap, n_words, marks);
	}
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(c->rep.sh.window[which].end, stream));
	c->rep.sh.calls++;
	return 0;
}

// after `stream` has been waited for: the launch's time goes to its array's sum
static void
mark_timed(ntedit_hip_ctx* c, int which)
{
	c->rep.sh.ms[which] += elapsed_ms(c->rep.sh.window[which]);
}

int
ntedit_hip_shared_begin(ntedit_hip_ctx* c)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	return shared_begin(c, "shared_begin");
}

int
ntedit_hip_shared_reset(ntedit_hip_ctx* c)
{
	if (!c || !c->rep.sh.bytes) {
		return fail(c, NTEDIT_E_ARG, "shared_reset: no marks (ntedit_hip_shared_begin)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	return shared_zero(c);
}

void
ntedit_hip_shared_free(ntedit_hip_ctx* c)
{
	if (c && hipSetDevice(c->device) == hipSuccess) {
		(void)hipStreamSynchronize(c->stream);
		c->rep.sh.release_marks();
	}
}

int
ntedit_hip_shared_mark(ntedit_hip_ctx* c, int which, const char* bases, uint64_t n, int on_device)
{
	const BatchArg b = { bases, n, on_device, nullptr, nullptr, 0 };
	int rc = b.check(c, "shared_mark", which >= 0 && which <= 1);
	if (rc) {
		return rc;
	}
	HIP_TRY(c, hipSetDevice(c->device));
	if ((rc = shared_begin(c, "shared_mark")) || (rc = refresh_params(c))) { // (the marks are begun before the parameters are looked at)
		return rc;
	}
	if (n == 0) {
		return 0;
	}
	const u64 n_words = (n + 63) / 64;
	const u8* d_seq = nullptr;
	if ((rc = stage_bases(c, bases, n, on_device, &d_seq)) || (rc = ensure(c, c->bitmap, (n_words + 8) * 8))) {
		return rc;
	}
	u64* d_bitmap = (u64*)c->bitmap.p;
	const Filter f0 = dev_filter(c->filt[0]);
	PlainScreen plain(c);
	if ((rc = screen_whole(c, d_seq, n, f0, d_bitmap, n_words)) || (rc = launch_mark(c, c->stream, d_seq, n, f0, d_bitmap, n_words, which))) {
		(void)hipStreamSynchronize(c->stream);
		return rc;
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	mark_timed(c, which);
	return 0;
}

int
ntedit_hip_shared_download(ntedit_hip_ctx* c, int which, uint8_t* bits)
{
	if (!c || which < 0 || which > 1 || !bits || !c->rep.sh.bytes) {
		return fail(c, NTEDIT_E_ARG, "shared_download: bad argument, or no marks (ntedit_hip_shared_begin)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(bits, c->rep.sh.marks[which].p, c->rep.sh.bytes, hipMemcpyDeviceToHost));
	return 0;
}

int
ntedit_hip_shared_counts(ntedit_hip_ctx* c, ntedit_hip_shared_stats* st)
{
	if (!c || !st || !c->rep.sh.bytes || !c->filt[0].set || c->filt[0].nbytes != c->rep.sh.bytes) {
		return fail(c, NTEDIT_E_ARG, "shared_counts: bad argument, or no marks (ntedit_hip_shared_begin)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	const DevFilter& f = c->filt[0];
	int rc = ensure(c, c->counters, 256);
	if (rc) {
		return rc;
	}
	unsigned long long* d_total = (unsigned long long*)c->counters.p;
	HIP_TRY(c, hipMemsetAsync(d_total, 0, 24, c->stream));
	const u64 n_words = (f.nbytes + 7) / 8; // (all three allocations are whole 64-bit words, zero behind nbytes)
	const u64* arrays[3] = { (const u64*)f.data, (const u64*)c->rep.sh.marks[0].p, (const u64*)c->rep.sh.marks[1].p };
	for (int i = 0; i < 3; i++) {
		hipLaunchKernelGGL(k_popcount, dim3((unsigned)(c->cu_count * 8)), dim3(256), 0, c->stream, arrays[i], n_words, 0, d_total + i);
	}
	HIP_TRY(c, hipGetLastError());
	unsigned long long h[3] = { 0, 0, 0 };
	HIP_TRY(c, hipMemcpyAsync(h, d_total, 24, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	memset(st, 0, sizeof *st);
	st->bits = f.nbytes * 8;
	st->hash_num = f.hash_num;
	st->k = f.k;
	st->filter_set = h[0];
	st->shared_set[0] = h[1];
	st->shared_set[1] = h[2];
	st->marked_calls = c->rep.sh.calls;
	st->ms_mark[0] = c->rep.sh.ms[0];
	st->ms_mark[1] = c->rep.sh.ms[1];
	return 0;
}

