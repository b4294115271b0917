// nte_api_results.inc -- part of nte_api.hip: the C ABI of results (statistics, edit records, rendering through
// host/render.cpp), host helpers (page-locked memory, NUMA binding), tuning knobs and the gather micro-benchmark.
extern "C" {

void
ntedit_hip_result_free(ntedit_hip_result* r)
{
	if (!r) {
		return;
	}
	// (a result may outlive its context: its pinned buffers are then released directly)
	pin_give(r->owner, r->arena_buf);
	pin_give(r->owner, r->first_buf);
	bgzf_pin_give(r->owner, r->bgzf_buf);
	if (r->edited.p) {
		// the edited bases go back to a context that has no buffer of its own by now, or to the device
		bool kept = false;
		if (r->owner && ctx_alive(r->owner)) {
			std::lock_guard<std::mutex> lk(r->owner->pin_mu);
			if (!r->owner->ap_edited.p) {
				r->owner->ap_edited = r->edited;
				kept = true;
			}
		}
		if (!kept) {
			(void)hipFree(r->edited.p);
		}
		r->edited = DevBuf();
	}
	delete r;
}

static thread_local std::string g_result_err;

const char*
ntedit_hip_result_last_error(void)
{
	return g_result_err.c_str();
}

static int
result_refuse(const ntedit_hip_result* r, const char* what)
{
	g_result_err = what;
	if (r && r->owner && ctx_alive(r->owner)) {
		r->owner->err = what;
	}
	return NTEDIT_E_ARG;
}

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
	if (!r || !dev_ptr || !n_bytes) {
		return result_refuse(r, "result_edited: bad argument");
	}
	if (!(r->apply_flags & NTEDIT_HIP_APPLY_EDITED)) {
		return result_refuse(r, "result_edited: the batch was polished without the APPLY_EDITED flag (ntedit_hip_set_apply)");
	}
	if (n_contigs != r->e_offs.size() && (offsets_out || lens_out)) {
		return result_refuse(r, "result_edited: the batch had another number of entries");
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
		g_result_err = "result_edited: the buffer is too small";
		return NTEDIT_E_OVERFLOW;
	}
	if (nb && (hipSetDevice(r->device) != hipSuccess || hipMemcpy(host_buf, d, nb, hipMemcpyDeviceToHost) != hipSuccess)) {
		g_result_err = "result_edited: the download failed";
		return NTEDIT_E_DEVICE;
	}
	return 0;
}

int
ntedit_hip_result_qv(const ntedit_hip_result* r, ntedit_hip_qv_row* rows, uint32_t n_contigs)
{
	if (!r || (n_contigs && !rows)) {
		return result_refuse(r, "result_qv: bad argument");
	}
	if (!(r->apply_flags & NTEDIT_HIP_APPLY_QV)) {
		return result_refuse(r, "result_qv: the batch was polished without the APPLY_QV flag (ntedit_hip_set_apply)");
	}
	if (n_contigs != r->qv.size()) {
		return result_refuse(r, "result_qv: the batch had another number of entries");
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
	*st = c->apply_last;
	return 0;
}

uint32_t
ntedit_hip_apply_tile(void)
{
	return APPLY_TILE;
}

// ---- the interval extractor (nte_track.hip)
static_assert(sizeof(ntedit_hip_track_interval) == sizeof(TrackInterval) && sizeof(TrackInterval) == 16, "the records are copied as they stand");

int
ntedit_hip_result_track(const ntedit_hip_result* r, int which, ntedit_hip_track_interval* out, uint64_t cap, uint64_t* n)
{
	if (!r || !n || which < 0 || which > 1 || (cap && !out)) {
		return result_refuse(r, "result_track: bad argument");
	}
	if (!(r->apply_flags & NTEDIT_HIP_APPLY_TRACK)) {
		return result_refuse(r, "result_track: the batch was polished without the APPLY_TRACK flag (ntedit_hip_set_apply)");
	}
	*n = r->track_n[which];
	if (*n > cap) {
		g_result_err = "result_track: the buffer is too small";
		return NTEDIT_E_OVERFLOW;
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
	if (!c || !n || (n_positions && !bitmap) || (n_entries && (!offs || !lens)) || (cap && !out)) {
		return fail(c, NTEDIT_E_ARG, "track_extract: bad argument");
	}
	*n = 0;
	if (k == 0 || k > TRACK_MAX_K) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "track_extract: k from 1 to %u", TRACK_MAX_K);
	}
	if (const u32 bad = nte_host::first_layout_break(n_positions, offs, lens, n_entries, false); bad != nte_host::LAYOUT_OK) {
		return fail(c, NTEDIT_E_ARG, "track_extract: entry %u breaks the batch layout", bad);
	}
	HIP_TRY(c, hipSetDevice(c->device));
	c->track_last = ntedit_hip_track_stats{ { 0.f, 0.f }, { 0, 0 }, { 0, 0 } };
	if (n_positions == 0 || n_entries == 0) {
		return 0;
	}
	int rc;
	const u64 n_words = (n_positions + 63) / 64;
	if ((rc = ensure(c, c->ap_bitmap, (size_t)(n_words + 8) * 8)) || (rc = ensure(c, c->offs, (size_t)n_entries * 8)) ||
	    (rc = ensure(c, c->lens, (size_t)n_entries * 4))) {
		return rc;
	}
	hipStream_t s = c->stream;
	HIP_TRY(c, hipMemcpyAsync(c->ap_bitmap.p, bitmap, (size_t)n_words * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(c, hipMemcpyAsync(c->offs.p, offs, (size_t)n_entries * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(c, hipMemcpyAsync(c->lens.p, lens, (size_t)n_entries * 4, hipMemcpyHostToDevice, s));
	ntedit_hip_track_interval* recs = nullptr;
	u64 n_recs = 0;
	rc = track_run(c, s, (const u64*)c->ap_bitmap.p, n_positions, (const u64*)c->offs.p, (const u32*)c->lens.p, n_entries, k, 0, &recs, &n_recs);
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
	*st = c->track_last;
	return 0;
}

// ---- the k-mer spectrum (k_spectrum, nte_kernels.hip; the helpers are in nte_api_screen.inc)

int
ntedit_hip_set_spectrum(ntedit_hip_ctx* c, int on)
{
	if (!c) {
		return NTEDIT_E_ARG;
	}
	c->spectrum_on = on != 0;
	return 0;
}

int
ntedit_hip_result_spectrum(const ntedit_hip_result* r, int which, uint64_t bins[256])
{
	if (!r || !bins || which < 0 || which > 1) {
		return result_refuse(r, "result_spectrum: bad argument");
	}
	if (!r->spectrum) {
		return result_refuse(r, "result_spectrum: the batch was polished with the spectrum switched off (ntedit_hip_set_spectrum)");
	}
	memcpy(bins, r->sp_bins.data() + (size_t)which * SPECTRUM_BINS, SPECTRUM_BINS * 8);
	return 0;
}

int
ntedit_hip_result_depth(const ntedit_hip_result* r, ntedit_hip_depth_row* rows, uint32_t n_contigs)
{
	if (!r || (n_contigs && !rows)) {
		return result_refuse(r, "result_depth: bad argument");
	}
	if (!r->spectrum) {
		return result_refuse(r, "result_depth: the batch was polished with the spectrum switched off (ntedit_hip_set_spectrum)");
	}
	if (n_contigs != r->depth.size()) {
		return result_refuse(r, "result_depth: the batch had another number of entries");
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
	if (!c || !bins || (n && !bases) || (n_entries && (!offs || !lens))) {
		return fail(c, NTEDIT_E_ARG, "spectrum_count: bad argument");
	}
	if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
		return fail(c, NTEDIT_E_ARG, "spectrum_count: bases must be host or device bytes");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = spectrum_refuse(c, "spectrum_count");
	if (rc || (rc = refresh_params(c))) {
		return rc;
	}
	if (const u32 bad = nte_host::first_layout_break(n, offs, lens, n_entries, false); bad != nte_host::LAYOUT_OK) {
		return fail(c, NTEDIT_E_ARG, "spectrum_count: entry %u breaks the batch layout", bad);
	}
	memset(bins, 0, SPECTRUM_BINS * 8);
	if (rows && n_entries) {
		memset(rows, 0, (size_t)n_entries * 24);
	}
	c->spectrum_last = ntedit_hip_spectrum_stats{ { 0.f, 0.f }, { 0, 0 } };
	if (n == 0 || n_entries == 0) {
		return 0;
	}
	hipStream_t s = c->stream;
	const u8* d_seq = nullptr;
	if ((rc = stage_bases(c, bases, n, on_device, &d_seq)) || (rc = ensure(c, c->offs, (size_t)n_entries * 8)) ||
	    (rc = ensure(c, c->lens, (size_t)n_entries * 4)) || (rc = spectrum_begin(c, s, n_entries))) {
		return rc;
	}
	HIP_TRY(c, hipMemcpyAsync(c->offs.p, offs, (size_t)n_entries * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(c, hipMemcpyAsync(c->lens.p, lens, (size_t)n_entries * 4, hipMemcpyHostToDevice, s));
	const Filter f0 = dev_filter(c->filt[0]);
	if ((rc = launch_spectrum(c, s, d_seq, n, f0, (const u64*)c->offs.p, (const u32*)c->lens.p, n_entries, 0, rows != nullptr))) {
		(void)hipStreamSynchronize(s);
		return rc;
	}
	HIP_TRY(c, hipMemcpyAsync(bins, spectrum_bins(c, 0), SPECTRUM_BINS * 8, hipMemcpyDeviceToHost, s));
	if (rows) {
		HIP_TRY(c, hipMemcpyAsync(rows, spectrum_rows(c, 0, n_entries), (size_t)n_entries * 24, hipMemcpyDeviceToHost, s));
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
	*st = c->spectrum_last;
	return 0;
}

// ---- the spectrum by copy number (nte_cn.hip: the draft store, k_cn_count, k_spectrum_cn)

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
	if (!c || which < 0 || which > 1 || (n && !bases) || (n_entries && (!offs || !lens))) {
		return fail(c, NTEDIT_E_ARG, "cn_append: bad argument");
	}
	if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
		return fail(c, NTEDIT_E_ARG, "cn_append: bases must be host or device bytes");
	}
	if (c->cn.state == CN_OFF) {
		return fail(c, NTEDIT_E_ARG, "cn_append: the copy numbers are switched off (ntedit_hip_set_cn)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = spectrum_refuse(c, "cn_append");
	if (rc) {
		return rc;
	}
	if (const u32 bad = nte_host::first_layout_break(n, offs, lens, n_entries, false); bad != nte_host::LAYOUT_OK) {
		return fail(c, NTEDIT_E_ARG, "cn_append: entry %u breaks the batch layout", bad);
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

// ---- the BGZF writer (nte_bgzf_deflate.hip)

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
	c->fa_names.assign(names, names + n);
	c->fa_names_set = true;
	return 0;
}

int
ntedit_hip_result_fa_bgzf(const ntedit_hip_result* r, const uint8_t** host, uint64_t* n_bytes, uint64_t* n_plain, uint32_t* n_members)
{
	if (!r) {
		return result_refuse(r, "result_fa_bgzf: bad argument");
	}
	if (!(r->apply_flags & NTEDIT_HIP_APPLY_BGZF)) {
		return result_refuse(r, "result_fa_bgzf: the batch was polished without the APPLY_BGZF flag (ntedit_hip_set_apply)");
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
	c->bgzf_last = { 0.f, t.ms_deflate, 0.f, t.plain, t.bytes, t.members, t.stored };
	if (t.bytes > cap) {
		return fail(c, NTEDIT_E_OVERFLOW, "bgzf_deflate: the members take %llu bytes, the buffer has %llu", (unsigned long long)t.bytes, (unsigned long long)cap);
	}
	if ((rc = bgzf_fetch(c, c->stream, out, t.bytes, &c->bgzf_last.ms_copy, &why))) {
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
	*st = c->bgzf_last;
	return 0;
}

// ---- the completeness marks (k_mark, nte_kernels.hip; the helpers are in nte_api_screen.inc)

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
	if (!c || !c->sh_bytes) {
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
		shared_release(c);
	}
}

int
ntedit_hip_shared_mark(ntedit_hip_ctx* c, int which, const char* bases, uint64_t n, int on_device)
{
	if (!c || which < 0 || which > 1 || (n && !bases)) {
		return fail(c, NTEDIT_E_ARG, "shared_mark: bad argument");
	}
	if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
		return fail(c, NTEDIT_E_ARG, "shared_mark: bases must be host or device bytes");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = shared_begin(c, "shared_mark");
	if (rc || (rc = refresh_params(c))) {
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
	if (!c || which < 0 || which > 1 || !bits || !c->sh_bytes) {
		return fail(c, NTEDIT_E_ARG, "shared_download: bad argument, or no marks (ntedit_hip_shared_begin)");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	HIP_TRY(c, hipMemcpy(bits, c->sh_marks[which].p, c->sh_bytes, hipMemcpyDeviceToHost));
	return 0;
}

int
ntedit_hip_shared_counts(ntedit_hip_ctx* c, ntedit_hip_shared_stats* st)
{
	if (!c || !st || !c->sh_bytes || !c->filt[0].set || c->filt[0].nbytes != c->sh_bytes) {
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
	const u64* arrays[3] = { (const u64*)f.data, (const u64*)c->sh_marks[0].p, (const u64*)c->sh_marks[1].p };
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
	st->marked_calls = c->sh_calls;
	st->ms_mark[0] = c->sh_ms[0];
	st->ms_mark[1] = c->sh_ms[1];
	return 0;
}

int
ntedit_hip_result_stats(const ntedit_hip_result* r, ntedit_hip_stats* s)
{
	if (!r || !s) {
		return NTEDIT_E_ARG;
	}
	*s = r->st;
	s->events_applied = r->rst.events_applied;
	s->substitutions = r->rst.substitutions;
	s->insertions = r->rst.insertions;
	s->deletions = r->rst.deletions;
	return 0;
}

struct ntedit_hip_annot
{
	nte_host::Annotations* a = nullptr;
};

int
ntedit_hip_annot_load(const char* vcf_path, ntedit_hip_annot** out)
{
	if (!vcf_path || !out) {
		return NTEDIT_E_ARG;
	}
	nte_host::Annotations* a = nte_host::annotations_load(vcf_path);
	if (!a) {
		return NTEDIT_E_IO;
	}
	*out = new ntedit_hip_annot();
	(*out)->a = a;
	return 0;
}

void
ntedit_hip_annot_free(ntedit_hip_annot* a)
{
	if (a) {
		nte_host::annotations_free(a->a);
		delete a;
	}
}

int
ntedit_hip_write_vcf_header(const char* vcf_path, const char* draft_filename)
{
	FILE* v = fopen(vcf_path, "wb");
	if (!v) {
		return NTEDIT_E_IO;
	}
	nte_host::write_vcf_header(v, draft_filename ? draft_filename : "");
	return fclose(v) == 0 ? 0 : NTEDIT_E_IO;
}

int
ntedit_hip_write_outputs_ex(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const ntedit_hip_write_options* wo)
{
	if (!r || !wo || (n_contigs && (!bases || !offsets || !lens || !names))) {
		return NTEDIT_E_ARG;
	}
	const char* fa_path = wo->fa_path;
	const char* tsv_path = wo->tsv_path;
	const char* vcf_path = wo->vcf_path;
	const int append = wo->append;
	FILE* fa = fa_path ? fopen(fa_path, append ? "ab" : "wb") : nullptr;
	FILE* tsv = tsv_path ? fopen(tsv_path, append ? "ab" : "wb") : nullptr;
	FILE* vcf = vcf_path ? fopen(vcf_path, append ? "ab" : "wb") : nullptr;
	if ((fa_path && !fa) || (tsv_path && !tsv) || (vcf_path && !vcf)) {
		if (fa) {
			fclose(fa);
		}
		if (tsv) {
			fclose(tsv);
		}
		if (vcf) {
			fclose(vcf);
		}
		return NTEDIT_E_IO;
	}
	if (fa) {
		setvbuf(fa, nullptr, _IOFBF, 4 << 20);
	}
	if (tsv) {
		setvbuf(tsv, nullptr, _IOFBF, 1 << 20);
	}
	if (vcf) {
		setvbuf(vcf, nullptr, _IOFBF, 1 << 20);
	}
	ntedit_hip_result* rw = const_cast<ntedit_hip_result*>(r);
	rw->rst = nte_host::RenderStats();
	nte_host::RenderOptions opt;
	opt.threads = g_host_threads.load();
	opt.snv = r->snv != 0;
	opt.annot = wo->annot ? wo->annot->a : nullptr;
	opt.segments = wo->segments;
	opt.out_sizes = wo->out_sizes;
	opt.part_margin = r->part_margin;
	if (wo->out_sizes) {
		memset(wo->out_sizes, 0, (size_t)n_contigs * 3 * sizeof(uint64_t));
	}
	int rc = nte_host::render_batch(
	    (const Item*)r->arena_buf.p,
	    r->arena_items,
	    (const u32*)r->first_buf.p,
	    r->n_ev_first,
	    bases,
	    offsets,
	    lens,
	    names,
	    n_contigs,
	    fa,
	    tsv,
	    &rw->rst,
	    vcf,
	    &opt);
	if (fa && fclose(fa) != 0) {
		rc = rc ? rc : -5;
	}
	if (tsv && fclose(tsv) != 0) {
		rc = rc ? rc : -5;
	}
	if (vcf && fclose(vcf) != 0) {
		rc = rc ? rc : -5;
	}
	if (rc == -7 || rc == -8) {
		return NTEDIT_E_SEGMENT;
	}
	if (rc == -9) {
		// (render.cpp: a MOD outside its part, a run that ends behind its part: the margin k + max_deletions + 48 that
		// the parts of a contig are cut with was crossed -- never seen; the hostsim tier renders with parts of one base)
		if (r->owner) {
			r->owner->err = "renderer: an event reaches across the margin its contig's parts were cut with (outputs incomplete)";
		}
		return NTEDIT_E_INTERNAL;
	}
	return rc ? NTEDIT_E_IO : 0;
}

int
ntedit_hip_write_outputs_vcf(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const char* fa_path,
    const char* tsv_path,
    const char* vcf_path,
    int append,
    int snv,
    const ntedit_hip_annot* annot)
{
	(void)snv; // (SNV mode follows the parameters the batch was polished with)
	ntedit_hip_write_options wo;
	memset(&wo, 0, sizeof wo);
	wo.fa_path = fa_path;
	wo.tsv_path = tsv_path;
	wo.vcf_path = vcf_path;
	wo.append = append;
	wo.annot = annot;
	return ntedit_hip_write_outputs_ex(r, bases, offsets, lens, names, n_contigs, &wo);
}

int
ntedit_hip_result_cover_ends(const ntedit_hip_result* r, uint32_t n_contigs, uint32_t* cover_ends)
{
	if (!r || (n_contigs && !cover_ends)) {
		return NTEDIT_E_ARG;
	}
	return nte_host::cover_ends((const Item*)r->arena_buf.p, r->arena_items, (const u32*)r->first_buf.p, r->n_ev_first,
	                            n_contigs, cover_ends)
	           ? NTEDIT_E_ARG
	           : 0;
}

int
ntedit_hip_result_cuts_ok(const ntedit_hip_result* r, uint32_t n_contigs, const uint32_t* lens, const ntedit_hip_segment* segments, uint8_t* ok)
{
	if (!r || (n_contigs && (!lens || !segments || !ok))) {
		return NTEDIT_E_ARG;
	}
	std::vector<u32> halos(n_contigs);
	for (u32 i = 0; i < n_contigs; i++) {
		halos[i] = segments[i].halo;
	}
	return nte_host::cuts_ok((const Item*)r->arena_buf.p, r->arena_items, (const u32*)r->first_buf.p, r->n_ev_first, n_contigs, lens,
	                         halos.data(), ok)
	           ? NTEDIT_E_ARG
	           : 0;
}

int
ntedit_hip_result_edits(
    ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    uint32_t n_contigs,
    const ntedit_hip_segment* segments,
    const ntedit_hip_edit** edits,
    uint64_t* n_edits,
    const char** base_pool)
{
	if (!r || !edits || !n_edits || (n_contigs && (!bases || !offsets || !lens))) {
		return NTEDIT_E_ARG;
	}
	if (!r->edits_built) {
		r->edits.clear();
		r->edit_pool.clear();
		std::vector<const char*> names(n_contigs, "");
		nte_host::RenderOptions opt;
		opt.threads = g_host_threads.load();
		opt.snv = r->snv != 0;
		opt.segments = segments;
		opt.part_margin = r->part_margin;
		opt.edits = &r->edits;
		opt.edit_pool = &r->edit_pool;
		nte_host::RenderStats st;
		const int rc = nte_host::render_batch(
		    (const Item*)r->arena_buf.p, r->arena_items, (const u32*)r->first_buf.p, r->n_ev_first, bases, offsets, lens,
		    names.data(), n_contigs, nullptr, nullptr, &st, nullptr, &opt);
		if (rc) {
			r->edits.clear();
			r->edit_pool.clear();
			return rc == -7 || rc == -8 ? NTEDIT_E_SEGMENT : NTEDIT_E_ARG;
		}
		r->edits_built = true;
	}
	*edits = r->edits.data();
	*n_edits = r->edits.size();
	if (base_pool) {
		*base_pool = r->edit_pool.c_str();
	}
	return 0;
}

int
ntedit_hip_write_outputs(
    const ntedit_hip_result* r,
    const char* bases,
    const uint64_t* offsets,
    const uint32_t* lens,
    const char* const* names,
    uint32_t n_contigs,
    const char* fa_path,
    const char* tsv_path,
    int append)
{
	return ntedit_hip_write_outputs_vcf(r, bases, offsets, lens, names, n_contigs, fa_path, tsv_path, nullptr, append, 0, nullptr);
}

int
ntedit_hip_write_tsv_header(const char* tsv_path, uint32_t k, uint32_t jump, int counting)
{
	FILE* tsv = fopen(tsv_path, "wb");
	if (!tsv) {
		return NTEDIT_E_IO;
	}
	nte_host::write_tsv_header(tsv, k, jump, counting != 0);
	return fclose(tsv) == 0 ? 0 : NTEDIT_E_IO;
}

void*
ntedit_hip_host_alloc(size_t bytes)
{
	void* p = nullptr;
	if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
		return nullptr;
	}
	return p;
}

void
ntedit_hip_host_free(void* p)
{
	if (p) {
		(void)hipHostFree(p);
	}
}

int
ntedit_hip_bind_near_device(int device)
{
	if (getenv("NTEDIT_HIP_NO_BIND")) {
		return -1;
	}
	char id[64] = { 0 };
	if (hipDeviceGetPCIBusId(id, (int)sizeof id - 1, device) != hipSuccess) {
		return -1;
	}
	for (char* q = id; *q; q++) {
		*q = (char)tolower((unsigned char)*q);
	}
	char path[256];
	snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", id);
	FILE* f = fopen(path, "r");
	if (!f) {
		return -1;
	}
	int node = -1;
	if (fscanf(f, "%d", &node) != 1) {
		node = -1;
	}
	fclose(f);
	if (node < 0) {
		return -1;
	}
	snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
	f = fopen(path, "r");
	if (!f) {
		return -1;
	}
	// "0-63,128-191"
	cpu_set_t want;
	CPU_ZERO(&want);
	int lo = 0, hi = 0, n_set = 0;
	for (;;) {
		if (fscanf(f, "%d", &lo) != 1) {
			break;
		}
		hi = lo;
		int ch = fgetc(f);
		if (ch == '-') {
			if (fscanf(f, "%d", &hi) != 1) {
				break;
			}
			ch = fgetc(f);
		}
		for (int cpu = lo; cpu <= hi && cpu < CPU_SETSIZE; cpu++) {
			CPU_SET(cpu, &want);
			n_set++;
		}
		if (ch != ',') {
			break;
		}
	}
	fclose(f);
	// only CPUs the process may use anyway; nothing to do when that leaves none (or all)
	cpu_set_t have;
	if (n_set == 0 || sched_getaffinity(0, sizeof have, &have) != 0) {
		return -1;
	}
	cpu_set_t both;
	CPU_AND(&both, &want, &have);
	if (CPU_COUNT(&both) == 0 || CPU_COUNT(&both) == CPU_COUNT(&have)) {
		return -1;
	}
	if (sched_setaffinity(0, sizeof both, &both) != 0) {
		return -1;
	}
	return node;
}

void
ntedit_hip_set_host_threads(unsigned n)
{
	g_host_threads.store(n);
}

} // extern "C"

// (host/fasta_abi.cpp: ntedit_hip_pack_bases with threads = 0)
unsigned
nte_host_threads_setting()
{
	return g_host_threads.load();
}

extern "C" {

float
ntedit_hip_last_kernel_ms(const ntedit_hip_ctx* c)
{
	return c ? c->last_ms : 0.f;
}

int
ntedit_hip_settle_info(ntedit_hip_ctx* c, ntedit_hip_settle_stats* st)
{
	if (!c || !st) {
		return fail(c, NTEDIT_E_ARG, "settle_info: bad argument");
	}
	*st = c->settle_last;
	return 0;
}

#ifndef NTE_BUILD_ID
#define NTE_BUILD_ID "unknown"
#endif
const char*
ntedit_hip_build_id(void)
{
	return NTE_BUILD_ID;
}

// The reference's candidate tables (ntedit.cpp:172, 176-199, 203-348) as the DEVICE code and params.cpp hold them, in
// the text form tests/tools/reference_tables.py extracts from the reference's source and hashes: the GPU tier checks the
// product against those hashes without the reference's text travelling.
int
ntedit_hip_device_tables(ntedit_hip_ctx* c, char* out, uint64_t cap, uint64_t* len)
{
	if (!c || !out || !len) {
		return fail(c, NTEDIT_E_ARG, "device_tables: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	u8* d = nullptr;
	HIP_TRY(c, hipMalloc((void**)&d, TABLES_RAW_BYTES));
	launch_k_tables(c->stream, d);
	std::vector<u8> raw(TABLES_RAW_BYTES);
	hipError_t e = hipMemcpyAsync(raw.data(), d, TABLES_RAW_BYTES, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) {
		e = hipStreamSynchronize(c->stream);
	}
	(void)hipFree(d);
	HIP_TRY(c, e);
	std::string t = "num_tries";
	for (uint32_t i = 0; i <= 5; i++) {
		ntedit_hip_params hp;
		nte_host::params_default(&hp);
		hp.max_insertions = i;
		hp.max_deletions = i < 2 ? i : hp.max_deletions;
		DevParams dp;
		if (nte_host::make_dev_params(hp, 25, 3, false, &dp)) {
			return fail(c, NTEDIT_E_ARG, "device_tables: parameters");
		}
		t += " " + std::to_string(dp.ins_tries);
	}
	t += "\n";
	const char* letters = "ATCGRYSWKMBDHVN";
	for (int snv = 0; snv < 2; snv++) {
		for (int l = 0; l < 15; l++) {
			const u8* o = raw.data() + (snv * 15 + l) * 8;
			t += snv ? "snv " : "polish ";
			t += letters[l];
			t += ' ';
			for (u32 q = 0; q < o[0] && q < 7; q++) {
				t += (char)o[1 + q];
			}
			t += '\n';
		}
	}
	for (int b = 0; b < 4; b++) {
		t += "multi ";
		t += "ACGT"[b];
		for (u32 i = 0; i < 341; i++) {
			const u8* o = raw.data() + 30 * 8 + ((size_t)b * 341 + i) * 8;
			t += ' ';
			for (u32 q = 0; q < o[0] && q < 7; q++) {
				t += (char)o[1 + q];
			}
		}
		t += '\n';
	}
	*len = t.size();
	if (t.size() + 1 > cap) {
		return fail(c, NTEDIT_E_ARG, "device_tables: buffer too small (%zu bytes needed)", t.size() + 1);
	}
	memcpy(out, t.c_str(), t.size() + 1);
	return 0;
}

int
ntedit_hip_set_tuning(ntedit_hip_ctx* c, const char* key, uint64_t value)
{
	if (!c || !key) {
		return fail(c, NTEDIT_E_ARG, "set_tuning: bad argument");
	}
	const std::string k(key);
	auto& t = c->tune;
	if (k == "screen_mode") {
		t.screen_mode = (u32)value;
	} else if (k == "bin_chunk") {
		t.bin_chunk = value;
	} else if (k == "bin_cap_percent") {
		t.bin_cap_percent = (u32)value;
	} else if (k == "force_xcc") {
		t.force_xcc = (u32)value;
	} else if (k == "bin_timing") {
		t.bin_timing = (u32)value;
	} else if (k == "chunk_bytes") {
		t.chunk_bytes = value;
	} else if (k == "h2d_piece") {
		t.h2d_piece = value;
	} else if (k == "inline_tries") {
		t.inline_tries = (u32)value;
		c->dp_valid = false;
	} else if (k == "assess") {
		t.assess = (u32)value;
	} else if (k == "machine_cfg") {
		t.machine_cfg = value ? ~0u : 0u; // (only "general" can be forced: a specialised instantiation is wrong for other configurations)
	} else if (k == "lanes") {
		t.lanes = (u32)value;
		c->dp_valid = false;
	} else if (k == "defer_run") {
		t.defer_run = (u32)value;
		c->dp_valid = false;
	} else if (k == "defer_fail_snv") {
		t.defer_fail_snv = (u32)value;
		c->dp_valid = false;
	} else if (k == "defer_fail") {
		t.defer_fail = (u32)value;
		c->dp_valid = false;
	} else if (k == "h2d_fixed_schedule") {
		t.h2d_fixed_schedule = (u32)value;
	} else if (k == "candmap") {
		t.candmap = (u32)value;
	} else if (k == "snv_wave") {
		t.snv_wave = (u32)value;
	} else if (k == "force_rounds") {
		t.force_rounds = (u32)value;
	} else if (k == "arena_chunks") {
		t.arena_chunks = value;
	} else if (k == "settle") {
		t.settle = value > 1 ? ~0u : (u32)value;
	} else if (k == "no_rounds") {
		t.no_rounds = (u32)value;
	} else if (k == "no_early_copy") {
		t.no_early_copy = (u32)value;
	} else if (k == "bin_scatter") {
		t.bin_scatter = (u32)value;
	} else if (k == "probe_parts_log2") {
		t.probe_parts_log2 = (u32)value;
	} else if (k == "bin_slice_log2") {
		t.bin_slice_log2 = (u32)value;
	} else if (k == "bin_wide_min_run") {
		t.bin_wide_min_run = (u32)value;
	} else if (k == "bin_ring") {
		t.bin_ring = (u32)value;
	} else if (k == "bin_fallback") {
		t.bin_fallback = value != 0;
	} else if (k == "bin_ovf_cap") {
		t.bin_ovf_cap = value;
	} else {
		return fail(c, NTEDIT_E_ARG, "set_tuning: unknown key '%s'", key);
	}
	return 0;
}

int
ntedit_hip_gather_bench(ntedit_hip_ctx* c, uint64_t nbytes, uint64_t n_probes, double* probes_per_s, float* ms)
{
	if (!c || nbytes < 4096 || (nbytes & (nbytes - 1))) {
		return fail(c, NTEDIT_E_ARG, "gather_bench: nbytes must be a power of two");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	u8* buf = nullptr;
	u32* sink = nullptr;
	HIP_TRY(c, hipMalloc((void**)&buf, nbytes));
	HIP_TRY(c, hipMalloc((void**)&sink, 64));
	HIP_TRY(c, hipMemset(buf, 0x5A, nbytes));
	const u64 threads = (u64)c->cu_count * 2048 * 2;
	u64 per_thread = (n_probes + threads - 1) / threads;
	per_thread = (per_thread + 11) / 12 * 12;
	const u64 mask = nbytes * 8 - 1;
	// warm-up + timed run
	hipLaunchKernelGGL(k_gather, dim3((unsigned)(threads / 256)), dim3(256), 0, c->stream, buf, mask, (u64)12, sink);
	HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(k_gather, dim3((unsigned)(threads / 256)), dim3(256), 0, c->stream, buf, mask, per_thread, sink);
	HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	float t = 0.f;
	HIP_TRY(c, hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
	(void)hipFree(buf);
	(void)hipFree(sink);
	if (ms) {
		*ms = t;
	}
	if (probes_per_s) {
		*probes_per_s = (double)(per_thread * threads) / ((double)t * 1e-3);
	}
	c->last_ms = t;
	return 0;
}

} // extern "C"

