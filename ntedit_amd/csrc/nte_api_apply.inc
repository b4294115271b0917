// nte_api_apply.inc -- part of nte_api.hip: the apply stage of ntedit_hip_polish_batch, behind the polish of a batch
// (PolishRun::apply() in nte_api_polish.inc hands it an ApplyInput when a report is on).  The reports' own state, sizes,
// helpers and entry points are in nte_api_reports.inc; this file queues them.
// ApplyStage::run()   the device applier (nte_apply.hip), then both sides of the draft -- the batch, the edited bases --
//                     through the reports: assess() per side, the spectrum and the draft store per side, the BGZF writer
// ApplyStage::assess() one side through the reports that read a bitmap: plain screening, QV count, marks, intervals
// apply_stage()       owns the edited bases while the stage runs: the one place a failure is cleaned up
namespace {

// one side of the draft in HBM: the batch as it came (which = 0) or its edited bases (1), and the entries of either
struct DraftSide
{
	int which;
	const u8* bases;
	u64 n;
	const u64* offs;
	const u32* lens;
	u32 n_entries;
};

struct ApplyStage
{
	const ApplyInput& in;
	ntedit_hip_ctx* const c;
	ntedit_hip_result* const r;
	ApplyReport& ap;
	const hipStream_t s;
	const u32 flags, k;
	// (APPLY_SHARED runs everything APPLY_QV runs and marks the present k-mers of both screenings: k_mark; APPLY_TRACK runs it
	// too and extracts the intervals of both bitmaps: nte_track.hip)
	const bool qv, shared, track, spectrum, cn;
	DraftSide side[2];                   // the batch, the edited bases (run() sets both before it assesses either)
	bool screened[2] = { false, false }; // the stage screened that side itself

	explicit ApplyStage(const ApplyInput& in_)
	  : in(in_)
	  , c(in_.c)
	  , r(in_.r)
	  , ap(in_.c->rep.ap)
	  , s(in_.c->stream)
	  , flags(in_.c->apply_flags)
	  , k(in_.c->dp.k)
	  , qv((flags & (NTEDIT_HIP_APPLY_QV | NTEDIT_HIP_APPLY_SHARED | NTEDIT_HIP_APPLY_TRACK)) != 0)
	  , shared((flags & NTEDIT_HIP_APPLY_SHARED) != 0)
	  , track((flags & NTEDIT_HIP_APPLY_TRACK) != 0)
	  , spectrum(in_.c->rep.sp.on)
	  , cn(in_.c->cn.state != CN_OFF)
	{}

	int run(DevBuf& eb);
	int assess(int which, const u64* plain_bitmap);
	int bgzf(const u8* d_edited);
};

// One side through the reports that read a bitmap, in one order for both sides: the plain screening into ap.bitmap where
// the side has no plain bitmap yet, the QV count, the completeness marks, the intervals -- each under its flag, inside the
// caller's PlainScreen.  Everything that reads the side's bitmap is queued when this returns (track_run waits for it).
int
ApplyStage::assess(int which, const u64* plain_bitmap)
{
	int rc;
	const DraftSide& sd = side[which];
	const u64 n_words = (sd.n + 63) / 64;
	const u64* bitmap = plain_bitmap;
	if (!bitmap) {
		const EventPair& ev = ap.screen[sd.which];
		if ((rc = screen_whole(c, sd.bases, sd.n, in.f0, (u64*)ap.bitmap.p, n_words, ev.begin, ev.end))) {
			return rc;
		}
		screened[sd.which] = true;
		bitmap = (const u64*)ap.bitmap.p;
	}
	QvRow* rows = (QvRow*)ap.rows.p;
	HIP_TRY(c, hipEventRecord(ap.count[sd.which].begin, s));
	if (sd.which == 0) { // (the rows are laid out once, before the first count: both sides' lengths)
		launch_qv_rows(s, rows, side[0].lens, side[1].lens, sd.n_entries);
	}
	launch_qv_count(s, sd.bases, sd.n, sd.offs, sd.lens, sd.n_entries, bitmap, k, rows, sd.which);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(ap.count[sd.which].end, s));
	if (sd.which == 1) { // (both counts are in: the rows go to the result)
		r->qv.resize(sd.n_entries);
		HIP_TRY(c, hipMemcpyAsync(r->qv.data(), rows, (size_t)sd.n_entries * sizeof(QvRow), hipMemcpyDeviceToHost, s));
	}
	if (shared && (rc = launch_mark(c, s, sd.bases, sd.n, in.f0, bitmap, n_words, sd.which))) {
		return rc;
	}
	if (track && (rc = track_run(c, s, bitmap, sd.n, sd.offs, sd.lens, sd.n_entries, k, sd.which, &r->track[sd.which], &r->track_n[sd.which]))) {
		return rc;
	}
	return 0;
}

// The device applier and both sides through the reports.  eb: the edited bases, the caller's (apply_stage) from the moment
// they are taken out of the context to the moment the result or the context has them again.  Crosses PCIe: five words of
// totals, the entries' offsets and lengths, the QV rows, what the reports themselves copy.
int
ApplyStage::run(DevBuf& eb)
{
	int rc;
	if (qv && k > QV_MAX_K) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "apply: the QV counts take k up to %u", QV_MAX_K);
	}
	if (track) {
		c->rep.tr.last = ntedit_hip_track_stats{ { 0.f, 0.f }, { 0, 0 }, { 0, 0 } };
	}
	if (shared && (rc = shared_begin(c, "polish_batch"))) { // (the completeness marks: begun here if that was not done)
		return rc;
	}
	const u64 n_ev = in.n_events;
	const u32 n_contigs = in.n_contigs;
	const size_t nc = n_contigs;
	if ((rc = ensure_events(c, ap.window)) || (rc = ensure_events(c, ap.screen)) || (rc = ensure_events(c, ap.count)) || (rc = ap.size_plan(c, n_ev, nc))) {
		return rc;
	}
	ApplyArgs a;
	memset(&a, 0, sizeof a);
	a.seq = in.d_seq;
	a.n_seq = in.n;
	a.offs = (const u64*)c->offs.p;
	a.lens = (const u32*)c->lens.p;
	a.n_contigs = n_contigs;
	a.arena = (const Item*)c->arena.p;
	a.arena_items = r->arena_items;
	a.ev_first = (const u32*)c->first_chunk.p;
	a.n_events = (u32)n_ev;
	a.ev = (ApplyEvent*)ap.ev.p;
	a.place = (ApplyPlace*)ap.place.p;
	a.ev_begin = (u32*)ap.range.p;
	a.ev_end = a.ev_begin + nc;
	a.contig = (ApplyContig*)ap.contig.p;
	a.out_offs = (u64*)ap.tabs.p;
	a.piece_base = a.out_offs + nc;
	a.totals = a.piece_base + nc + 1;
	a.status = (u32*)(a.totals + 3);
	a.out_lens = (u32*)(a.totals + 4);
	HIP_TRY(c, hipMemsetAsync(a.place, 0, (size_t)(n_ev + 1) * sizeof(ApplyPlace), s));
	HIP_TRY(c, hipMemsetAsync(a.ev_begin, 0xFF, nc * 4, s));
	HIP_TRY(c, hipMemsetAsync(a.ev_end, 0, nc * 4, s));
	HIP_TRY(c, hipMemsetAsync(a.totals, 0, 32, s));
	HIP_TRY(c, hipEventRecord(ap.window[0].begin, s));
	launch_apply_plan(s, a);
	HIP_TRY(c, hipGetLastError());
	u64 h_tot[4] = { 0, 0, 0, 0 };
	HIP_TRY(c, hipMemcpyAsync(h_tot, a.totals, 32, hipMemcpyDeviceToHost, s));
	HIP_TRY(c, hipStreamSynchronize(s));
	const u32 st = (u32)h_tot[3];
	if (st) {
		const int code = (st & AP_BAD_INDEX) ? -1 : (st & AP_BAD_ORDER) ? -2 : (st & AP_BAD_COUNT) ? -3 : (st & AP_BAD_ITEM) ? -4 : (st & AP_UNFINISHED) ? -6 : 0;
		if (!code) {
			return fail(c, NTEDIT_E_OVERFLOW, "apply: an edited contig of 4 GiB or more");
		}
		return fail(c, NTEDIT_E_INTERNAL, "apply: malformed event records (the renderer's code %d)", code);
	}
	const u64 total_bytes = h_tot[0], total_pieces = h_tot[1];
	{
		std::lock_guard<std::mutex> lk(c->pin_mu); // (a result that is freed hands its buffer back from another thread)
		eb = ap.edited;
		ap.edited = DevBuf();
	}
	if ((rc = ap.size_write(c, eb, total_bytes, total_pieces))) {
		return rc;
	}
	a.pieces = (ApplyPiece*)ap.pieces.p;
	a.out = (u8*)eb.p;
	launch_apply_write(s, a, total_bytes, total_pieces);
	HIP_TRY(c, hipGetLastError());
	HIP_TRY(c, hipEventRecord(ap.window[0].end, s));
	r->e_offs.resize(nc);
	r->e_lens.resize(nc);
	HIP_TRY(c, hipMemcpyAsync(r->e_offs.data(), a.out_offs, nc * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(c, hipMemcpyAsync(r->e_lens.data(), a.out_lens, nc * 4, hipMemcpyDeviceToHost, s));
	side[0] = DraftSide{ 0, in.d_seq, in.n, a.offs, a.lens, n_contigs };
	side[1] = DraftSide{ 1, a.out, total_bytes, a.out_offs, a.out_lens, n_contigs };
	if (qv) {
		// before: the batch and step 1's bitmap; after: the edited bases, screened the way a batch of that size is.  With
		// -s 1 step 1 marks every k-mer of accepted bases (k_screen: "no probe decides that"), so c->bitmap is not the plain
		// answer: both screenings then run with the flag down, the batch's into ap.bitmap first.  The screening of the
		// edited bases overwrites that bitmap: assess() has queued everything that reads the batch's by then.
		PlainScreen plain(c);
		const bool rescreen = plain.dp_snv != 0;
		if ((rc = ap.size_assess(c, rescreen && in.n > total_bytes ? in.n : total_bytes, nc))) { // (the larger side, before either is assessed)
			return rc;
		}
		if (!rescreen && (rc = bin_reset(c, s))) { // (the record chunks of step 1's screening; each screening here forgets the last one's)
			return rc;
		}
		if ((rc = assess(0, rescreen ? nullptr : in.d_bitmap)) || (rc = assess(1, nullptr))) {
			return rc;
		}
	}
	// The k-mer spectrum (ntedit_hip_set_spectrum; k_spectrum): the counters under the batch's k-mers and under those of the
	// edited bases, behind the applier and whatever the QV counts queued.  No bitmap is read: -s 1 changes nothing here.
	std::vector<uint64_t> sp_host;
	if (spectrum) {
		sp_host.resize(2 * (size_t)SPECTRUM_BINS + 2 * nc * 3);
		if ((rc = spectrum_begin(c, s, n_contigs))) {
			return rc;
		}
		for (const DraftSide& sd : side) {
			if ((rc = launch_spectrum(c, s, sd.bases, sd.n, in.f0, sd.offs, sd.lens, sd.n_entries, sd.which, true))) {
				return rc;
			}
		}
		HIP_TRY(c, hipMemcpyAsync(sp_host.data(), c->rep.sp.buf.p, sp_host.size() * 8, hipMemcpyDeviceToHost, s));
	}
	// The spectrum by copy number (ntedit_hip_set_cn; nte_cn.hip): both sides go into the draft store, device to device;
	// nothing is counted before ntedit_hip_cn_finish.  A store that passes its cap releases itself and fails nothing.
	if (cn) {
		std::string why;
		for (const DraftSide& sd : side) {
			if ((rc = cn_append(c->cn, sd.which, s, sd.bases, sd.n, sd.offs, sd.lens, sd.n_entries, &why))) {
				return fail(c, rc, "apply: %s", why.c_str());
			}
		}
	}
	HIP_TRY(c, hipStreamSynchronize(s));
	HIP_TRY(c, hipGetLastError());
	if (spectrum) {
		r->sp_bins.assign(sp_host.begin(), sp_host.begin() + 2 * SPECTRUM_BINS);
		r->depth.resize(nc);
		const uint64_t* rows0 = sp_host.data() + 2 * SPECTRUM_BINS;
		const uint64_t* rows1 = rows0 + nc * 3;
		for (size_t i = 0; i < nc; i++) {
			r->depth[i] = { rows0[3 * i], rows0[3 * i + 1], rows0[3 * i + 2], rows1[3 * i], rows1[3 * i + 1], rows1[3 * i + 2] };
		}
		spectrum_timed(c, 0, r->sp_bins.data());
		spectrum_timed(c, 1, r->sp_bins.data() + SPECTRUM_BINS);
		r->spectrum = true;
	}
	// ntedit_hip_apply_info: the applier's window, the screenings the stage ran, the two count windows
	ntedit_hip_apply_stats as = { elapsed_ms(ap.window[0]), 0.f, 0.f, total_pieces, total_bytes, h_tot[2] };
	for (int which = 0; which < 2; which++) {
		as.ms_screen += screened[which] ? elapsed_ms(ap.screen[which]) : 0.f;
		as.ms_count += qv ? elapsed_ms(ap.count[which]) : 0.f;
	}
	if (shared) {
		mark_timed(c, 0);
		mark_timed(c, 1);
	}
	ap.last = as;
	r->edited_bytes = total_bytes;
	if ((flags & NTEDIT_HIP_APPLY_BGZF) && (rc = bgzf(a.out))) {
		return rc;
	}
	if (flags & NTEDIT_HIP_APPLY_EDITED) {
		r->edited = eb; // the result's own until ntedit_hip_result_free()
	} else {
		std::lock_guard<std::mutex> lk(c->pin_mu);
		if (ap.edited.p) {
			release(eb);
		} else {
			ap.edited = eb;
		}
	}
	return 0;
}

// The BGZF writer (nte_bgzf_deflate.hip) behind the applier, on its stream: the batch's _edited.fa text laid out in HBM from
// the edited bases and the header lines, compressed block by block, the members packed and copied into page-locked memory
// of the result's.  Crosses PCIe: the image's tables and the names down, two words of totals and the members up.
int
ApplyStage::bgzf(const u8* d_edited)
{
	const u32 n_contigs = in.n_contigs;
	std::vector<u64> name_offs(n_contigs + 1, 0);
	std::string blob;
	for (u32 i = 0; i < n_contigs; i++) {
		blob += (*in.fa_names)[i];
		name_offs[i + 1] = blob.size();
	}
	const FaImage im = { d_edited, r->e_offs.data(), r->e_lens.data(), n_contigs, blob.data(), name_offs.data() };
	const u8* d_image = nullptr;
	u64 n_image = 0;
	BgzfTotals t;
	std::string why;
	int rc = bgzf_image(c, c->device, c->stream, im, &d_image, &n_image, &t.ms_image, &why);
	if (!rc) {
		rc = bgzf_encode(c, c->device, c->stream, d_image, n_image, &t, &why);
	}
	if (!rc && (rc = bgzf_pin_take(c, (size_t)t.bytes + 16, &r->bgzf_buf))) {
		return rc;
	}
	if (!rc) {
		rc = bgzf_fetch(c, c->stream, r->bgzf_buf.p, t.bytes, &t.ms_copy, &why);
	}
	if (rc) {
		bgzf_pin_give(c, r->bgzf_buf);
		return fail(c, rc, "apply: %s", why.c_str());
	}
	r->bgzf_bytes = t.bytes;
	r->bgzf_plain = t.plain;
	r->bgzf_members = t.members;
	c->rep.bz.last = { t.ms_image, t.ms_deflate, t.ms_copy, t.plain, t.bytes, t.members, t.stored };
	return 0;
}

// The stage for one polished batch.  The edited bases are this function's from start to end: on any failure whatever is
// queued is waited for, they are released and the result keeps no QV rows; the first error is the one reported.
int
apply_stage(const ApplyInput& in)
{
	ApplyStage stage(in);
	DevBuf eb;
	const int rc = stage.run(eb);
	if (rc) {
		const hipError_t he = hipDeviceSynchronize();
		if (he != hipSuccess) {
			in.c->err += std::string(" (then: ") + hipGetErrorString(he) + ")";
		}
		release(eb);
		in.r->qv.clear();
	}
	return rc;
}

} // namespace
