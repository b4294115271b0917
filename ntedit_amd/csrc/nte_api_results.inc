// nte_api_results.inc -- part of nte_api.hip: the C ABI of results (statistics, edit records, rendering through
// host/render.cpp; what the reports put into a result is read through nte_api_reports.inc), host helpers (page-locked
// memory, NUMA binding), tuning knobs and the gather micro-benchmark.
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
			if (!r->owner->rep.ap.edited.p) {
				r->owner->rep.ap.edited = r->edited;
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

const char*
ntedit_hip_result_last_error(void)
{
	return g_result_err.c_str();
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
	const char* const paths[3] = { wo->fa_path, wo->tsv_path, wo->vcf_path };
	FILE* out[3] = { nullptr, nullptr, nullptr }; // fa, tsv, vcf
	bool opened = true;
	for (int i = 0; i < 3; i++) {
		out[i] = paths[i] ? fopen(paths[i], wo->append ? "ab" : "wb") : nullptr;
		opened = opened && (!paths[i] || out[i]);
	}
	for (int i = 0; i < 3; i++) {
		if (out[i] && !opened) {
			fclose(out[i]);
		} else if (out[i]) {
			setvbuf(out[i], nullptr, _IOFBF, i == 0 ? 4 << 20 : 1 << 20);
		}
	}
	if (!opened) {
		return NTEDIT_E_IO;
	}
	FILE *fa = out[0], *tsv = out[1], *vcf = out[2];
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
	for (FILE* f : out) {
		if (f && fclose(f) != 0) {
			rc = rc ? rc : -5;
		}
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

