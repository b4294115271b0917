// nte_api_filters.inc -- part of nte_api.hip: the C ABI of contexts, parameters, Bloom filters and the screening-only call.
extern "C" {

void
ntedit_hip_params_default(ntedit_hip_params* p)
{
	nte_host::params_default(p);
}

void
ntedit_hip_params_clamp(ntedit_hip_params* p, char* warn, size_t cap)
{
	nte_host::params_clamp(p, warn, cap);
}

int
ntedit_hip_create(int device, ntedit_hip_ctx** out)
{
	if (!out) {
		return NTEDIT_E_ARG;
	}
	*out = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
		return NTEDIT_E_DEVICE;
	}
	if (device < 0 || device >= count) {
		return NTEDIT_E_ARG;
	}
	if (hipSetDevice(device) != hipSuccess) {
		return NTEDIT_E_DEVICE;
	}
	ntedit_hip_ctx* c = new ntedit_hip_ctx();
	c->device = device;
	nte_host::params_default(&c->hp);
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
		c->cu_count = (u32)prop.multiProcessorCount;
		int lds = 0;
		if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && lds > 0) {
			c->lds_per_block = (size_t)lds;
		}
	}
	if (hipStreamCreate(&c->stream) != hipSuccess || hipStreamCreate(&c->stream2) != hipSuccess) {
		delete c;
		return NTEDIT_E_DEVICE;
	}
	if (ensure_events(c, c->ev) || ensure_events(c, c->ev_assess) || ensure_events(c, c->ev_settle)) {
		delete c;
		return NTEDIT_E_DEVICE;
	}
	{
		std::lock_guard<std::mutex> lk(g_live_mu);
		g_live_ctx.push_back(c);
	}
	*out = c;
	return 0;
}

void
ntedit_hip_destroy(ntedit_hip_ctx* c)
{
	if (!c) {
		return;
	}
	{
		std::lock_guard<std::mutex> lk(g_live_mu);
		for (size_t i = 0; i < g_live_ctx.size(); i++) {
			if (g_live_ctx[i] == c) {
				g_live_ctx.erase(g_live_ctx.begin() + (long)i);
				break;
			}
		}
	}
	(void)hipSetDevice(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (auto& f : c->filt) {
		if (f.owned && f.data) {
			(void)hipFree(f.data);
		}
	}
	DevBuf* bufs[] = { &c->seq,      &c->bitmap,   &c->block_counts, &c->block_offsets, &c->events,
		               &c->first_chunk, &c->arena, &c->counters, &c->deferred,     &c->ws_nodes,      &c->ws_ov_pos,
		               &c->ws_ov_chr, &c->ws_prev, &c->ws_lps, &c->ws_win, &c->runmap, &c->candmap, &c->packed, &c->bin_records, &c->bin_fill, &c->bin_ctl, &c->bin_ovf, &c->bin_state, &c->ev_cover, &c->ev_before, &c->ev_flags, &c->ev_list, &c->ev_bmax, &c->ev_rest,       &c->offs,          &c->lens };
	for (DevBuf* b : bufs) {
		release(*b);
	}
	for (auto& pb : c->pin_pool) {
		(void)hipHostFree(pb.p);
	}
	c->pin_pool.clear();
	c->rep.release(); // (every report's buffers and events)
	bgzf_release(c); // (the BGZF writer's buffers: nte_bgzf_deflate.hip)
	cn_free(c->cn);
	if (c->d_tab) {
		(void)hipFree(c->d_tab);
	}
	destroy_events(c->ev);
	destroy_events(c->ev_assess);
	destroy_events(c->ev_settle);
	for (auto* evs : { &c->chunk_ev, &c->h2d_ev, &c->bin_ev }) {
		for (auto& e : *evs) {
			(void)hipEventDestroy(e);
		}
	}
	if (c->stream_copy) {
		(void)hipStreamSynchronize(c->stream_copy);
		(void)hipStreamDestroy(c->stream_copy);
	}

	if (c->stream2) {
		(void)hipStreamSynchronize(c->stream2);
		(void)hipStreamDestroy(c->stream2);
	}
	if (c->stream) {
		(void)hipStreamDestroy(c->stream);
	}
	delete c;
}

const char*
ntedit_hip_last_error(const ntedit_hip_ctx* c)
{
	return c ? c->err.c_str() : "no context";
}

static int
drop_filter(ntedit_hip_ctx* c, int slot)
{
	DevFilter& f = c->filt[slot];
	if (f.owned && f.data) {
		HIP_TRY(c, hipFree(f.data));
	}
	f = DevFilter();
	c->dp_valid = false;
	if (slot == 0) {
		c->rep.sh.release_marks(); // (the completeness marks were this filter's)
		cn_reset(c->cn);   // (and the draft store's copy numbers belong to one round: every round of a cascade starts clean)
	}
	return 0;
}

int
ntedit_hip_set_filter(
    ntedit_hip_ctx* c,
    int slot,
    const uint8_t* bits,
    uint64_t nbytes,
    uint32_t hash_num,
    uint32_t k,
    int counting)
{
	if (!c || slot < 0 || slot > 1 || !bits || nbytes == 0) {
		return fail(c, NTEDIT_E_ARG, "set_filter: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = drop_filter(c, slot);
	if (rc) {
		return rc;
	}
	DevFilter& f = c->filt[slot];
	// the slot arithmetic uses exactly nbytes (btllib takes the header's size as it is); only the
	// allocation is padded to whole 64-bit words (zero-filled: k_popcount reads words)
	const u64 padded = (nbytes + 7) / 8 * 8;
	HIP_TRY(c, hipMalloc((void**)&f.data, padded));
	f.owned = true;
	if (padded != nbytes) {
		HIP_TRY(c, hipMemset(f.data + (padded - 8), 0, 8));
	}
	HIP_TRY(c, hipMemcpy(f.data, bits, nbytes, hipMemcpyHostToDevice));
	f.nbytes = nbytes;
	f.hash_num = hash_num;
	f.k = k;
	f.counting = counting != 0;
	f.set = true;
	return 0;
}

int
ntedit_hip_set_filter_device(
    ntedit_hip_ctx* c,
    int slot,
    void* device_bits,
    uint64_t nbytes,
    uint32_t hash_num,
    uint32_t k,
    int counting)
{
	// (the caller's allocation must reach the next multiple of 8 bytes, zero-filled behind nbytes)
	if (!c || slot < 0 || slot > 1 || !device_bits || nbytes == 0 || ((uintptr_t)device_bits & 7)) {
		return fail(c, NTEDIT_E_ARG, "set_filter_device: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = drop_filter(c, slot);
	if (rc) {
		return rc;
	}
	DevFilter& f = c->filt[slot];
	f.data = (u8*)device_bits;
	f.owned = false;
	f.nbytes = nbytes;
	f.hash_num = hash_num;
	f.k = k;
	f.counting = counting != 0;
	f.set = true;
	return 0;
}

int
ntedit_hip_load_filter_file(ntedit_hip_ctx* c, int slot, const char* path)
{
	if (!c || slot < 0 || slot > 1 || !path) {
		return fail(c, NTEDIT_E_ARG, "load_filter_file: bad argument");
	}
	nte_host::BfHeader h;
	const char* why = nullptr;
	FILE* f = nte_host::bf_open(path, &h, &why);
	if (!f) {
		return fail(c, NTEDIT_E_IO, "`%s': %s", path, why ? why : "not a readable btllib Bloom filter file");
	}
	if (h.k < 12 || h.k > 200 || h.hash_num > MAX_HASHES) {
		fclose(f);
		return fail(c, NTEDIT_E_ARG, "`%s': k = %u, hash_num = %u: this build supports k in [12, 200] and at most %u hash functions",
		            path, h.k, h.hash_num, MAX_HASHES);
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = drop_filter(c, slot);
	if (rc) {
		fclose(f);
		return rc;
	}
	DevFilter& d = c->filt[slot];
	const u64 nbytes = (h.bytes + 7) / 8 * 8;
	if (hipMalloc((void**)&d.data, nbytes) != hipSuccess) {
		fclose(f);
		return fail(c, NTEDIT_E_DEVICE, "hipMalloc(%llu) failed", (unsigned long long)nbytes);
	}
	d.owned = true;
	(void)hipMemset(d.data, 0, nbytes);
	// stream the array through a pinned bounce buffer
	const size_t CH = 64u << 20;
	void* bounce = nullptr;
	if (hipHostMalloc(&bounce, CH, hipHostMallocDefault) != hipSuccess) {
		fclose(f);
		(void)drop_filter(c, slot);
		return fail(c, NTEDIT_E_DEVICE, "hipHostMalloc failed");
	}
	u64 done = 0;
	bool ok = true;
	while (done < h.bytes) {
		size_t want = (size_t)((h.bytes - done) < CH ? (h.bytes - done) : CH);
		size_t got = fread(bounce, 1, want, f);
		if (got != want) {
			ok = false;
			break;
		}
		if (hipMemcpy(d.data + done, bounce, got, hipMemcpyHostToDevice) != hipSuccess) {
			ok = false;
			break;
		}
		done += got;
	}
	(void)hipHostFree(bounce);
	fclose(f);
	if (!ok) {
		drop_filter(c, slot);
		return fail(c, NTEDIT_E_IO, "`%s': truncated Bloom filter file", path);
	}
	d.nbytes = h.bytes; // the size in the header IS the modulus (the allocation is padded to 64-bit words)
	d.hash_num = h.hash_num;
	d.k = h.k;
	d.counting = h.counting;
	d.set = true;
	return 0;
}

int
ntedit_hip_filter_info(
    const ntedit_hip_ctx* c,
    int slot,
    uint32_t* k,
    uint32_t* hash_num,
    uint64_t* nbytes,
    int* counting)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set) {
		return NTEDIT_E_NOFILTER;
	}
	const DevFilter& f = c->filt[slot];
	if (k) {
		*k = f.k;
	}
	if (hash_num) {
		*hash_num = f.hash_num;
	}
	if (nbytes) {
		*nbytes = f.nbytes;
	}
	if (counting) {
		*counting = f.counting;
	}
	return 0;
}

void*
ntedit_hip_filter_device_ptr(const ntedit_hip_ctx* c, int slot)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set) {
		return nullptr;
	}
	return c->filt[slot].data;
}

int
ntedit_hip_filter_alloc(ntedit_hip_ctx* c, int slot, uint64_t nbytes, uint32_t hash_num, uint32_t k)
{
	if (!c || slot < 0 || slot > 1 || nbytes == 0 || hash_num == 0 || hash_num > MAX_HASHES) {
		return fail(c, NTEDIT_E_ARG, "filter_alloc: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = drop_filter(c, slot);
	if (rc) {
		return rc;
	}
	nbytes = (nbytes + 7) / 8 * 8;
	DevFilter& f = c->filt[slot];
	HIP_TRY(c, hipMalloc((void**)&f.data, nbytes));
	f.owned = true;
	HIP_TRY(c, hipMemset(f.data, 0, nbytes));
	f.nbytes = nbytes;
	f.hash_num = hash_num;
	f.k = k;
	f.counting = false;
	f.set = true;
	return 0;
}

int
ntedit_hip_filter_insert(ntedit_hip_ctx* c, int slot, const char* bases, uint64_t n, int on_device)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set || !bases) {
		return fail(c, NTEDIT_E_ARG, "filter_insert: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	const DevFilter& df = c->filt[slot];
	if (df.counting) {
		return fail(c, NTEDIT_E_UNSUPPORTED, "filter_insert: counting filters are built on the host (ntStat)");
	}
	// insertion only needs k, the multipliers and the seed tables
	ntedit_hip_params hp;
	nte_host::params_default(&hp);
	DevParams saved = c->dp;
	bool saved_valid = c->dp_valid;
	int rc = nte_host::make_dev_params(hp, df.k, df.hash_num, false, &c->dp);
	if (rc) {
		c->dp = saved;
		return fail(c, rc, "filter_insert: unsupported k/hash_num");
	}
	if (!c->d_tab) {
		HIP_TRY(c, hipMalloc((void**)&c->d_tab, TAB_WORDS * sizeof(u64)));
	}
	if (c->tab_k != df.k) {
		u64 tab[TAB_WORDS];
		build_seed_tables(df.k, tab);
		HIP_TRY(c, hipMemcpy(c->d_tab, tab, sizeof tab, hipMemcpyHostToDevice));
		c->tab_k = df.k;
	}
	if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
		return fail(c, NTEDIT_E_ARG, "filter_insert: bases must be host or device bytes");
	}
	const u8* d_seq = nullptr;
	rc = stage_bases(c, bases, n, on_device, &d_seq);
	if (rc == 0) {
		HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
		rc = launch_screen<true>(c, d_seq, n, dev_filter(df), nullptr, 0);
		HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
		HIP_TRY(c, hipStreamSynchronize(c->stream));
		HIP_TRY(c, hipEventElapsedTime(&c->last_ms, c->ev[0], c->ev[1]));
	}
	c->dp = saved;
	c->dp_valid = saved_valid;
	return rc;
}

int
ntedit_hip_filter_occupancy(ntedit_hip_ctx* c, int slot, uint64_t* occupied, uint64_t* slots)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set || !occupied) {
		return fail(c, NTEDIT_E_ARG, "filter_occupancy: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	const DevFilter& f = c->filt[slot];
	int rc = ensure(c, c->counters, 256);
	if (rc) {
		return rc;
	}
	unsigned long long* d_total = (unsigned long long*)c->counters.p;
	HIP_TRY(c, hipMemsetAsync(d_total, 0, 8, c->stream));
	const u64 n_words = (f.nbytes + 7) / 8; // (allocations are whole 64-bit words, zero behind nbytes)
	hipLaunchKernelGGL(k_popcount, dim3((unsigned)(c->cu_count * 8)), dim3(256), 0, c->stream, (const u64*)f.data, n_words,
	                   f.counting ? 1 : 0, d_total);
	HIP_TRY(c, hipGetLastError());
	unsigned long long h = 0;
	HIP_TRY(c, hipMemcpyAsync(&h, d_total, 8, hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	*occupied = h;
	if (slots) {
		*slots = f.counting ? f.nbytes : f.nbytes * 8;
	}
	return 0;
}

int
ntedit_hip_filter_download(const ntedit_hip_ctx* c, int slot, uint8_t* bits)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set || !bits) {
		return NTEDIT_E_ARG;
	}
	if (hipSetDevice(c->device) != hipSuccess) {
		return NTEDIT_E_DEVICE;
	}
	const DevFilter& f = c->filt[slot];
	return hipMemcpy(bits, f.data, f.nbytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : NTEDIT_E_DEVICE;
}

int
ntedit_hip_filter_save_file(const ntedit_hip_ctx* c, int slot, const char* path)
{
	if (!c || slot < 0 || slot > 1 || !c->filt[slot].set || !path) {
		return NTEDIT_E_ARG;
	}
	const DevFilter& f = c->filt[slot];
	std::vector<u8> host(f.nbytes);
	int rc = ntedit_hip_filter_download(c, slot, host.data());
	if (rc) {
		return rc;
	}
	nte_host::BfHeader h;
	h.bytes = f.nbytes;
	h.hash_num = f.hash_num;
	h.k = f.k;
	h.counting = f.counting;
	return nte_host::bf_save(path, h, host.data()) ? NTEDIT_E_IO : 0;
}

int
ntedit_hip_set_params(ntedit_hip_ctx* c, const ntedit_hip_params* p)
{
	if (!c || !p) {
		return NTEDIT_E_ARG;
	}
	c->hp = *p;
	c->dp_valid = false;
	return 0;
}

int
ntedit_hip_screen(ntedit_hip_ctx* c, const char* bases, uint64_t n, int on_device, uint64_t* bitmap)
{
	if (!c || !bases || !bitmap) {
		return fail(c, NTEDIT_E_ARG, "screen: bad argument");
	}
	HIP_TRY(c, hipSetDevice(c->device));
	int rc = refresh_params(c);
	if (rc) {
		return rc;
	}
	if (on_device != NTEDIT_HIP_BASES_HOST && on_device != NTEDIT_HIP_BASES_DEVICE) {
		return fail(c, NTEDIT_E_ARG, "screen: bases must be host or device bytes");
	}
	const u64 n_words = (n + 63) / 64;
	const u8* d_seq = nullptr;
	rc = stage_bases(c, bases, n, on_device, &d_seq);
	if (rc) {
		return rc;
	}
	u64* d_bitmap = bitmap;
	if (!on_device) {
		rc = ensure(c, c->bitmap, (n_words + 1) * 8);
		if (rc) {
			return rc;
		}
		d_bitmap = (u64*)c->bitmap.p;
	}
	if ((rc = screen_whole(c, d_seq, n, dev_filter(c->filt[0]), d_bitmap, n_words, c->ev[0], c->ev[1]))) {
		return rc;
	}
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (!on_device) {
		HIP_TRY(c, hipMemcpy(bitmap, d_bitmap, n_words * 8, hipMemcpyDeviceToHost));
	}
	HIP_TRY(c, hipEventElapsedTime(&c->last_ms, c->ev[0], c->ev[1]));
	return 0;
}

} // extern "C"

