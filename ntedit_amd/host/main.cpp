// main.cpp -- `ntedit` host driver for the MI355X hot path.
//
// The command line is the reference's (cli_options.cpp).  A run parses it, opens the device, and polishes in one round, or
// with --reads -k K1,...,Kn in a cascade of n.  A round is a sequence of stages: the filter (cli_filter.cpp), the parameter
// echo, the device set-up, then the draft through three pipeline stages that share a pool of three batches
// (cli_batches.h) -- a reader with kseq semantics, the GPU through the C ABI (include/ntedit_hip.h), and a writer of
// <prefix>_edited.fa and <prefix>_changes.tsv byte-identical to the reference's, plus <prefix>_variants.vcf (the
// ##fileDate line carries today's date, as in the reference) -- and the summaries (cli_report.cpp).  With --bgzip the
// edited draft is <prefix>_edited.fa.gz: the GPU stage's results hold its BGZF members, the writer stage appends them.
// With --qv --bed the results hold the unsupported regions before and after as intervals, and the writer stage appends
// them to <prefix>_absent_before.bed and <prefix>_absent_after.bed.  With --spectrum they hold the k-mer spectrum before
// and after and a depth row per contig: the writer stage sums the bins and appends the rows to <prefix>_depth.tsv,
// <prefix>_spectrum.tsv is written at the round's end.  With --spectrum --cn the library keeps the batches and their edited
// entries in HBM; at the round's end they are counted once and <prefix>_spectrum_cn.tsv and <prefix>_cn_contigs.tsv written.
#include "../../include/ntedit_hip.h"
#include "cli_batches.h"
#include "cli_common.h"
#include "cli_filter.h"
#include "cli_options.h"
#include "cli_report.h"
#include "fasta.h"
#include "fasta_map.h"
#include "k_list.h"

#include <cerrno>
#include <cstring>
#include <fcntl.h>
#include <memory>
#include <sstream>
#include <thread>

using namespace nte_cli;

// the state of a run, across its rounds
struct Run
{
	ntedit_hip_ctx* ctx;
	BatchPool& pool;
	bool store_lost = false; // a cascade's store was released: no round tries it again
};

// what the three pipeline stages of a round share.  Each total has one writer: the reader stage `bases` and `s_read`, the
// GPU stage `s_call` and the --qv, --bed and --spectrum times, the writer stage the rest; they are read after the stages are joined.
struct Round
{
	const CliOptions& opt;
	ntedit_hip_ctx* ctx;
	uint32_t k = 0;
	std::string fa_path, tsv_path, vcf_path, qv_path, bed_path[2];
	FILE *qv_f = nullptr, *index_f = nullptr;
	FILE* bed_f[2] = { nullptr, nullptr }; // --bed: <prefix>_absent_before.bed, _absent_after.bed
	std::string spectrum_path[2];          // --spectrum: <prefix>_spectrum.tsv, <prefix>_depth.tsv
	FILE* depth_f = nullptr;
	std::vector<std::string> cn_names; // --cn: the entries in the order the GPU stage polished them (= the store's rows)
	int fa_fd = -1; // --bgzip: <prefix>_edited.fa.gz, open for the writer stage
	ntedit_hip_annot* annot = nullptr;
	Channel free_q, gpu_q, write_q;
	RoundTotals tot;
};

static std::string
base_name(const std::string& p)
{
	return p.substr(p.find_last_of("/\\") + 1);
}

// the host threads of a stage that scales up to `cap` of them: -t, or the machine's
static unsigned
threads_up_to(const CliOptions& opt, unsigned cap)
{
	const unsigned n = opt.threads_given ? opt.nthreads : std::thread::hardware_concurrency();
	return n > cap ? cap : n;
}

// the BLOOM:: line of the primary filter; what the filter's kind decides
static void
describe_filter(ntedit_hip_ctx* ctx, const CliOptions& opt, const std::string& bf, ntedit_hip_params* p, uint32_t* k, int* counting)
{
	uint32_t h = 0;
	uint64_t nbytes = 0;
	ntedit_hip_filter_info(ctx, NTEDIT_FILTER_PRIMARY, k, &h, &nbytes, counting);
	printf("BLOOM::\tcounting: %s\tsize: %llu\tnumber hash functions: %u\tkmer size: %u\n", *counting ? "YES" : "NO",
	       (unsigned long long)nbytes, h, *k);
	if (opt.completeness && *counting) {
		// (before any output file is opened and before a batch is polished)
		fail("--completeness: `%s' is a counting filter; completeness takes a plain filter", bf.c_str());
	}
	if (opt.spectrum && !*counting) {
		// (the same, the other way round)
		fail("--spectrum: `%s' is a plain filter; the spectrum takes a counting filter", bf.c_str());
	}
	if (!*counting && p->min_threshold != 1) {
		// ntedit.cpp:2453-2458
		fprintf(stderr, PROGRAM ": warning: Bloom filter is not counting, min k-mer presence threshold will be set to 1.\n");
		p->min_threshold = 1;
	}
}

// "verifying parameters": the clamps, the default prefix, the echo
static void
echo_parameters(const CliOptions& opt, ntedit_hip_params& p, uint32_t k, int counting, const std::string& draft, const FilterStage& fs,
                std::string& prefix)
{
	const std::string& bf = fs.bf;
	printf("\n---------- verifying parameters                     : %s", now_text());
	char warn[1024];
	ntedit_hip_params_clamp(&p, warn, sizeof warn);
	if (warn[0]) {
		fputs(warn, stderr);
	}
	if (prefix.empty()) {
		// ntedit.cpp:2496-2502
		std::ostringstream o;
		o << base_name(draft) << "_k" << k << "_z" << p.min_contig_len << "_r" << base_name(bf) << "_i"
		  << p.max_insertions << "_d" << p.max_deletions << "_m" << p.mode;
		prefix = o.str();
	}
	printf("\nrunning : " PROGRAM " (MI355X HIP hot path)\n -f %s\n -k %u\n -z %u\n -b %s\n -r %s\n -e %s\n -i %u\n -d %u",
	       base_name(draft).c_str(), k, p.min_contig_len, prefix.c_str(), base_name(bf).c_str(),
	       base_name(fs.bfrep).c_str(), p.max_insertions, p.max_deletions);
	if (p.use_ratio) {
		printf("\n -X %g\n -Y %g", p.missing_ratio, p.edit_ratio);
	} else {
		printf("\n -x %g\n -y %g", p.missing_threshold, p.edit_threshold);
	}
	printf("\n -j %u\n -m %d\n -s %d\n -l %s\n -a %d\n -t %u\n -v %d\n\n", p.jump, p.mode, p.snv, base_name(opt.vcf).c_str(),
	       p.mask, opt.nthreads, opt.verbose);
	if (counting) {
		printf(" -p %u\n -q %u\n\n", p.min_threshold, p.max_threshold); // ntedit.cpp:2519-2522
	}
}

// the secondary filter: loaded from the -e file, unless the reads stage built it
static void
secondary_filter(ntedit_hip_ctx* ctx, const std::string& bfrep, bool built_from_reads, uint32_t k)
{
	if (built_from_reads) {
		printf("---------- secondary Bloom filter built from reads   : %s\n", now_text());
	} else {
		printf("---------- loading secondary Bloom filter from file : %s\n", now_text());
		if (ntedit_hip_load_filter_file(ctx, NTEDIT_FILTER_SECONDARY, bfrep.c_str()) != 0) {
			fail("secondary Bloom filter file supplied (-e) is incorrect.");
		}
	}
	uint32_t k2 = 0;
	ntedit_hip_filter_info(ctx, NTEDIT_FILTER_SECONDARY, &k2, nullptr, nullptr, nullptr);
	if (k2 != k) {
		fail("secondary Bloom filter k size (%u) is different than main Bloom filter k size (%u)", k2, k);
	}
}

// The parameters into the context, and start-up, like the filter load: the context's buffers for the largest batch + one
// internal warm-up batch, so that the first polish_batch call costs what the later ones do (ntedit_hip_reserve)
static void
prepare_device(Run& run, const CliOptions& opt, const ntedit_hip_params& p, bool store_held, size_t round)
{
	ntedit_hip_ctx* ctx = run.ctx;
	if (ntedit_hip_set_params(ctx, &p) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	const uint32_t apply = (opt.qv ? NTEDIT_HIP_APPLY_QV | (opt.completeness ? NTEDIT_HIP_APPLY_SHARED : 0u) : 0u) | (opt.bgzip ? NTEDIT_HIP_APPLY_BGZF : 0u) |
	                       (opt.bed ? NTEDIT_HIP_APPLY_TRACK : 0u);
	if (apply && ntedit_hip_set_apply(ctx, apply) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	if (opt.spectrum && ntedit_hip_set_spectrum(ctx, 1) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	// --cn: the draft store begins empty in every round
	if (opt.cn && ntedit_hip_set_cn(ctx, 1, opt.cn_store) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	// --completeness: the two mark arrays of this round's filter, mapped here and not inside the first batch
	if (opt.completeness && ntedit_hip_shared_begin(ctx) != 0) {
		fail("%s", ntedit_hip_last_error(ctx));
	}
	auto reserve = [&]() {
		return ntedit_hip_reserve(ctx, run.pool.pin_bytes(), 1u << 16, 0, opt.no_pack ? NTEDIT_HIP_BASES_HOST : NTEDIT_HIP_BASES_PACKED);
	};
	int reserved = reserve();
	if (reserved != 0 && store_held) {
		// the store is held for the next round: when the polish buffers do not fit beside it, it goes, and the later
		// rounds read the files
		ntedit_hip_sketch_free(ctx);
		run.store_lost = true;
		printf("Resident store: released (the polish buffers of round %zu did not fit beside it); the later rounds read the files\n",
		       round + 1);
		reserved = reserve();
	}
	if (reserved != 0) {
		// (optional: the buffers then grow on demand, inside the first calls)
		fprintf(stderr, PROGRAM ": warning: buffers could not be sized ahead (%s); they grow on demand\n", ntedit_hip_last_error(ctx));
	}
	run.pool.join_pin_thread();
}

// the output files of a round, opened or begun; -l's annotated variants
static void
open_outputs(Round& r, const ntedit_hip_params& p, int counting, const std::string& draft)
{
	const CliOptions& opt = r.opt;
	FILE* f = fopen(r.fa_path.c_str(), "wb");
	if (!f) {
		fail("cannot write `%s'", r.fa_path.c_str());
	}
	fclose(f);
	if (opt.bgzip && (r.fa_fd = open(r.fa_path.c_str(), O_WRONLY | O_APPEND)) < 0) {
		fail("cannot write `%s'", r.fa_path.c_str());
	}
	if (ntedit_hip_write_tsv_header(r.tsv_path.c_str(), r.k, p.jump, counting) != 0) {
		fail("cannot write `%s'", r.tsv_path.c_str());
	}
	if (ntedit_hip_write_vcf_header(r.vcf_path.c_str(), draft.c_str()) != 0) { // ntedit.cpp:2192-2211
		fail("cannot write `%s'", r.vcf_path.c_str());
	}
	// --qv: <prefix>_qv.tsv, a row per written contig as the batches come back, "#total" at the end
	if (opt.qv) {
		r.qv_f = fopen(r.qv_path.c_str(), "wb");
		if (!r.qv_f) {
			fail("cannot write `%s'", r.qv_path.c_str());
		}
		fputs(ntedit_hip_qv_header(), r.qv_f);
	}
	// --bed: the two tracks, the rows of a batch as it comes back
	for (int which = 0; opt.bed && which < 2; which++) {
		r.bed_f[which] = fopen(r.bed_path[which].c_str(), "wb");
		if (!r.bed_f[which]) {
			fail("cannot write `%s'", r.bed_path[which].c_str());
		}
	}
	// --spectrum: the depth table, a row per written contig as the batches come back, "#total" at the end
	if (opt.spectrum) {
		r.depth_f = fopen(r.spectrum_path[1].c_str(), "wb");
		if (!r.depth_f) {
			fail("cannot write `%s'", r.spectrum_path[1].c_str());
		}
		fputs(ntedit_hip_depth_header(), r.depth_f);
	}
	if (!opt.vcf.empty()) {
		// -l: annotated variants (e.g. clinvar.vcf[.gz]), ntedit.cpp:2524-2562
		if (access(opt.vcf.c_str(), R_OK) == -1) { // ntedit.cpp:476-483
			fail("`%s': %s", opt.vcf.c_str(), strerror(errno));
		}
		if (ntedit_hip_annot_load(opt.vcf.c_str(), &r.annot) != 0) {
			fprintf(stderr, "Unable to open file\n");
		}
	}
}

// --shard: a first pass over the draft collects the lengths of the contigs >= -z, in draft order
static std::vector<uint64_t>
shard_lengths(nte_host::FastaMap& fmap, const std::string& draft, uint32_t min_contig_len)
{
	std::vector<uint64_t> lens;
	if (fmap.ok()) {
		fmap.measure(0, fmap.records());
		for (size_t i = 0; i < fmap.records(); i++) {
			if (fmap.length(i) >= min_contig_len) {
				lens.push_back(fmap.length(i));
			}
		}
		return lens;
	}
	nte_host::FastaReader scan(draft.c_str());
	if (!scan.ok()) {
		fail("`%s': cannot open", draft.c_str());
	}
	std::string h, sq;
	while (scan.next(h, sq)) {
		const void* z = memchr(sq.data(), 0, sq.size());
		const size_t len = z ? (size_t)((const char*)z - sq.data()) : sq.size();
		if (len >= min_contig_len) {
			lens.push_back(len);
		}
		sq.clear();
	}
	if (scan.io_error()) {
		// (a partition computed from half a draft would differ between the shards)
		fail("`%s': %s", draft.c_str(), scan.io_error_text().c_str());
	}
	return lens;
}

// The reader stage's end of the pipeline: the batch being filled, and the time spent filling it.
class BatchFeed
{
  public:
	explicit BatchFeed(Round& r)
	  : r_(r)
	  , w_(r.free_q.pop())
	{}
	Batch& batch() { return w_->b; }
	// the next free batch (the wait for it is not reading time)
	Work* wait_free()
	{
		r_.tot.s_read += clock_.s();
		Work* next = r_.free_q.pop();
		clock_.restart();
		return next;
	}
	// the open batch goes to the GPU stage; `next` is filled from here on
	void hand_over(Work* next)
	{
		Batch& b = w_->b;
		if (!r_.opt.no_pack && b.size()) {
			// (--pack.  Measured on the 3 Gbp draft: the GPU stage gains ~10 ms per 3 GB, packing costs the reader stage
			// 0.5 s on 4 threads -- 1 GB/s per thread, a table look-up per byte -- and puts it on the critical path:
			// 0.94 s end to end against 0.67 s.  Off by default; the packed form pays where the producer has
			// cycles to spare or emits it directly.)
			const uint64_t need = ntedit_hip_packed_size(b.size());
			if (b.packed.size() < need) {
				b.packed.resize(need + need / 8);
			}
			b.is_packed = ntedit_hip_pack_bases(b.data(), b.size(), b.packed.data(), r_.opt.nthreads) == 0;
		}
		r_.tot.s_read += clock_.s();
		r_.gpu_q.push(w_);
		w_ = next;
		clock_.restart();
	}
	// the (possibly empty) last batch, and the end of the stream
	void finish(const Admission& adm)
	{
		r_.tot.bases = adm.bases();
		hand_over(nullptr);
		r_.gpu_q.push(nullptr);
	}

  private:
	Round& r_;
	Work* w_;
	Stopwatch clock_;
};

static void
say_progress(const Admission& adm)
{
	if (adm.seen() % 1000000 == 0) {
		printf("Processed %llu\n", (unsigned long long)adm.seen());
	}
}

// Reader stage over a mapping of a plain multi-FASTA file (fasta_map.h): picks the records of a batch, then measures and
// copies them concurrently.
static void
read_mapped(Round& r, nte_host::FastaMap& fmap, Admission adm)
{
	BatchFeed feed(r);
	const size_t N = fmap.records(), GROUP = 1024;
	std::vector<size_t> pick;
	std::vector<char*> dst;
	auto copy_picked = [&]() {
		Batch& b = feed.batch();
		if (pick.empty()) {
			return;
		}
		const size_t total = b.offs.back() + b.lens.back() + 1;
		if (!b.reserve_raw(total)) {
			fail("out of memory for a batch of %zu bytes", total);
		}
		dst.resize(pick.size());
		for (size_t q = 0; q < pick.size(); q++) {
			dst[q] = b.raw + b.offs[q];
			b.raw[b.offs[q] + b.lens[q]] = '\n';
		}
		fmap.copy(pick.data(), dst.data(), pick.size());
		b.raw_n = total;
		pick.clear();
	};
	for (size_t i = 0, measured = 0; i < N; i++) {
		if (i >= measured) {
			const size_t cnt = N - measured < GROUP ? N - measured : GROUP;
			fmap.measure(measured, cnt);
			measured += cnt;
		}
		const uint64_t len = fmap.length(i);
		const Admission::Verdict v = adm.offer(len);
		if (v == Admission::TOO_LONG) {
			fail("contig longer than 2^32 bases");
		}
		if (v == Admission::CLOSE_THEN_TAKE) {
			copy_picked();
			feed.hand_over(feed.wait_free());
		}
		if (v != Admission::SKIP) {
			feed.batch().add(adm.offset(), (uint32_t)len, fmap.header(i), adm.ordinal());
			pick.push_back(i);
		}
		say_progress(adm);
	}
	copy_picked();
	feed.finish(adm);
}

// Reader stage over anything else (gzip, FASTQ, CR line ends, ...; --no-map): appends from the stream.
static void
read_streamed(Round& r, nte_host::FastaReader& reader, Admission adm)
{
	BatchFeed feed(r);
	std::string hdr;
	for (;;) {
		Batch& b = feed.batch();
		const size_t before = b.blob.size();
		if (!reader.next(hdr, b.blob)) {
			break;
		}
		// strings holding an embedded NUL end there in the reference (contigSeq = seq->seq.s)
		const void* z = memchr(b.blob.data() + before, 0, b.blob.size() - before);
		if (z) {
			b.blob.resize((size_t)((const char*)z - b.blob.data()));
		}
		const size_t len = b.blob.size() - before;
		const Admission::Verdict v = adm.offer(len);
		if (v == Admission::TOO_LONG) {
			fail("contig longer than 2^32 bases");
		}
		if (v == Admission::CLOSE_THEN_TAKE) {
			Work* next = feed.wait_free();
			next->b.blob.assign(b.blob, before, std::string::npos);
			b.blob.resize(before);
			feed.hand_over(next);
		}
		if (v == Admission::SKIP) {
			b.blob.resize(before);
		} else {
			feed.batch().add(adm.offset(), (uint32_t)len, hdr, adm.ordinal());
			feed.batch().blob.push_back('\n');
		}
		say_progress(adm);
	}
	feed.finish(adm);
}

// --bgzip: all of p[0 .. n) to the edited draft
static void
write_bgzf(Round& r, const uint8_t* p, uint64_t n)
{
	while (n) {
		const ssize_t w = write(r.fa_fd, p, n < (1u << 30) ? (size_t)n : (size_t)1 << 30);
		if (w < 0 && errno == EINTR) {
			continue;
		}
		if (w <= 0) {
			fail("cannot write `%s'", r.fa_path.c_str());
		}
		p += w;
		n -= (uint64_t)w;
	}
}

// --bed: the rows of one batch's intervals, before or after, under the names of its entries
static void
write_bed_rows(Round& r, const ntedit_hip_result* res, const std::vector<const char*>& names, int which)
{
	uint64_t n = 0;
	int rc = ntedit_hip_result_track(res, which, nullptr, 0, &n);
	std::vector<ntedit_hip_track_interval> ivs((size_t)n);
	if (rc == NTEDIT_E_OVERFLOW) {
		rc = ntedit_hip_result_track(res, which, ivs.data(), n, &n);
	}
	if (rc != 0) {
		fail("%s", ntedit_hip_result_last_error());
	}
	std::string line;
	bool ok = true;
	for (size_t i = 0; ok && i < ivs.size(); i++) {
		ok = ivs[i].entry < names.size();
		if (ok) {
			line.resize(strlen(names[ivs[i].entry]) + 64);
			ok = ntedit_hip_track_format_row(names[ivs[i].entry], &ivs[i], &line[0], line.size()) == 0 && fputs(line.c_str(), r.bed_f[which]) >= 0;
			r.tot.bed_bases[which] += ivs[i].end - ivs[i].begin;
		}
	}
	r.tot.bed_intervals[which] += ivs.size();
	if (!ok) {
		fail("cannot write `%s'", r.bed_path[which].c_str());
	}
}

// --spectrum: one batch's bins into the round's, its depth rows under the names of its entries
static void
write_spectrum_rows(Round& r, const ntedit_hip_result* res, const std::vector<const char*>& names)
{
	for (int which = 0; which < 2; which++) {
		uint64_t bins[256];
		if (ntedit_hip_result_spectrum(res, which, bins) != 0) {
			fail("%s", ntedit_hip_result_last_error());
		}
		for (int c = 0; c < 256; c++) {
			r.tot.spectrum[which][c] += bins[c];
		}
	}
	std::vector<ntedit_hip_depth_row> rows(names.size());
	std::string line;
	bool ok = ntedit_hip_result_depth(res, rows.data(), (uint32_t)rows.size()) == 0;
	for (size_t i = 0; ok && i < rows.size(); i++) {
		line.resize(strlen(names[i]) + 256);
		ok = ntedit_hip_depth_format_row(names[i], &rows[i], &line[0], line.size()) == 0 && fputs(line.c_str(), r.depth_f) >= 0;
		r.tot.depth.kmers_before += rows[i].kmers_before;
		r.tot.depth.sum_before += rows[i].sum_before;
		r.tot.depth.saturated_before += rows[i].saturated_before;
		r.tot.depth.kmers_after += rows[i].kmers_after;
		r.tot.depth.sum_after += rows[i].sum_after;
		r.tot.depth.saturated_after += rows[i].saturated_after;
	}
	if (!ok) {
		fail("cannot write `%s'", r.spectrum_path[1].c_str());
	}
}

// Writer stage: renders the batches the GPU stage hands over, in order, and sums their statistics.
static void
write_batches(Round& r)
{
	while (Work* w = r.write_q.pop()) {
		Batch& b = w->b;
		const Stopwatch clock;
		std::vector<const char*> names(b.names.size());
		for (size_t i = 0; i < b.names.size(); i++) {
			names[i] = b.names[i].c_str();
		}
		ntedit_hip_write_options wo;
		memset(&wo, 0, sizeof wo);
		wo.fa_path = r.opt.bgzip ? nullptr : r.fa_path.c_str(); // (--bgzip: the result holds the FASTA text, compressed)
		wo.tsv_path = r.tsv_path.c_str();
		wo.vcf_path = r.vcf_path.c_str();
		wo.append = 1;
		wo.annot = r.annot;
		std::vector<uint64_t> sizes;
		if (r.index_f) {
			sizes.assign(names.size() * 3 + 3, 0);
			wo.out_sizes = sizes.data();
		}
		if (ntedit_hip_write_outputs_ex(w->res, b.data(), b.offs.data(), b.lens.data(), names.data(), (uint32_t)names.size(), &wo) != 0) {
			fail("cannot write outputs");
		}
		if (r.opt.bgzip) {
			const uint8_t* members = nullptr;
			uint64_t n_bytes = 0;
			if (ntedit_hip_result_fa_bgzf(w->res, &members, &n_bytes, nullptr, nullptr) != 0) {
				fail("%s", ntedit_hip_result_last_error());
			}
			write_bgzf(r, members, n_bytes);
		}
		for (size_t i = 0; r.index_f && i < names.size(); i++) {
			fprintf(r.index_f, "%llu\t%llu\t%llu\t%llu\n", (unsigned long long)b.ordinals[i], (unsigned long long)sizes[3 * i],
			        (unsigned long long)sizes[3 * i + 1], (unsigned long long)sizes[3 * i + 2]);
		}
		if (r.qv_f) {
			std::vector<ntedit_hip_qv_row> rows(names.size());
			std::string line;
			bool ok = ntedit_hip_result_qv(w->res, rows.data(), (uint32_t)rows.size()) == 0;
			for (size_t i = 0; ok && i < rows.size(); i++) {
				line.resize(b.names[i].size() + 256);
				ok = ntedit_hip_qv_format_row(names[i], &rows[i], r.k, &line[0], line.size()) == 0 && fputs(line.c_str(), r.qv_f) >= 0;
				r.tot.add(rows[i]);
			}
			if (!ok) {
				fail("cannot write `%s'", r.qv_path.c_str());
			}
		}
		for (int which = 0; r.opt.bed && which < 2; which++) {
			write_bed_rows(r, w->res, names, which);
		}
		if (r.depth_f) {
			write_spectrum_rows(r, w->res, names);
		}
		ntedit_hip_stats st;
		ntedit_hip_result_stats(w->res, &st);
		r.tot.add(st);
		ntedit_hip_result_free(w->res);
		w->res = nullptr;
		b.clear();
		r.tot.s_write += clock.s();
		r.free_q.push(w);
	}
}

// GPU stage: polishes the batches the reader stage hands over, until the end of its stream
static void
polish_batches(Round& r)
{
	while (Work* w = r.gpu_q.pop()) {
		Batch& b = w->b;
		if (b.names.empty()) {
			b.clear();
			r.free_q.push(w);
			continue;
		}
		const Stopwatch clock;
		if (r.opt.bgzip) {
			std::vector<const char*> names(b.names.size());
			for (size_t i = 0; i < b.names.size(); i++) {
				names[i] = b.names[i].c_str();
			}
			if (ntedit_hip_set_fa_names(r.ctx, names.data(), (uint32_t)names.size()) != 0) {
				fail("%s", ntedit_hip_last_error(r.ctx));
			}
		}
		if (ntedit_hip_polish_batch(r.ctx, b.is_packed ? b.packed.data() : b.data(), b.size(), b.offs.data(), b.lens.data(),
		                            (uint32_t)b.names.size(), b.is_packed ? NTEDIT_HIP_BASES_PACKED : NTEDIT_HIP_BASES_HOST, &w->res) != 0) {
			fail("%s", ntedit_hip_last_error(r.ctx));
		}
		r.tot.s_call += clock.s();
		if (r.opt.cn) {
			r.cn_names.insert(r.cn_names.end(), b.names.begin(), b.names.end());
		}
		ntedit_hip_apply_stats as;
		if (r.opt.qv && ntedit_hip_apply_info(r.ctx, &as) == 0) {
			r.tot.ms_apply += as.ms_apply;
			r.tot.ms_qv_screen += as.ms_screen;
			r.tot.ms_qv_count += as.ms_count;
		}
		ntedit_hip_track_stats ts;
		if (r.opt.bed && ntedit_hip_track_info(r.ctx, &ts) == 0) {
			r.tot.ms_track[0] += ts.ms[0];
			r.tot.ms_track[1] += ts.ms[1];
		}
		ntedit_hip_spectrum_stats ss;
		if (r.opt.spectrum && ntedit_hip_spectrum_info(r.ctx, &ss) == 0) {
			r.tot.ms_spectrum[0] += ss.ms[0];
			r.tot.ms_spectrum[1] += ss.ms[1];
		}
		ntedit_hip_bgzf_stats bs;
		if (r.opt.bgzip && ntedit_hip_bgzf_info(r.ctx, &bs) == 0) {
			r.tot.add(bs);
		}
		r.write_q.push(w);
	}
	r.write_q.push(nullptr);
}

// One round: build or load the filter, echo the parameters, polish `draft`, write the three outputs under `prefix_in`;
// returns the name of the edited draft.  A run is one round, or with --reads -k K1,K2,...,Kn a cascade of n: round i + 1
// polishes round i's _edited.fa (through the file: 1/30 of the data, and every round stays byte-comparable with a
// stand-alone run), and from round 2 on every pass of the filter build reads the resident store that round 1 filled.
static std::string
polish_round(Run& run, const CliOptions& opt, size_t round, const std::string& draft, const std::string& prefix_in)
{
	ntedit_hip_ctx* ctx = run.ctx;
	const bool cascade = opt.rounds.size() > 1;
	const ntedit_hip_reads_rules& rr = opt.rounds[round];
	ntedit_hip_params p = opt.params;
	std::string prefix = prefix_in;
	// ---- the filter (with a list of k the names of the saved files carry {k}: this round's k goes there)
	const RoundNames names = { cascade ? nte_host::with_k(opt.hist, rr.k) : opt.hist,
		                       cascade ? nte_host::with_k(opt.save_bf, rr.k) : opt.save_bf,
		                       cascade ? nte_host::with_k(opt.save_reject_bf, rr.k) : opt.save_reject_bf };
	const FilterStage fs = opt.genome_mode  ? filter_from_genome(ctx, opt, names)
	                       : opt.reads_mode ? filter_from_reads(ctx, opt, round, names, &run.store_lost)
	                                        : filter_from_file(ctx, opt);
	// ---- the parameters
	Round r{ opt, ctx };
	int counting = 0;
	describe_filter(ctx, opt, fs.bf, &p, &r.k, &counting);
	echo_parameters(opt, p, r.k, counting, draft, fs, prefix);
	if (!fs.bfrep.empty()) {
		secondary_filter(ctx, fs.bfrep, rr.reject_cmin != 0, r.k);
	}
	prepare_device(run, opt, p, fs.store_held, round);

	// ---- the outputs (--report: from this stamp to "process complete")
	printf("---------- reading/processing input sequence        : %s", now_text());
	const Stopwatch run_clock;
	r.fa_path = prefix + (opt.bgzip ? "_edited.fa.gz" : "_edited.fa");
	r.tsv_path = prefix + "_changes.tsv";
	r.vcf_path = prefix + "_variants.vcf";
	r.qv_path = prefix + "_qv.tsv";
	r.bed_path[0] = prefix + "_absent_before.bed";
	r.bed_path[1] = prefix + "_absent_after.bed";
	r.spectrum_path[0] = prefix + "_spectrum.tsv";
	r.spectrum_path[1] = prefix + "_depth.tsv";
	open_outputs(r, p, counting, draft);

	// ---- the draft.  Plain multi-FASTA files are taken apart by several threads from a mapping of the file (fasta_map.h);
	// anything else (gzip, FASTQ, CR line ends, ...) goes through the streaming reader.  --no-map forces the latter.
	// (BGZF members are inflated before the parse: compute-bound, so on more threads than the memory-bound parse)
	const unsigned ingest_threads = threads_up_to(opt, 16) < 1 ? 1 : threads_up_to(opt, 16);
	r.tot.s_before_index = run_clock.s();
	const Stopwatch index_clock;
	nte_host::FastaMap fmap(opt.no_map ? "" : draft.c_str(), ingest_threads, threads_up_to(opt, 64));
	r.tot.s_index = index_clock.s();
	std::vector<uint8_t> mine; // --shard I/N: by ordinal, the contigs of this share
	if (opt.shard_n > 1) {
		mine = shard_partition(shard_lengths(fmap, draft, p.min_contig_len), opt.shard_n, opt.shard_i);
	}
	// (the streaming reader and its inflate thread only when the mapped reader does not serve the run)
	std::unique_ptr<nte_host::FastaReader> reader_p;
	if (!fmap.ok()) {
		reader_p.reset(new nte_host::FastaReader(draft.c_str()));
	}
	if (reader_p && !reader_p->ok()) {
		fail("`%s': cannot open", draft.c_str());
	}
	if (opt.shard_n > 1) {
		r.index_f = fopen((prefix + ".index.tsv").c_str(), "wb");
		if (!r.index_f) {
			fail("cannot write `%s.index.tsv'", prefix.c_str());
		}
		fprintf(r.index_f, "#shard %u/%u\tordinal\tfa_bytes\ttsv_bytes\tvcf_bytes\n", opt.shard_i, opt.shard_n);
	}
	if (opt.threads_given) {
		ntedit_hip_set_host_threads(opt.nthreads); // -t: contigs rendered concurrently
	}

	// ---- the pipeline.  Batch sizes: end to end the writer is the slowest stage (a write() per output byte into the page
	// cache), so the run takes the writer's time plus what passes before its first byte: unless the user fixes the size, the
	// first batches are small (128 Mbases, doubling: the writer starts after 30 ms instead of 120) and grow to 1 Gbase --
	// every batch costs the writer a start-up of its own (round 5: 3 Gbp in 7 batches of <= 512 Mbases 0.52 s of writer
	// time, in 3 of 1 Gbase 0.43 s).
	const unsigned long long batch_cap = opt.batch_given ? opt.batch_bases : 1ull << 30;
	const Admission admission(p.min_contig_len, opt.shard_n > 1 ? &mine : nullptr, opt.batch_given ? batch_cap : 1ull << 27, batch_cap);
	// Three stages, one batch each at a time: the reader parses the draft into batch N+1 while the GPU polishes batch N and
	// the writer renders batch N-1.  Output order = input order (the reference at -t 1).
	for (Work& w : run.pool) {
		r.free_q.push(&w);
	}
	run.pool.reserve_blobs((size_t)(batch_cap < (1ull << 32) ? batch_cap : (1ull << 32)) + (1 << 20));
	std::thread reader_thread([&r, &fmap, &reader_p, admission]() {
		if (fmap.ok()) {
			read_mapped(r, fmap, admission);
		} else {
			read_streamed(r, *reader_p, admission);
		}
	});
	std::thread writer_thread([&r]() { write_batches(r); });
	polish_batches(r);
	reader_thread.join();
	writer_thread.join();
	if (opt.bgzip) {
		uint32_t n_eof = 0;
		const uint8_t* eof = ntedit_hip_bgzf_eof(&n_eof);
		write_bgzf(r, eof, n_eof);
		if (close(r.fa_fd) != 0) {
			fail("cannot write `%s'", r.fa_path.c_str());
		}
	}
	for (int which = 0; which < 2; which++) {
		if (r.bed_f[which] && fclose(r.bed_f[which]) != 0) {
			fail("cannot write `%s'", r.bed_path[which].c_str());
		}
	}
	if (r.index_f && fclose(r.index_f) != 0) {
		fail("cannot write `%s.index.tsv'", prefix.c_str());
	}
	if (reader_p && reader_p->io_error()) {
		// a corrupt / truncated input must not pass for a (shorter) genome
		fail("`%s': %s -- the outputs are incomplete", draft.c_str(), reader_p->io_error_text().c_str());
	}
	r.tot.seconds = run_clock.s();
	printf("---------- process complete                         : %s", now_text());

	// ---- the summaries
	if (r.qv_f) {
		finish_qv(ctx, r.qv_f, r.qv_path, r.k, r.tot);
	}
	if (opt.completeness) {
		finish_completeness(ctx, prefix, r.k, opt.report != 0);
	}
	if (opt.bgzip) {
		finish_bgzip(r.tot, r.fa_path, opt.report != 0);
	}
	if (opt.bed) {
		finish_bed(r.tot, r.bed_path, opt.report != 0);
	}
	if (r.depth_f) {
		finish_spectrum(r.tot, r.depth_f, r.spectrum_path, r.k, opt.report != 0);
	}
	if (opt.cn) {
		const std::string cn_path[2] = { prefix + "_spectrum_cn.tsv", prefix + "_cn_contigs.tsv" };
		finish_cn(ctx, r.cn_names, cn_path, r.k, opt.cn_sketch, opt.report != 0);
	}
	if (opt.report && opt.qv) {
		report_qv(r.tot);
	}
	if (opt.report) {
		report_round(r.tot);
	}
	ntedit_hip_annot_free(r.annot);
	return r.fa_path;
}

int
main(int argc, char** argv)
{
	const CliOptions opt = parse_cli(argc, argv);
	ntedit_hip_ctx* ctx = nullptr;
	if (ntedit_hip_create(opt.gpu, &ctx) != 0) {
		fail("no usable HIP device %d (this build has no CPU path).", opt.gpu);
	}
	for (const auto& t : opt.tunes) {
		if (t.first == "host_zlib") {
			// (a host-side switch, not the library's: 1 = inflate .gz drafts through zlib instead of host/gunzip.cpp)
			nte_host::set_gzip_through_zlib((int)t.second);
			continue;
		}
		if (ntedit_hip_set_tuning(ctx, t.first.c_str(), t.second) != 0) {
			fail("%s", ntedit_hip_last_error(ctx));
		}
	}
	// every thread and batch buffer from here on: on the socket the GPU hangs off
	(void)ntedit_hip_bind_near_device(opt.gpu);
	BatchPool pool(opt.gpu, opt.batch_given ? opt.batch_bases : 1ull << 30, opt.draft, !(opt.no_map || getenv("NTEDIT_NO_PINNED_BATCHES")));
	Run run{ ctx, pool };
	std::string round_draft = opt.draft;
	for (size_t round = 0; round < opt.rounds.size(); round++) {
		// the last round writes under the prefix, an earlier one at Ki under <prefix>_k<Ki>
		const bool last_round = round + 1 == opt.rounds.size();
		round_draft = polish_round(run, opt, round, round_draft, last_round ? opt.prefix : opt.prefix + "_k" + std::to_string(opt.rounds[round].k));
	}
	pool.release();
	ntedit_hip_destroy(ctx);
	return 0;
}
