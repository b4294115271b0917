// reads_pass.cpp -- the host side of the reads k-mer filter build, shared by ntedit-make-reads-bf and the sharded driver
// (ntedit_amd/make_reads.py): one pass over a list of byte ranges of the input files, parsed by FastaReader into bounded
// batches double-buffered through page-locked memory (a second thread parses the next batch while the GPU works on the
// current one), or with --gpu_parse shipped raw or still compressed and parsed on the device; and the tool's sizing.  The
// feeds and the loop that overlaps their copies are chunk_feed.h's; the build that runs the passes is reads_build.cpp.
// With a reject cutoff pass 2 fills the SECONDARY slot too (the filter ntedit -e loads), from the same walk.
//
// A range [begin, end) of a file owns the records whose first byte lies in it.  A range that starts past byte 0 first
// moves forward to the first record start: a line that starts with '>' in a FASTA file, or in a FASTQ file a line that
// starts with '@' whose line + 2 starts with '+' (unambiguous for 4-line FASTQ).  The parser then runs with kseq's rules
// and stops before the first record that starts at or past `end`; where it stopped is reported (`nexts`), as is where
// the range started (`starts`).  Only when every range's stop is the next range's start did the ranges parse the file
// exactly as one reader would: the driver checks that after pass 1 (multi-line FASTQ can break it).  Gzip files are
// single units.
#include "../csrc/nte_reads_internal.h"
#include "chunk_feed.h"
#include "fasta.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include <sys/stat.h>

namespace {

using nte_host::Batch;
using nte_host::BgzfChunk;
using nte_host::BgzfProducer;
using nte_host::Feed;
using nte_host::RawChunk;
using nte_host::RawProducer;

const uint64_t WHOLE = ~0ull; // `end` of a range that runs to the end of its file

// default sketch: 16 output bytes' worth of counters, within [64 MiB, 32 GiB]; sized from the histogram (the output
// size not known yet): one counter per input byte, a gzip file counted at 4 x its size, within the same bounds
const uint64_t SKETCH_PER_OUTPUT_BYTE = 16;
const uint64_t SKETCH_MIN = 64ull << 20;
const uint64_t SKETCH_MAX = 32ull << 30;

int
pfail(const ntedit_hip_ctx* c, int code, const std::string& why)
{
	return nte_reads::set_error(c, code, why); // (ntedit_hip_reads_last_error's store, nte_reads.hip)
}

// what the head of the file says it is (chunk_feed.h: file_kind; a BGZF file is a gzip file too)
bool
is_gzip(const char* path)
{
	int first;
	return nte_host::file_kind(path, &first) != 0;
}

bool
is_bgzf(const char* path)
{
	int first;
	return nte_host::file_kind(path, &first) == 2;
}

// the first record start at or past `begin` (> 0) of a plain file, or its size when there is none
bool
find_record_start(const char* path, uint64_t begin, uint64_t* out, std::string* why)
{
	FILE* fp = fopen(path, "rb");
	if (!fp) {
		*why = std::string("cannot open ") + path;
		return false;
	}
	std::vector<char> buf(1 << 16);
	setvbuf(fp, buf.data(), _IOFBF, buf.size());
	// the file's kind: its first '>' or '@' (where kseq's first record starts)
	int c, kind = 0;
	while ((c = getc(fp)) != EOF) {
		if (c == '>' || c == '@') {
			kind = c;
			break;
		}
	}
	struct stat st;
	*out = fstat(fileno(fp), &st) == 0 ? (uint64_t)st.st_size : 0;
	if (!kind || fseeko(fp, (off_t)(begin - 1), SEEK_SET) != 0) {
		fclose(fp);
		return true;
	}
	// the first characters of the last three line starts at or past begin
	uint64_t at[3] = { 0, 0, 0 };
	int first[3] = { 0, 0, 0 }, n = 0;
	int prev = getc(fp);
	for (uint64_t p = begin;; p++) {
		c = getc(fp);
		if (prev == '\n') {
			if (kind == '>' && c == '>') {
				*out = p;
				break;
			}
			if (n == 3) {
				at[0] = at[1], at[1] = at[2], first[0] = first[1], first[1] = first[2];
				n = 2;
			}
			at[n] = p, first[n] = c, n++;
			if (n == 3 && first[0] == '@' && first[2] == '+') {
				*out = at[0];
				break;
			}
		}
		if (c == EOF) {
			break;
		}
		prev = c;
	}
	fclose(fp);
	return true;
}

// every record of one range, in order: seq_fn(record, its bases that had a quality, those of them masked) for each, the
// record masked by min_qual (0: off, and the two counts are 0); *start / *next as ntedit_hip_reads_pass reports them
using SeqFn = std::function<bool(const std::string&, uint64_t, uint64_t)>;

// what the reads passes ask of the host parser beyond kseq's rules: --min_qual, and the read filter (filter.min_len: the
// shortest record kept, the caller's k already in it).  A record the filter drops never reaches seq_fn; *counts (may be
// NULL) += what the records came to.  Only the reads passes set these: a draft or a genome is never filtered.
struct HostRules
{
	uint32_t min_qual = 0;
	nte_parse::ReadFilter filter = nte_parse::ReadFilter();
	nte_parse::ReadFilterCounts* counts = nullptr;
};

bool
read_range(const char* path, uint64_t begin, uint64_t end, const HostRules& rules, const SeqFn& seq_fn, uint64_t* start, uint64_t* next,
           std::string* why, bool exact = false, uint64_t skip = 0)
{
	uint64_t s = exact ? begin : 0; // exact: begin is a record start (where --gpu_parse hands a range back)
	if (skip) {
		// a whole gzip file from the inflated offset `skip`, a record start (where --gpu_parse hands a BGZF file back):
		// the bytes before it are inflated and dropped
		s = skip;
	}
	if (begin > 0 || end != WHOLE) {
		struct stat st;
		if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) {
			*why = std::string("cannot open ") + path + " (a range needs a regular file)";
			return false;
		}
		if (is_gzip(path)) {
			*why = std::string(path) + ": a gzip file is read whole, not in ranges";
			return false;
		}
		if (begin > 0 && !exact && !find_record_start(path, begin, &s, why)) {
			return false;
		}
	}
	*start = s;
	if (s >= end) {
		*next = s; // no record starts in the range
		return true;
	}
	nte_host::FastaReader reader(path, skip ? 0 : s, end);
	if (!reader.ok()) {
		*why = std::string("cannot open ") + path;
		return false;
	}
	reader.skip(skip);
	reader.set_min_qual(rules.min_qual);
	reader.set_read_filter(rules.filter);
	const bool filtered = nte_parse::rp_filter_on(rules.filter);
	std::string hdr, seq;
	for (;;) {
		seq.clear();
		if (!reader.next(hdr, seq)) {
			break;
		}
		if (filtered) {
			const unsigned why = reader.drop_reason();
			if (rules.counts) {
				rules.counts->records++;
				rules.counts->by_length += why == nte_parse::RP_DROP_LENGTH;
				rules.counts->by_mean_qual += why == nte_parse::RP_DROP_MEAN_QUAL;
			}
			if (why != nte_parse::RP_KEPT) {
				continue;
			}
		}
		if (!seq_fn(seq, reader.qual_bases(), reader.masked_bases())) {
			return false;
		}
	}
	if (reader.io_error()) {
		*why = std::string(path) + ": " + reader.io_error_text();
		return false;
	}
	*next = reader.next_start();
	return true;
}

struct Range
{
	const char* path;
	uint64_t begin, end;
	bool exact = false; // begin is a record start: no search for one
	uint64_t skip = 0;  // of a whole gzip file: the inflated offset, a record start, the records are taken from
};

// the host parser as a producer of batches (chunk_feed.h): every record of the ranges, in order
struct BatchProducer
{
	std::vector<Range> ranges;
	unsigned k;
	size_t batch_bytes;
	uint64_t *starts, *nexts;
	HostRules rules;       // (rules.counts: read once the feed has ended, like qual_counts)
	uint64_t* qual_counts; // [2], of the records kept: with a quality, masked (read once the feed has ended)

	void operator()(Feed<Batch>& feed) const
	{
		Batch* b = nte_host::batch_begin(feed);
		for (size_t i = 0; i < ranges.size(); i++) {
			if (!b) {
				return;
			}
			const Range& r = ranges[i];
			uint64_t start = 0, next = 0;
			bool stopped = false;
			std::string why;
			auto add = [&](const std::string& seq, uint64_t with_qual, uint64_t masked) {
				stopped = !nte_host::batch_add(feed, b, seq, k, batch_bytes);
				if (seq.size() >= k) { // (what batch_add keeps)
					qual_counts[0] += with_qual;
					qual_counts[1] += masked;
				}
				return !stopped;
			};
			const bool ok = read_range(r.path, r.begin, r.end, rules, add, &start, &next, &why, r.exact, r.skip);
			if (stopped) {
				return; // (batch_add failed the feed, or it is being torn down)
			}
			if (!ok) {
				feed.fail(why);
				return;
			}
			if (starts) {
				starts[i] = start;
			}
			if (nexts) {
				nexts[i] = next;
			}
		}
		if (b) {
			b->last = true;
			feed.put_full(b);
		}
	}
};

double
ms_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// one ntedit_hip_reads_pass: what its ranges share, and a range by each of the three ways it can take
struct Pass
{
	ntedit_hip_ctx* ctx;
	int pass;
	uint32_t cmin, rmin; // SOLID: the cutoff, and the reject cutoff when one is set (both slots are filled then)
	uint32_t keep;       // the shortest record the parsers keep: the sketch's k, or below it what ntedit_hip_reads_set_min_read asks for
	uint64_t batch_bytes;
	uint32_t min_qual;   // ntedit_hip_reads_set_min_qual (the host parser's part: the device parsers read the context's setting)
	nte_parse::ReadFilter filter; // ntedit_hip_reads_set_read_filter, alike
	uint64_t bases = 0;
	double gpu_ms = 0.0;
	ntedit_hip_reads_parse_stats* info;
	ntedit_hip_reads_inflate_stats* zinfo;
	ntedit_hip_reads_bam_stats* binfo;

	// one batch of text, host or device, through the pass's kernels
	int run_batch(const char* text, uint64_t len, int where) const
	{
		return pass == NTEDIT_READS_PASS_COUNT  ? ntedit_hip_sketch_count(ctx, text, len, where)
		       : pass == NTEDIT_READS_PASS_HIST ? ntedit_hip_sketch_histogram(ctx, text, len, where)
		       : rmin                           ? ntedit_hip_filter_insert_solid2(ctx, text, len, where, cmin, rmin)
		                                        : ntedit_hip_filter_insert_solid(ctx, NTEDIT_FILTER_PRIMARY, text, len, where, cmin);
	}

	// the host parser over some ranges (all of them, without --gpu_parse)
	int host_ranges(const std::vector<Range>& rs, uint64_t* rs_starts, uint64_t* rs_nexts)
	{
		uint64_t counts[2] = { 0, 0 };
		nte_parse::ReadFilterCounts fcounts = nte_parse::ReadFilterCounts();
		HostRules rules;
		rules.min_qual = min_qual;
		rules.filter = filter;
		rules.filter.min_len = nte_parse::rp_filter_on(filter) ? nte_parse::rp_min_len(filter, keep) : 0;
		rules.counts = &fcounts;
		Feed<Batch> feed(BatchProducer{ rs, keep, (size_t)batch_bytes, rs_starts, rs_nexts, rules, counts });
		for (;;) {
			Batch* b = feed.take();
			if (!b) {
				return pfail(ctx, NTEDIT_E_IO, feed.error());
			}
			const auto g0 = std::chrono::steady_clock::now();
			const int rc = b->len ? run_batch(b->buf.p, b->len, NTEDIT_HIP_BASES_HOST) : 0; // (an input without any read of k bases ends in an empty batch)
			if (rc) {
				return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
			}
			gpu_ms += ms_since(g0);
			bases += b->bases;
			const bool last = b->last;
			feed.give_back(b);
			if (last) {
				nte_reads::min_qual_count(ctx, 0, counts[0], counts[1]); // (the producer is through: its last batch came after them)
				nte_reads::read_filter_count(ctx, 0, &fcounts);
				return 0;
			}
		}
	}

	// --gpu_parse, a range of a plain file: raw chunks cut at record starts, parsed on the device.  From the first unclean
	// chunk on the rest of the range is the host parser's.
	int plain_range(const Range& r, uint64_t size, uint64_t* start_out, uint64_t* next_out)
	{
		// the range's first record start as the host parser finds it, and where its last chunk ends: the first
		// record start at or past `end` by the same rule
		uint64_t start = 0, stop = size;
		std::string why;
		if ((r.begin > 0 && !find_record_start(r.path, r.begin, &start, &why)) ||
		    (r.end < size && r.end > 0 && !find_record_start(r.path, r.end, &stop, &why))) {
			return pfail(ctx, NTEDIT_E_IO, why);
		}
		if (start_out) {
			*start_out = start;
		}
		if (start >= r.end || start >= size) {
			if (next_out) {
				*next_out = start; // no record starts in the range
			}
			return 0;
		}
		uint64_t handed_back = WHOLE; // where an unclean chunk started
		{
			Feed<RawChunk> feed(RawProducer{ r.path, start, stop, (size_t)batch_bytes, nte_host::CUT_RECORDS });
			auto begin = [&](const RawChunk& c, int which) {
				return nte_reads::parse_copy_begin(ctx, which, c.buf.p, c.len) != 0 ? NTEDIT_E_DEVICE : 0;
			};
			auto work = [&](const RawChunk& c, int which, auto release) {
				const auto g0 = std::chrono::steady_clock::now();
				const char* text = nullptr;
				ntedit_hip_reads_parse_result res;
				int rc = nte_reads::parse_copied(ctx, which, c.len, keep, &text, &res);
				const uint64_t off = c.off, len = c.len;
				if (rc == 0) {
					release(); // (its copy is done: the reader may fill it again)
				}
				if (rc == 0 && res.clean && res.text_len) {
					rc = run_batch(text, res.text_len, NTEDIT_HIP_BASES_DEVICE);
				}
				if (rc) {
					return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
				}
				gpu_ms += ms_since(g0);
				if (!res.clean) {
					info->fallback_chunks++;
					info->broken |= res.broken;
					handed_back = off;
					return (int)nte_host::OVERLAP_STOP;
				}
				info->device_chunks++;
				info->raw_bytes += len;
				info->text_bytes += res.text_len;
				bases += res.bases;
				return 0;
			};
			const int rc = nte_host::overlap(feed, begin, work, [&](int which) { return nte_reads::parse_copy_wait(ctx, which); });
			if (rc != 0 && rc != nte_host::OVERLAP_STOP) {
				return rc == nte_host::OVERLAP_FEED ? pfail(ctx, NTEDIT_E_IO, feed.error()) : rc;
			}
		}
		if (handed_back != WHOLE) {
			// the rest of the range, from that chunk's first byte, with kseq's rules
			Range rest = r;
			rest.begin = handed_back;
			rest.exact = true;
			return host_ranges({ rest }, nullptr, next_out);
		}
		if (next_out) {
			*next_out = stop;
		}
		return 0;
	}

	// --gpu_parse, a BGZF file, whole: shipped compressed, inflated and cut on the device.  `base` is the inflated offset
	// of the raw buffer's first byte, always a record start; `tail` the bytes carried behind a cut.
	// A BAM takes the same loop: its walk in place of the last record start, its decode in place of the text parser.
	// There is no host parser to hand it back to: what the BGZF path hands back fails the pass.
	int bgzf_file(const Range& r, uint64_t* start_out, uint64_t* next_out)
	{
		zinfo->files++;
		const bool bam = ntedit_hip_reads_is_bam(r.path) != 0;
		bool bam_header_done = false;
		auto bam_fail = [&](const std::string& what, uint64_t at) {
			return pfail(ctx, NTEDIT_E_IO, std::string(r.path) + ": BAM: " + what + " at inflated offset " + std::to_string(at));
		};
		if (bam) {
			binfo->files++;
		}
		uint64_t base = 0, tail = 0;
		bool handed_back = false;
		{
			Feed<BgzfChunk> feed(BgzfProducer{ r.path, (size_t)batch_bytes });
			auto begin = [&](const BgzfChunk& c, int which) {
				return nte_reads::inflate_copy_begin(ctx, which, c.buf.p, c.len, c.m(), c.n_members) != 0 ? NTEDIT_E_DEVICE : 0;
			};
			auto work = [&](const BgzfChunk& c, int which, auto release) {
				const auto g0 = std::chrono::steady_clock::now();
				const char* raw = nullptr;
				uint64_t bad = 0, cut = 0;
				uint32_t reason = 0, broken = 0;
				int rc = nte_reads::inflate_copied(ctx, which, c.len, c.m(), c.n_members, tail, c.n_out, &raw, &bad, &reason);
				const uint64_t total = tail + c.n_out, first_member = c.first_member;
				const bool last = c.last, whole = c.whole;
				if (rc == 0) {
					release(); // (its copy is done: the reader may fill it again)
				}
				if (rc == 0 && reason) {
					zinfo->bad_member = first_member + bad;
					zinfo->bad_reason = reason;
					return pfail(ctx, NTEDIT_E_IO, std::string(r.path) + ": BGZF member " + std::to_string(first_member + bad) +
					                                   " is damaged (" + nte_reads::inflate_reason(reason) + ")");
				}
				// the chunk's cut: the end of the file's bytes, else the last record start on the device
				if (rc == 0 && !bam) {
					if (last && whole) {
						cut = total;
					} else {
						rc = nte_reads::inflate_last_start(ctx, raw, total, &cut, &broken);
					}
				}
				ntedit_hip_reads_parse_result res = ntedit_hip_reads_parse_result();
				res.clean = 1;
				const char* text = nullptr;
				ntedit_hip_reads_bam_result bres = ntedit_hip_reads_bam_result();
				if (rc == 0 && bam) {
					// the first record that does not lie completely inside is the cut; the records before it are the text
					rc = nte_reads::bam_buffer(ctx, raw, total, bam_header_done ? 0 : 1, keep, &text, &bres);
					res.clean = bres.clean;
					res.text_len = bres.text_len;
					res.bases = bres.bases;
					cut = bres.cut;
				} else if (rc == 0 && broken) {
					res.clean = 0;
					res.broken = broken;
				} else if (rc == 0 && cut) {
					rc = nte_reads::parse_buffer(ctx, raw, cut, keep, &text, &res);
				}
				if (rc == 0 && res.clean && res.text_len) {
					rc = run_batch(text, res.text_len, NTEDIT_HIP_BASES_DEVICE);
				}
				if (rc) {
					return pfail(ctx, rc, ntedit_hip_reads_last_error(ctx));
				}
				gpu_ms += ms_since(g0);
				if (bam && !res.clean) {
					return bam_fail(bres.broken & NTEDIT_BAM_BAD_MAGIC    ? "the header does not start with the BAM magic"
					                : bres.broken & NTEDIT_BAM_BAD_HEADER ? "a header with a negative length or an empty reference name"
					                : bres.broken & NTEDIT_BAM_BAD_SIZE   ? "a record with a block_size outside [0, 2^30), or a chunk of 2 GiB"
					                                                      : "a record whose parts do not fit its block_size",
					                base + bres.cut);
				}
				if (!res.clean) {
					info->fallback_chunks++;
					info->broken |= res.broken;
					handed_back = true;
					return (int)nte_host::OVERLAP_STOP;
				}
				if (cut && !bam) { // (a BAM's chunks are the BAM counters': the text parser saw none of them)
					info->device_chunks++;
					info->raw_bytes += cut;
					info->text_bytes += res.text_len;
				}
				if (cut) {
					bases += res.bases;
				}
				// a chunk without a record start past its first byte grows by the next one (cut = 0: all is tail)
				if (cut && cut < total && nte_reads::inflate_carry(ctx, cut, total) != 0) {
					return NTEDIT_E_DEVICE;
				}
				base += cut;
				tail = total - cut;
				bam_header_done = bam_header_done || cut > 0; // (a header that does not fit gives cut 0)
				if (bam && last && !whole) {
					return bam_fail("what follows the last whole BGZF member is not one (a damaged or truncated file); the records end", base);
				}
				if (bam && last && tail) {
					return bam_fail(std::to_string(tail) + " bytes are left over behind the last whole record (a truncated file)", base);
				}
				if (last && !whole) {
					handed_back = true; // what follows the members is not BGZF: the host parser's, from `base`
				}
				return 0;
			};
			const int rc = nte_host::overlap(feed, begin, work, [&](int which) { return nte_reads::inflate_copy_wait(ctx, which); });
			if (rc != 0 && rc != nte_host::OVERLAP_STOP) {
				return rc == nte_host::OVERLAP_FEED ? pfail(ctx, NTEDIT_E_IO, feed.error()) : rc;
			}
		}
		if (start_out) {
			*start_out = 0;
		}
		if (handed_back) {
			zinfo->handed_back++;
			zinfo->handed_back_at = base;
			Range rest = r;
			rest.skip = base;
			return host_ranges({ rest }, nullptr, next_out);
		}
		if (next_out) {
			*next_out = base;
		}
		return 0;
	}
};

} // namespace

extern "C" {

uint64_t
ntedit_hip_reads_last_record_start(const char* buf, uint64_t n, int kind)
{
	const size_t at = buf ? nte_host::last_record_start(buf, (size_t)n, kind) : nte_host::NO_CUT;
	return at == nte_host::NO_CUT ? NTEDIT_READS_NO_START : (uint64_t)at;
}

int
ntedit_hip_reads_pass(ntedit_hip_ctx* ctx, int pass, const char* const* files, const uint64_t* begins, const uint64_t* ends,
                      uint32_t n, uint64_t batch_bytes, uint32_t cmin, ntedit_hip_reads_pass_stats* stats,
                      uint64_t* starts, uint64_t* nexts)
{
	if (!ctx || (n && (!files || !begins || !ends)) || batch_bytes < 4096 ||
	    (pass != NTEDIT_READS_PASS_COUNT && pass != NTEDIT_READS_PASS_HIST && pass != NTEDIT_READS_PASS_SOLID)) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_pass: bad argument");
	}
	std::vector<Range> ranges(n);
	for (uint32_t i = 0; i < n; i++) {
		if (!files[i] || begins[i] > ends[i]) {
			return pfail(ctx, NTEDIT_E_ARG, "reads_pass: bad range " + std::to_string(i));
		}
		ranges[i] = Range{ files[i], begins[i], ends[i] };
	}
	uint64_t counters = 0;
	uint32_t hash_num = 0, k = 0;
	if (ntedit_hip_sketch_info(ctx, &counters, &hash_num, &k) != 0) {
		return pfail(ctx, NTEDIT_E_ARG, "reads_pass: no sketch (ntedit_hip_sketch_alloc / _set_device)");
	}
	const auto t0 = std::chrono::steady_clock::now();
	Pass p{ ctx, pass, cmin, pass == NTEDIT_READS_PASS_SOLID ? nte_reads::reject_cutoff(ctx) : 0, nte_reads::min_read(ctx, k), batch_bytes,
		    nte_reads::min_qual(ctx), nte_reads::read_filter(ctx) };
	nte_reads::min_qual_count(ctx, 1, 0, 0);
	nte_reads::read_filter_count(ctx, 1, nullptr);
	if (!nte_reads::parse_is_on(ctx)) {
		for (const Range& r : ranges) { // (the host parser would read whatever '@' and '>' bytes the binary stream holds)
			if (ntedit_hip_reads_is_bam(r.path)) {
				return pfail(ctx, NTEDIT_E_ARG, std::string("--reads ") + r.path + ": BAM needs --gpu_parse");
			}
		}
		const int rc = p.host_ranges(ranges, starts, nexts);
		if (rc) {
			return rc;
		}
	} else {
		*(p.info = nte_reads::parse_info(ctx)) = ntedit_hip_reads_parse_stats();
		*(p.zinfo = nte_reads::inflate_info(ctx)) = ntedit_hip_reads_inflate_stats();
		*(p.binfo = nte_reads::bam_info(ctx)) = ntedit_hip_reads_bam_stats();
		for (uint32_t i = 0; i < n; i++) {
			const Range& r = ranges[i];
			uint64_t* const start = starts ? starts + i : nullptr;
			uint64_t* const next = nexts ? nexts + i : nullptr;
			struct stat sb;
			const bool regular = stat(r.path, &sb) == 0 && S_ISREG(sb.st_mode);
			int rc;
			if (regular && r.begin == 0 && r.end == WHOLE && is_bgzf(r.path)) {
				rc = p.bgzf_file(r, start, next);
			} else if (regular && ntedit_hip_reads_is_bam(r.path)) {
				return pfail(ctx, NTEDIT_E_ARG, std::string(r.path) + ": a BAM file is read whole, not in ranges");
			} else if (!regular || is_gzip(r.path)) { // a gzip file (or what the host parser will refuse in its own words)
				p.info->host_files++;
				rc = p.host_ranges({ r }, start, next);
			} else {
				rc = p.plain_range(r, (uint64_t)sb.st_size, start, next);
			}
			if (rc) {
				return rc;
			}
		}
	}
	if (stats) {
		stats->bases = p.bases;
		stats->ms_wall = ms_since(t0);
		stats->ms_gpu = p.gpu_ms;
	}
	return 0;
}

int
ntedit_hip_reads_range_text(const char* path, uint64_t begin, uint64_t end, char* out, uint64_t cap, uint64_t* len,
                            uint64_t* reads, uint64_t* start, uint64_t* next)
{
	return ntedit_hip_reads_range_text_q(path, begin, end, 0, out, cap, len, reads, start, next);
}

int
ntedit_hip_reads_range_text_q(const char* path, uint64_t begin, uint64_t end, uint32_t min_qual, char* out, uint64_t cap, uint64_t* len,
                              uint64_t* reads, uint64_t* start, uint64_t* next)
{
	return ntedit_hip_reads_range_text_f(path, begin, end, min_qual, 0, 0, out, cap, len, reads, start, next, nullptr);
}

int
ntedit_hip_reads_range_text_f(const char* path, uint64_t begin, uint64_t end, uint32_t min_qual, uint32_t min_len, uint32_t min_mean_qual,
                              char* out, uint64_t cap, uint64_t* len, uint64_t* reads, uint64_t* start, uint64_t* next,
                              ntedit_hip_reads_read_filter_stats* st)
{
	HostRules rules;
	if (!path || !len || !reads || !start || !next || begin > end || (cap && !out) || min_qual > 93 ||
	    !nte_parse::rp_make_filter(min_len, min_mean_qual, 0.0f, &rules.filter)) { // (rq is a BAM field: the host parser reads none)
		return pfail(nullptr, NTEDIT_E_ARG, "reads_range_text: bad argument");
	}
	uint64_t used = 0, count = 0;
	std::string why;
	nte_parse::ReadFilterCounts fcounts = nte_parse::ReadFilterCounts();
	rules.min_qual = min_qual;
	rules.counts = &fcounts;
	static_assert(sizeof(ntedit_hip_reads_read_filter_stats) == sizeof(nte_parse::ReadFilterCounts), "field for field");
	const bool ok = read_range(path, begin, end, rules, [&](const std::string& seq, uint64_t, uint64_t) {
		if (used + seq.size() + 1 <= cap) {
			memcpy(out + used, seq.data(), seq.size());
			out[used + seq.size()] = '\n';
		}
		used += seq.size() + 1;
		count++;
		return true;
	}, start, next, &why);
	if (!ok) {
		return pfail(nullptr, NTEDIT_E_IO, why);
	}
	*len = used;
	*reads = count;
	if (st) {
		memcpy(st, &fcounts, sizeof fcounts);
	}
	return used > cap ? NTEDIT_E_OVERFLOW : 0;
}

// as ntedit-make-genome-bf (ntedit_make_genome_bf.cpp:41-47)
uint64_t
ntedit_hip_reads_bf_size(uint64_t num_elements, uint32_t hash_num, double fpr)
{
	const double h = (double)hash_num;
	const double r = -h / log(1.0 - exp(log(fpr) / h));
	return (uint64_t)(ceil((double)num_elements * r) / 8u);
}

uint64_t
ntedit_hip_reads_default_sketch(const char* const* files, uint32_t n, uint64_t bf_bytes)
{
	uint64_t counters = 0;
	if (bf_bytes) {
		counters = bf_bytes > SKETCH_MAX / SKETCH_PER_OUTPUT_BYTE ? SKETCH_MAX : bf_bytes * SKETCH_PER_OUTPUT_BYTE;
	} else {
		// an input that cannot be read counts 0 here and fails in pass 1
		for (uint32_t i = 0; i < n; i++) {
			struct stat st;
			if (!files || !files[i] || stat(files[i], &st) != 0 || !S_ISREG(st.st_mode)) {
				continue;
			}
			counters += (uint64_t)st.st_size * (is_gzip(files[i]) ? NTEDIT_READS_GZIP_WEIGHT : 1);
		}
		counters = counters > SKETCH_MAX ? SKETCH_MAX : counters;
	}
	return counters < SKETCH_MIN ? SKETCH_MIN : counters;
}

int
ntedit_hip_reads_is_gzip(const char* path)
{
	return path && is_gzip(path) ? 1 : 0;
}

} // extern "C"
